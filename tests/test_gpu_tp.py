"""The general tensor-product kernels (csrc/xeq_tp.hip: k_tp_path, k_tp_fused, k_tp_tied, k_tp_wgrad behind tp.TensorProduct) at their
tile and lane edges, in f64 and f32, against oracle/tp_oracle.py in f64 (tests/tp_cases.py holds the cases, the references and the
bounds; tests/test_tp_cases_host.py shows that the bounds reject every defect of its list):

  tile form   node tiles 1, 2, 4, 8, 16 from the default start and 5, 3 from an LDS-limited one, each above 1 with a partial last tile;
              output multiplicities 1, 4, 5 around the blocks of four w; shared weights and a set per row; 'uvuv' into 16 blocks
  tied form   1, 63, 64, 65, 129 channels (one, two and three lane rounds) at 1, 3, 4, 5, 9 rows (a wave per node, four per workgroup);
              'uuw' m -> 1 and m -> 3, 'uvu' and 'uvv' with unequal multiplicities; l up to 4
  weight gradient   one chunk, two, three, 512 full ones, 512 with seven empty ones; two gridDim.y pieces

Every input sits between guard bands and every allocation of the pass comes from ``guard_allocations()``: ``out`` and the input
gradients as zeros between bands, the parts buffer of the weight gradient holding the never-written pattern.

Bounds per output (tp_cases.judge): f64 1e-12 of the largest entry for values, 1e-11 for gradients; f32 max(4 x the f32 oracle's own
error against the f64 oracle, 4 ulp of the largest entry).  Every figure is printed before it is asserted (``tp-parity`` lines;
profiles/tp_parity.txt is their record)."""
import pytest
import torch

from tests import guard_bands as gb, tp_cases as tc
from xequinet_amd import lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPE = {"f64": torch.float64, "f32": torch.float32}
ESIZE = {"f64": 8, "f32": 4}


def _in(t, dtype, grad=False):
    return None if t is None else gb.guarded_copy(t.to(dtype).to(DEV).contiguous()).requires_grad_(grad)


def _forms(mod, b, x, y, G):
    """The form of every pass as the library's query states it for the tensors of the run."""
    res = {}
    for kind, (p, q) in {"fwd": (x, y), "dx1": (G, y), "dx2": (x, G)}.items():
        if kind != "fwd" and not b.grads:
            continue
        t = mod._fused_table(kind, x)
        f = 0 if t is None else mod.pass_form(t, p, q)
        res[kind] = ("tied", 0) if f == -1 else ("tile", f) if f > 0 else ("path", 0)
    return res


def _run(b, prec, fused=True, forms=None):
    """The module of the case on the GPU -> name -> tensor on the CPU; ``forms``: a dict that receives the form of every pass."""
    dtype = DTYPE[prec]
    mod = tc.module(b).to(DEV)
    mod.fused = fused
    x, y, w, G = _in(b.x, dtype, b.grads), _in(b.y, dtype, b.grads), _in(b.w, dtype, b.grads), _in(b.G, dtype)
    if forms is not None:
        forms.update(_forms(mod, b, x, y, G))
        assert forms == tc.forms(b, ESIZE[prec]), (b.name, forms)
    first = lib.launch_count()
    with gb.guard_allocations():
        out = mod(x, y, w)
        grads = torch.autograd.grad(out, [v for v in (x, y, w) if v is not None], G) if b.grads else ()
    gb.check(*[v for v in (x, y, w, G) if v is not None])
    names = lib.launch_names(first)
    if forms is not None and fused:         # the launches are the forms': one per fused pass, one per instruction otherwise
        want_fused = sum(f != "path" for f, _ in forms.values())
        assert names.count("xeq_tensor_product") == want_fused and names.count("xeq_tensor_product_path") == (len(forms) - want_fused) * len(b.ins)
    assert out.shape == (b.n, b.out.dim)
    return {k: v.detach().cpu() for k, v in zip(tc.outputs(b), (out, *grads))}


class _Record:
    """Every figure of one test, printed as it comes; failures asserted at the end."""

    def __init__(self):
        self.failed = []

    def add(self, b, prec, forms, res):
        tag = "/".join(f"{f}{tn if f == 'tile' else ''}" for f, tn in forms.values())
        for k, err, e32, bound, top in res:
            print(f"tp-parity {b.name} {prec} {tag} {k}: kernel {err:.3e} oracle32 {e32:.3e} kernel/oracle32 {err / max(e32, 1e-300):.2f} largest {top:.3e} "
                  f"bound {bound:.3e} kernel/bound {err / bound:.3f}")
            if not err <= bound:
                self.failed.append((b.name, prec, k, err, e32, bound))

    def close(self):
        assert not self.failed, self.failed


def _sweep(cases):
    rec = _Record()
    for c in cases:
        b = tc.build(c)
        for prec in c.dtypes:
            forms = {}
            got = _run(b, prec, forms=forms)
            rec.add(b, prec, forms, tc.judge(b.ref, b.ref32, got, tc.outputs(b), prec == "f64"))
    rec.close()


_TILE = [c.name for c in tc.tagged("tile") if "coeff" not in c.tags]
_TIED = sorted({c.name.rsplit("-m", 1)[0] for c in tc.tagged("tied") if not {"l4", "coeff"} & set(c.tags)})


@pytest.mark.parametrize("name", _TILE)
def test_tile_form_against_the_f64_oracle(name):
    _sweep([tc.by_name(name)])


@pytest.mark.parametrize("sweep", _TIED)
def test_tied_form_against_the_f64_oracle(sweep):
    """One product at 1, 63, 64, 65, 129 channels x 1, 3, 4, 5, 9 rows."""
    cases = [c for c in tc.tagged("tied") if c.name.rsplit("-m", 1)[0] == sweep]
    assert len(cases) == len(tc.TIED_MULS) * len(tc.TIED_ROWS)
    _sweep(cases)


@pytest.mark.parametrize("name", [c.name for c in tc.cases() if {"l4", "coeff"} & set(c.tags)])
def test_reference_products_and_unequal_path_weights(name):
    """The self-mix product (l up to 4) and the Cartesian-tensor head at 65 channels; paths with different coefficients into one block."""
    _sweep([tc.by_name(name)])


@pytest.mark.parametrize("name", [c.name for c in tc.tagged("wgrad")])
def test_weight_gradient_chunks_and_grid_pieces(name):
    _sweep([tc.by_name(name)])


# ------------------------------------------------------------------------------------------------------------------ written outputs
def _holes(c):
    """The case with a block in front of and a block behind its output irreps that no path ends in."""
    return tc.make(c.name + "-holes", c.in1, c.in2, None, c.mode, c.weights, c.n, out=f"2x1e+{c.out!r}+3x0e",
                   ins=[(i1, i2, io + 1, *rest) for i1, i2, io, *rest in c.ins])


@pytest.mark.parametrize("name", ["uvw-m145-shared-n16370", "uvuv-n16370", "uuu-shared-m65-n5", "uuw-sample-o3-m65-n5"])
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_every_block_a_path_ends_in_is_written_and_no_other(name, prec):
    """_run_fused on an ``out`` that holds the never-written pattern: k_tp_fused on blocks of four w and on single elements, k_tp_tied with
    the output tied to the lane and summed over the lanes."""
    c = _holes(tc.by_name(name))
    x, y, w, _ = tc.inputs(c)
    dtype = DTYPE[prec]
    mod = tc.module(c).to(DEV)
    x, y, w = _in(x, dtype), _in(y, dtype), _in(w, dtype)
    out = gb.guarded((c.n, c.out.dim), dtype, DEV, body="unwritten")
    t = mod._fused_table("fwd", x)
    assert mod.pass_form(t, x, y) == (-1 if tc.form(c, "fwd", ESIZE[prec])[0] == "tied" else 16)
    mod._run_fused(t, x, y, w, out)
    torch.cuda.synchronize()
    gb.check(out, x, y, *([w] if w is not None else []))
    blk = tc.block_of(c.out)
    untouched = ((blk == 0) | (blk == len(c.out) - 1)).to(DEV)
    assert bool(gb.unwritten(out)[:, untouched].all()), "a block without a path was written"
    assert not bool(gb.unwritten(out)[:, ~untouched].any()), ("unwritten", int(gb.unwritten(out)[:, ~untouched].sum()))
    assert bool(torch.isfinite(out[:, ~untouched]).all())


# ---------------------------------------------------------------------------------------------------------------- row independence
@pytest.mark.parametrize("name,row", [("uvw-s145-sample-n16370", 16 * 500 + 7), ("uvw-m145-shared-n16370", 16 * 1023),
                                       ("uuw-sample-o3-m65-n9", 5), ("uuu-shared-m129-n9", 6)])
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_a_row_of_out_depends_on_its_own_row_of_the_inputs_alone(name, row, prec):
    """Another row ``row`` of x1, x2 (and of per-sample weights) changes that row of ``out`` and no bit of any other: a row in the middle
    of a tile of 16, a row of the partial last tile, a wave in the middle of a workgroup."""
    c = tc.by_name(name)
    b = tc.build(c)
    dtype = DTYPE[prec]
    mod = tc.module(c).to(DEV)
    x, y, w = (None if v is None else v.to(dtype).to(DEV) for v in (b.x, b.y, b.w))
    assert tc.form(c, "fwd", ESIZE[prec]) in (("tile", 16), ("tied", 0)) and 0 < row < c.n - 1
    with torch.no_grad():
        base = mod(x, y, w)
        x2, y2 = x.clone(), y.clone()
        x2[row], y2[row] = x[row - 1], -y[row + 1]
        w2 = w
        if c.weights == "sample":
            w2 = w.clone()
            w2[row] = w[row - 1] * 0.5
        moved = mod(x2, y2, w2)
    others = torch.arange(c.n, device=DEV) != row
    assert torch.equal(base[others], moved[others]) and not torch.equal(base[row], moved[row])


# ------------------------------------------------------------------------------------------------- one launch against one per path
@pytest.mark.parametrize("name", ["uvw-m6-shared-n2047", "uvw-m6-shared-n4094", "uvw-m6-shared-n8186", "uvw-m6-shared-n16370",
                                  "uvw-m145-pad-n5118", "uvw-m145-pad-n3071", "uvw-m145-sample-n2047"])
def test_all_paths_in_one_launch_equal_one_launch_per_path_on_tiles_above_one(name):
    """tests/test_tp.py::test_all_paths_in_one_launch_equal_one_launch_per_path where the node tile is 2, 4, 8, 16, 5 and 3, in f64."""
    b = tc.build(tc.by_name(name))
    forms = {}
    fused = _run(b, "f64", forms=forms)
    assert forms["fwd"][0] == "tile" and forms["fwd"][1] > 1
    per_path = _run(b, "f64", fused=False)
    for k in tc.outputs(b):
        assert float((fused[k] - per_path[k]).abs().max()) <= 1e-12 * max(1.0, float(per_path[k].abs().max())), k


# ---------------------------------------------------------------------------------------------------------------- reproducibility
@pytest.mark.parametrize("prec", ["f64", "f32"])
def test_shared_weight_gradient_is_reproducible_and_is_the_sum_over_rows(prec):
    """32 769 rows: 512 chunks of 65 rows, seven of them empty.  Two runs give the same bits; the value is the f64 sum over the rows of
    the per-row weight gradient (the oracle with the weights copied to every row)."""
    c = tc.by_name("wgrad-uuu-m2-shared-n32769")
    b = tc.build(c)
    assert tc.chunk_plan(c.n, True) == (512, 65, 7)
    one, two = _run(b, prec), _run(b, prec)
    assert torch.equal(one["grad_w"], two["grad_w"])
    per_row = tc.make("per-row", c.in1, c.in2, None, c.mode, "sample", c.n, ins=c.ins, out=c.out)
    rows = tc.oracle(per_row, b.x, b.y, b.w.expand(c.n, -1).contiguous(), b.G, torch.float64)["grad_w"]
    want = {"grad_w": rows.sum(0)}
    assert float((want["grad_w"] - b.ref["grad_w"]).abs().max()) <= 1e-12 * float(want["grad_w"].abs().max())
    rec = _Record()
    rec.add(b, prec, {"wgrad": ("sum-over-rows", 0)}, tc.judge(want, b.ref32, one, ("grad_w",), prec == "f64"))
    rec.close()


# ------------------------------------------------------------------------------------------------------------------------- limits
@pytest.mark.parametrize("name", [c.name for c in tc.tagged("limit")])
def test_products_beyond_the_fused_kernels_limits_run_one_launch_per_path_and_match_the_oracle(name):
    """17 written blocks, 41 paths, rows that do not fit the LDS tile: the forward pass is one xeq_tensor_product_path launch per
    instruction (and so is every reverse pass the same limit holds for: _run counts them), and all outputs match the oracle."""
    c = tc.by_name(name)
    b = tc.build(c)
    rec = _Record()
    for prec in c.dtypes:
        forms = {}
        got = _run(b, prec, forms=forms)
        assert forms["fwd"] == ("path", 0)
        rec.add(b, prec, forms, tc.judge(b.ref, b.ref32, got, tc.outputs(b), prec == "f64"))
        mod = tc.module(c).to(DEV)
        x, y, w = (v.to(DTYPE[prec]).to(DEV) for v in (b.x, b.y, b.w))
        first = lib.launch_count()
        with torch.no_grad():
            mod(x, y, w)
        assert lib.launch_names(first) == ["xeq_tensor_product_path"] * len(c.ins)
    rec.close()


def test_the_fused_entry_refuses_what_its_limits_exclude_and_launches_nothing():
    """xeq_tensor_product itself: 41 paths, 17 blocks, rows beyond the LDS tile -- its own error through lib.call, no launch."""
    for name, message in (("limit-41-paths-n5", "at most 40 paths"), ("limit-17-blocks-n5", "at most 16 blocks"), ("limit-lds-n3", "do not fit the LDS tile")):
        c = tc.by_name(name)
        b = tc.build(c)
        mod = tc.module(c).to(DEV)
        assert mod._fused_table("fwd", torch.empty(0, dtype=torch.float64, device=DEV)) is None or name == "limit-lds-n3"
        mod.MAX_FUSED_PATHS = mod.MAX_FUSED_SLOTS = 64          # (on this instance: let the table be built, so that the entry is asked)
        mod._fused.clear()
        x, y, w = (v.to(DEV) for v in (b.x, b.y, b.w))
        out = torch.zeros((c.n, c.out.dim), dtype=torch.float64, device=DEV)
        first = lib.launch_count()
        with pytest.raises(RuntimeError, match=message):
            mod._run_fused(mod._fused_table("fwd", x), x, y, w, out)
        assert lib.launch_count() == first and not bool(out.any())
