"""The C entry points of csrc/xeq_painn.hip, called directly (lib.call / lib.ptr, as nn/painn.py calls them) at every width, basis
count, radial kind, envelope and list kind that ``xeq_painn_supported`` admits, against the f64 references of
tests/painn_kernel_cases.py.  ``h`` (the scalar MLP's output) and ``a`` (the update MLP's output) are random inputs, so no case needs
the 128-wide MLP kernels.

Every input sits between NaN guard bands (a read past the end poisons a result), every output is handed over holding the
never-written pattern between bands of its own; after the run the bands are compared bit for bit and every output the call was asked to
fill must hold no never-written word.

Bound per output tensor: tests/test_gpu_painn.py::_bound, max(1e-4 max(1, max|ref|), 1.5 err32), err32 the distance of the same
reference evaluated in f32 on the CPU from its f64 value.  tests/test_painn_kernel_cases_host.py shows that every defect of its list
moves the reference by at least 10 x that bound.  The worst error per family and width goes to the parity record."""
import numpy as np
import pytest
import torch

from tests import guard_bands as gb, painn_kernel_cases as pc, painn_oracle as po, parity_record
from xequinet_amd import lib
from xequinet_amd.lib import call, ptr, stream

pytestmark = pytest.mark.gpu

DEV = "cuda"
WIDTHS = (32, 64, 96, 128, 160, 192, 224, 256)
WORST = {}   # (family, F) -> (err / bound, err, bound, output, case)


@pytest.fixture(scope="module", autouse=True)
def _parity_records():
    yield
    for (family, F), (ratio, err, bnd, name, case) in sorted(WORST.items()):
        parity_record.add({"test": f"painn:kernels:{family}:F={F}", "err": err, "bound": bnd, "err_over_bound": ratio, "output": name, "case": case})


def _compare(family, F, case, got, ref, ref32, names):
    """every named output against the f64 reference under the project's bound; the family's worst goes to the record"""
    failed = []
    for k in names:
        assert torch.isfinite(got[k]).all(), (case, k)
        err, bnd = float((got[k].double() - ref[k]).abs().max()), pc.bound(ref[k], ref32[k])
        print(f"{family} F={F} {case} {k}: err {err:.3e} bound {bnd:.3e}")
        if (family, F) not in WORST or err / bnd > WORST[(family, F)][0]:
            WORST[(family, F)] = (err / bnd, err, bnd, k, case)
        if not err <= bnd:
            failed.append((k, err, bnd))
    assert not failed, (family, F, case, failed)


def _in(t, dtype=torch.float32):
    """an input between NaN bands"""
    if t is None:
        return None
    t = torch.as_tensor(t)
    return gb.guarded_copy(t.to(dtype).to(DEV).contiguous())


def _out(*shape):
    return gb.guarded(shape, torch.float32, DEV, body="unwritten")


def _finish(inputs, filled, untouched=()):
    """bands of everything, no never-written word in what the call was asked to fill, nothing but that word in what it was not"""
    torch.cuda.synchronize()
    gb.check(*[t for t in list(inputs) + list(filled) + list(untouched) if t is not None])
    for t in filled:
        assert not bool(gb.unwritten(t).any()), ("unwritten", tuple(t.shape), int(gb.unwritten(t).sum()))
    for t in untouched:
        assert bool(gb.unwritten(t).all()), ("written", tuple(t.shape))


# -------------------------------------------------------------------------------------------------------------------- message
def _message_inputs(c):
    el, sp = c.edges, c.spec
    d = {"c_rowptr": _in(el.c_rowptr, torch.int32), "c_perm": _in(el.c_perm, torch.int32), "n_rowptr": _in(el.n_rowptr, torch.int32),
         "n_perm": _in(el.n_perm, torch.int32), "edge_index": _in(el.edge_index, torch.int64), "p0": _in(sp["p0"]), "p1": _in(sp["p1"]),
         "w": _in(c.w), "b": _in(c.b)}
    d.update({k: _in(getattr(c, k)) for k in ("vec", "h", "s", "x", "g_s", "g_x")})
    d["wp"] = _out(int(lib.load().xeq_painn_filter_packed_floats(c.F)))
    call("xeq_painn_pack_filter", ptr(d["w"]), ptr(d["b"]), c.F, c.B, ptr(d["wp"]), stream())
    return d


def _cfg(c):
    sp = c.spec
    return (sp["rbf_code"], sp["cutoff_code"], c.B, float(sp["cutoff"]), c.F)


def _message_fwd(c, d):
    s_out, x_out = _out(c.n, c.F), _out(c.n, 3, c.F)
    call("xeq_painn_message_fwd", c.n, c.edges.n_edges, ptr(d["c_rowptr"]), ptr(d["c_perm"]), ptr(d["edge_index"]), ptr(d["vec"]), ptr(d["h"]),
         ptr(d["s"]), ptr(d["x"]), ptr(d["wp"]), ptr(d["p0"]), ptr(d["p1"]), *_cfg(c), ptr(s_out), ptr(x_out), stream())
    _finish(d.values(), [s_out, x_out])
    return {"s_out": s_out, "x_out": x_out}


def _message_bwd(c, d, g_x="given", want_g_x_in=True, prefill=None):
    """g_x: "given" | "zeros" | None (null); prefill: accumulate_vec = 1 on a copy of this buffer"""
    g_h, g_x_in = _out(c.n, 3 * c.F), (_out(c.n, 3, c.F) if want_g_x_in else None)
    g_vec = _out(c.edges.n_edges, 3) if prefill is None else _in(prefill)
    gx = {"given": d["g_x"], "zeros": _in(torch.zeros_like(c.g_x)), None: None}[g_x]
    call("xeq_painn_message_bwd", c.n, c.edges.n_edges, ptr(d["n_rowptr"]), ptr(d["n_perm"]), ptr(d["edge_index"]), ptr(d["vec"]), ptr(d["h"]),
         ptr(d["x"]), ptr(d["wp"]), ptr(d["p0"]), ptr(d["p1"]), *_cfg(c), ptr(d["g_s"]), ptr(gx), ptr(g_h), ptr(g_x_in), ptr(g_vec),
         int(prefill is not None), stream())
    _finish(list(d.values()) + [gx], [g_h, g_vec] + ([g_x_in] if want_g_x_in else []))
    return {"g_h": g_h, "g_x_in": g_x_in, "g_vec": g_vec}


def _message_both(c):
    d = _message_inputs(c)
    got = {**_message_fwd(c, d), **_message_bwd(c, d)}
    return d, {k: v.cpu() for k, v in got.items()}


def _check_message(c, tag):
    d, got = _message_both(c)
    assert torch.equal(d["wp"].cpu().reshape(pc.KPAD, 3 * c.F), pc.packed_filter(c.w.float(), c.b.float())), "packed filter"
    _compare("message_fwd", c.F, tag, got, c.ref, c.ref32, ("s_out", "x_out"))
    _compare("message_bwd", c.F, tag, got, c.ref, c.ref32, ("g_h", "g_x_in", "g_vec"))
    _check_message_exact_rows(c, got)
    return got


def _check_message_exact_rows(c, got):
    """What must hold to the bit: rows of nodes without walked edges, and everything that belongs to edges at or beyond the cutoff."""
    el = c.edges
    s32, x32, gx32 = c.s.float(), c.x.float(), c.g_x.float()
    fwd_empty = torch.tensor(np.diff(el.c_rowptr) == 0)
    rev_empty = torch.tensor(np.diff(el.n_rowptr) == 0)
    assert int(fwd_empty.sum()) >= 2 and int(rev_empty.sum()) >= 2 and bool(fwd_empty[-1]) and bool(rev_empty[-1])
    assert torch.equal(got["s_out"][fwd_empty], s32[fwd_empty]) and torch.equal(got["x_out"][fwd_empty], x32[fwd_empty])
    assert float(got["g_h"][rev_empty].abs().max()) == 0.0 and torch.equal(got["g_x_in"][rev_empty], gx32[rev_empty])
    assert int(c.beyond.sum()) >= 7 and float(got["g_vec"][c.beyond].abs().max()) == 0.0
    # a node all of whose walked edges are at or beyond the cutoff passes through as one without edges
    ei, live = torch.tensor(el.edge_index), ~c.beyond
    fwd_dead = torch.ones(c.n, dtype=torch.bool).index_put_((ei[0][live],), torch.tensor(False)) & ~fwd_empty
    rev_dead = torch.ones(c.n, dtype=torch.bool).index_put_((ei[1][live],), torch.tensor(False)) & ~rev_empty
    assert bool(fwd_dead.any()) or bool(rev_dead.any())
    assert torch.equal(got["s_out"][fwd_dead], s32[fwd_dead]) and torch.equal(got["x_out"][fwd_dead], x32[fwd_dead])
    if bool(rev_dead.any()):
        assert float(got["g_h"][rev_dead].abs().max()) == 0.0 and torch.equal(got["g_x_in"][rev_dead], gx32[rev_dead])


def test_the_bound_is_the_projects_rule():
    from tests.test_gpu_painn import _bound

    c = pc.update_case(32, 17)
    assert lib.load().xeq_painn_few_rows_limit() == pc.FEW_ROWS
    for k in pc.UPDATE_OUTPUTS:
        assert pc.bound(c.ref[k], c.ref32[k]) == _bound(c.ref[k], c.ref32[k])


@pytest.mark.parametrize("list_kind", ["directed", "transpose", "symmetric"])
@pytest.mark.parametrize("F", WIDTHS)
def test_message_width_sweep(F, list_kind):
    assert lib.load().xeq_painn_supported(lib.XEQ_F32, F, 20) == 1
    _check_message(pc.message_case(F, 20, list_kind=list_kind), f"width:{list_kind}")


@pytest.mark.parametrize("F", [32, 128])
@pytest.mark.parametrize("B", [1, 3, 4, 7, 8, 20, 31])
def test_message_basis_sweep(B, F):
    assert lib.load().xeq_painn_supported(lib.XEQ_F32, F, B) == 1
    _check_message(pc.message_case(F, B, list_kind="symmetric"), f"basis:B={B}")


@pytest.mark.parametrize("cutoff_kind", pc.CUTOFF_NAMES)
@pytest.mark.parametrize("rbf_kind", pc.RBF_NAMES)
def test_message_radial_and_envelope_sweep(rbf_kind, cutoff_kind):
    _check_message(pc.message_case(64, 8, rbf_kind, cutoff_kind), f"radial:{rbf_kind}:{cutoff_kind}")


@pytest.mark.parametrize("rbf_kind, cutoff_kind", [("bessel", "polynomial"), ("expnorm", "cosine")])
def test_message_with_a_cutoff_of_3_7(rbf_kind, cutoff_kind):
    _check_message(pc.message_case(64, 8, rbf_kind, cutoff_kind, cutoff=3.7, list_kind="symmetric"), f"cutoff3.7:{rbf_kind}:{cutoff_kind}")


@pytest.mark.parametrize("F", [96, 128])
def test_message_on_a_shuffled_list(F):
    c = pc.message_case(F, 20, list_kind="shuffled")
    assert c.edges.c_perm is not None and c.edges.n_perm is not None
    _check_message(c, "shuffled")


@pytest.mark.parametrize("F, list_kind", [(64, "symmetric"), (160, "transpose")])
def test_edges_beyond_the_cutoff_contribute_nothing(F, list_kind):
    """Besides the exact zeros of _check_message_exact_rows: other vectors beyond the cutoff in their place change no bit anywhere."""
    c = pc.message_case(F, 20, list_kind=list_kind)
    d, got = _message_both(c)
    vec = c.vec.clone()
    vec[c.beyond] = vec[c.beyond].flip(-1) * 1.5
    d["vec"] = _in(vec)
    other = {**_message_fwd(c, d), **_message_bwd(c, d)}
    for k in pc.MESSAGE_OUTPUTS:
        assert torch.equal(other[k].cpu(), got[k]), k


@pytest.mark.parametrize("F, list_kind", [(32, "symmetric"), (128, "directed"), (256, "transpose")])
def test_message_reverse_options(F, list_kind):
    c = pc.message_case(F, 20, list_kind=list_kind)
    d = _message_inputs(c)
    full = _message_bwd(c, d)
    # g_x null = a zero g_x, bit for bit
    null, zero = _message_bwd(c, d, g_x=None), _message_bwd(c, d, g_x="zeros")
    for k in ("g_h", "g_x_in", "g_vec"):
        assert torch.equal(null[k], zero[k]), k
    assert not torch.equal(null["g_h"], full["g_h"])
    # g_x_in null: the other outputs do not move
    lean = _message_bwd(c, d, want_g_x_in=False)
    assert torch.equal(lean["g_h"], full["g_h"]) and torch.equal(lean["g_vec"], full["g_vec"])
    # accumulate_vec = 1: the buffer's contents plus the accumulate_vec = 0 result
    pre = torch.randn((c.edges.n_edges, 3), generator=torch.Generator().manual_seed(F)).float()
    acc = _message_bwd(c, d, prefill=pre)
    assert torch.equal(acc["g_vec"], pre.to(DEV) + full["g_vec"])
    assert torch.equal(acc["g_h"], full["g_h"]) and torch.equal(acc["g_x_in"], full["g_x_in"])


@pytest.mark.parametrize("F", [32, 256])
def test_message_zero_node_and_zero_edge_calls(F):
    c = pc.message_case(F, 20)
    d = _message_inputs(c)
    # n_nodes = 0: nothing is touched
    outs = [_out(c.n, c.F), _out(c.n, 3, c.F), _out(c.n, 3 * c.F), _out(c.n, 3, c.F), _out(c.edges.n_edges, 3)]
    call("xeq_painn_message_fwd", 0, c.edges.n_edges, ptr(d["c_rowptr"]), ptr(d["c_perm"]), ptr(d["edge_index"]), ptr(d["vec"]), ptr(d["h"]),
         ptr(d["s"]), ptr(d["x"]), ptr(d["wp"]), ptr(d["p0"]), ptr(d["p1"]), *_cfg(c), ptr(outs[0]), ptr(outs[1]), stream())
    call("xeq_painn_message_bwd", 0, c.edges.n_edges, ptr(d["n_rowptr"]), ptr(d["n_perm"]), ptr(d["edge_index"]), ptr(d["vec"]), ptr(d["h"]),
         ptr(d["x"]), ptr(d["wp"]), ptr(d["p0"]), ptr(d["p1"]), *_cfg(c), ptr(d["g_s"]), ptr(d["g_x"]), ptr(outs[2]), ptr(outs[3]), ptr(outs[4]),
         0, stream())
    _finish(d.values(), [], outs)
    # n_edges = 0 with null edge_index / vec (/ g_vec): the inputs are copied through
    rowptr = _in(np.zeros(c.n + 1, dtype=np.int32), torch.int32)
    s_out, x_out, g_h, g_x_in = outs[:4]
    call("xeq_painn_message_fwd", c.n, 0, ptr(rowptr), None, None, None, ptr(d["h"]), ptr(d["s"]), ptr(d["x"]), ptr(d["wp"]), ptr(d["p0"]),
         ptr(d["p1"]), *_cfg(c), ptr(s_out), ptr(x_out), stream())
    call("xeq_painn_message_bwd", c.n, 0, ptr(rowptr), None, None, None, ptr(d["h"]), ptr(d["x"]), ptr(d["wp"]), ptr(d["p0"]), ptr(d["p1"]),
         *_cfg(c), ptr(d["g_s"]), ptr(d["g_x"]), ptr(g_h), ptr(g_x_in), None, 0, stream())
    _finish(list(d.values()) + [rowptr], [s_out, x_out, g_h, g_x_in], [outs[4]])
    assert torch.equal(s_out, d["s"]) and torch.equal(x_out, d["x"]) and torch.equal(g_x_in, d["g_x"]) and float(g_h.abs().max()) == 0.0


# --------------------------------------------------------------------------------------------------------------------- update
def _update_inputs(c, rows=None):
    """the case's tensors (``rows``: a slice of them) between NaN bands, and the packed U / V weights"""
    sl = slice(None) if rows is None else rows
    d = {k: _in(getattr(c, k)[sl]) for k in ("s", "x", "a", "g_s", "g_x", "g_cat")}
    d["wu"], d["wv"] = _in(c.wu), _in(c.wv)
    d["wp"] = _out(int(lib.load().xeq_painn_uv_packed_floats(c.F)))
    call("xeq_painn_pack_uv", ptr(d["wu"]), ptr(d["wv"]), c.F, ptr(d["wp"]), stream())
    return d


def _update_run(F, d, x_out=True, g_x="given"):
    """uv_fwd, out_fwd, out_bwd, uv_bwd in the order nn/painn.py::UpdateFn runs them; the reverse reads the forward's own U, V, ip, cat"""
    n = d["s"].shape[0]
    o = {"U": _out(n, 3, F), "V": _out(n, 3, F), "ip": _out(n, F), "cat": _out(n, 2 * F), "s_out": _out(n, F),
         "x_out": _out(n, 3, F) if x_out else None, "g_a": _out(n, 3 * F), "g_s_in": _out(n, F), "g_x_in": _out(n, 3, F)}
    gx = {"given": d["g_x"], "zeros": _in(torch.zeros((n, 3, F))), None: None}[g_x]
    call("xeq_painn_update_uv_fwd", n, F, ptr(d["s"]), ptr(d["x"]), ptr(d["wp"]), ptr(o["U"]), ptr(o["V"]), ptr(o["ip"]), ptr(o["cat"]), stream())
    call("xeq_painn_update_out_fwd", n, F, ptr(d["s"]), ptr(d["x"]), ptr(d["a"]), ptr(o["U"]), ptr(o["ip"]), ptr(o["s_out"]), ptr(o["x_out"]), stream())
    call("xeq_painn_update_out_bwd", n, F, ptr(d["g_s"]), ptr(gx), ptr(o["U"]), ptr(o["ip"]), ptr(o["g_a"]), stream())
    call("xeq_painn_update_uv_bwd", n, F, ptr(d["g_s"]), ptr(gx), ptr(d["a"]), ptr(o["U"]), ptr(o["V"]), ptr(o["cat"]), ptr(d["g_cat"]),
         ptr(d["wp"]), ptr(o["g_s_in"]), ptr(o["g_x_in"]), stream())
    _finish(list(d.values()) + [gx], [v for v in o.values() if v is not None])
    return o


UPDATE_CASES = [(F, n) for F in WIDTHS for n in (1, 15, 16, 17, 33)] + [(F, n) for F in (32, 96, 128, 256) for n in (2048, 2049)]


@pytest.mark.parametrize("F, n", UPDATE_CASES)
def test_update_width_and_row_sweep(F, n):
    assert lib.load().xeq_painn_supported(lib.XEQ_F32, F, 1) == 1
    c = pc.update_case(F, n)
    got = {k: v.cpu() for k, v in _update_run(F, _update_inputs(c)).items()}
    _compare("update_fwd", F, f"n={n}", got, c.ref, c.ref32, ("U", "V", "ip", "cat", "s_out", "x_out"))
    _compare("update_bwd", F, f"n={n}", got, c.ref, c.ref32, ("g_a", "g_s_in", "g_x_in"))
    assert torch.equal(got["cat"][:, :F], c.s.float()) and torch.equal(got["g_a"][:, :F], c.g_s.float())
    assert (n > pc.ZERO_ROW_INSIDE + 1) == bool(c.zero_rows)
    for r in c.zero_rows:   # x = 0: V = 0, |V| exactly 0, a finite reverse (compared above with the reference's zero subgradient)
        assert float(got["V"][r].abs().max()) == 0.0 and float(got["U"][r].abs().max()) == 0.0 and float(got["cat"][r, F:].abs().max()) == 0.0
        assert torch.isfinite(got["g_x_in"][r]).all() and torch.equal(got["x_out"][r], torch.zeros(3, F))


@pytest.mark.parametrize("F, n", [(32, 17), (160, 33), (256, 2049)])
def test_update_null_options(F, n):
    c = pc.update_case(F, n)
    d = _update_inputs(c)
    full = _update_run(F, d)
    lean = _update_run(F, d, x_out=False)
    assert torch.equal(lean["s_out"], full["s_out"])
    null, zero = _update_run(F, d, g_x=None), _update_run(F, d, g_x="zeros")
    for k in ("g_a", "g_s_in", "g_x_in"):
        assert torch.equal(null[k], zero[k]), k
    assert not torch.equal(null["g_x_in"], full["g_x_in"])


@pytest.mark.parametrize("F", [32, 96, 256])
def test_update_rows_have_the_same_bits_in_every_launch_shape(F):
    """the first 2 048 rows of a 2 049-row call (the large launch shape) are bit-equal to a 2 048-row call on the
    same rows (the few-row shape), and a row evaluated alone is bit-equal to itself inside the batch."""
    assert lib.load().xeq_painn_few_rows_limit() == 2048
    c = pc.update_case(F, 2049)
    large = _update_run(F, _update_inputs(c))
    few = _update_run(F, _update_inputs(c, slice(0, 2048)))
    for k in pc.UPDATE_OUTPUTS:
        assert torch.equal(large[k][:2048], few[k]), k
    for r in (0, 1000, 2047, 2048):
        one = _update_run(F, _update_inputs(c, slice(r, r + 1)))
        for k in pc.UPDATE_OUTPUTS:
            assert torch.equal(one[k][0], large[k][r]), (k, r)


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_add(n):
    gen = torch.Generator().manual_seed(n)
    a, b = _in(torch.randn(n, generator=gen)), _in(torch.randn(n, generator=gen))
    out = _out(n)
    call("xeq_painn_add", ptr(a), ptr(b), n, ptr(out), stream())
    _finish([a, b], [out])
    assert torch.equal(out, a + b)
    none = _out(n)
    call("xeq_painn_add", ptr(a), ptr(b), 0, ptr(none), stream())
    _finish([a, b], [], [none])


# ------------------------------------------------------------------------------------------------------------------- refusals
BAD_WIDTHS = (0, 16, 48, 288)
BAD_BASES = (0, 32)


def test_supported_says_no_outside_the_instantiated_shapes():
    L = lib.load()
    for F in BAD_WIDTHS:
        assert L.xeq_painn_supported(lib.XEQ_F32, F, 20) == 0, F
    for B in BAD_BASES:
        assert L.xeq_painn_supported(lib.XEQ_F32, 128, B) == 0, B
    for F in WIDTHS:
        assert L.xeq_painn_supported(lib.XEQ_F64, F, 20) == 0
        for B in (1, 20, 31):
            assert L.xeq_painn_supported(lib.XEQ_F32, F, B) == 1


@pytest.mark.parametrize("F, B", [(F, 20) for F in BAD_WIDTHS] + [(128, B) for B in BAD_BASES])
def test_every_entry_point_refuses_a_shape_that_is_not_supported(F, B):
    """The status comes back through lib.call as an exception; the outputs keep the never-written pattern and their bands."""
    c = pc.message_case(128, 20)
    u = pc.update_case(128, 17)
    d = _message_inputs(c)   # buffers of the largest admitted row all over: a kernel that ran anyway would stay inside them
    du = _update_inputs(u)
    big = lambda: _out(c.n, 3, 288)
    outs = [big() for _ in range(9)]
    cfg = (c.spec["rbf_code"], c.spec["cutoff_code"], B, 5.0, F)
    msg_fwd = lambda: call("xeq_painn_message_fwd", c.n, c.edges.n_edges, ptr(d["c_rowptr"]), ptr(d["c_perm"]), ptr(d["edge_index"]), ptr(d["vec"]),
                           ptr(d["h"]), ptr(d["s"]), ptr(d["x"]), ptr(d["wp"]), ptr(d["p0"]), ptr(d["p1"]), *cfg, ptr(outs[0]), ptr(outs[1]), stream())
    msg_bwd = lambda: call("xeq_painn_message_bwd", c.n, c.edges.n_edges, ptr(d["n_rowptr"]), ptr(d["n_perm"]), ptr(d["edge_index"]), ptr(d["vec"]),
                           ptr(d["h"]), ptr(d["x"]), ptr(d["wp"]), ptr(d["p0"]), ptr(d["p1"]), *cfg, ptr(d["g_s"]), ptr(d["g_x"]), ptr(outs[2]),
                           ptr(outs[3]), ptr(outs[4]), 0, stream())
    calls = {"pack_filter": lambda: call("xeq_painn_pack_filter", ptr(d["w"]), ptr(d["b"]), F, B, ptr(outs[5]), stream()),
             "message_fwd": msg_fwd, "message_bwd": msg_bwd}
    if F != 128:
        n = u.n
        calls.update({
            "pack_uv": lambda: call("xeq_painn_pack_uv", ptr(du["wu"]), ptr(du["wv"]), F, ptr(outs[6]), stream()),
            "update_uv_fwd": lambda: call("xeq_painn_update_uv_fwd", n, F, ptr(du["s"]), ptr(du["x"]), ptr(du["wp"]), ptr(outs[0]), ptr(outs[1]),
                                          ptr(outs[2]), ptr(outs[3]), stream()),
            "update_out_fwd": lambda: call("xeq_painn_update_out_fwd", n, F, ptr(du["s"]), ptr(du["x"]), ptr(du["a"]), ptr(du["x"]), ptr(du["s"]),
                                           ptr(outs[4]), ptr(outs[5]), stream()),
            "update_out_bwd": lambda: call("xeq_painn_update_out_bwd", n, F, ptr(du["g_s"]), ptr(du["g_x"]), ptr(du["x"]), ptr(du["s"]), ptr(outs[7]),
                                           stream()),
            "update_uv_bwd": lambda: call("xeq_painn_update_uv_bwd", n, F, ptr(du["g_s"]), ptr(du["g_x"]), ptr(du["a"]), ptr(du["x"]), ptr(du["x"]),
                                          ptr(du["g_cat"]), ptr(du["g_cat"]), ptr(du["wp"]), ptr(outs[8]), ptr(outs[6]), stream())})
    for name, fn in calls.items():
        with pytest.raises(RuntimeError, match="not supported"):
            fn()
    _finish(list(d.values()) + list(du.values()), [], outs)


# ------------------------------------------------------------------------------------------------- through the Python wrappers
def test_edge_graph_mirror_map_is_the_numpy_reverse_edge_map():
    from xequinet_amd import ops

    el = pc.edge_list("symmetric")
    graph = ops.EdgeGraph(torch.tensor(el.edge_index, device=DEV), el.n_nodes, symmetric=True)
    assert torch.equal(graph.mirror_map.cpu(), torch.tensor(el.n_perm)) and torch.equal(graph.n_perm.cpu(), torch.tensor(el.n_perm))
    assert torch.equal(graph.c_rowptr.cpu(), torch.tensor(el.c_rowptr)) and graph.n_rowptr is graph.c_rowptr and graph.c_perm is None


@pytest.mark.parametrize("list_kind", ["symmetric", "directed", "shuffled"])
def test_message_through_the_python_wrappers(list_kind):
    """MessageFn.apply at F = 128 over an ops.EdgeGraph built by the project (symmetric / center-sorted directed / unsorted), with
    h = scalar_mlp(s), against the same reference: ties the numpy-built views above to the ones the model uses."""
    from xequinet_amd import ops
    from xequinet_amd.nn import painn
    from xequinet_amd.nn.rbf import resolve_cutoff, resolve_rbf

    F, B = 128, 20
    c = pc.message_case(F, B, list_kind=list_kind)
    el = c.edges
    mod = painn.PainnMessage(F, B)
    shapes = {k: tuple(v.shape) for k, v in mod.state_dict().items()}
    p = po.seeded_weights(shapes, 5)
    p["rbf_lin.weight"], p["rbf_lin.bias"] = c.w, c.b
    p = {k: v.float().double() for k, v in p.items()}
    mod.load_state_dict({k: v.float() for k, v in p.items()})
    mod = mod.to(DEV).eval().requires_grad_(False)
    rbf, env = resolve_rbf("bessel", B, 5.0).to(DEV), resolve_cutoff("cosine", 5.0)
    graph = ops.EdgeGraph(torch.tensor(el.edge_index, device=DEV), el.n_nodes, symmetric=el.symmetric)
    views = [(graph.c_rowptr, el.c_rowptr), (graph.c_perm, el.c_perm), (graph.n_rowptr, el.n_rowptr), (graph.n_perm, el.n_perm)]
    for got, want in views:   # the project's views of this list are the numpy ones
        assert (got is None) == (want is None) and (got is None or torch.equal(got.cpu(), torch.tensor(want)))

    def reference(dtype):
        t = lambda v: v.detach().to(dtype).clone()
        s, x, vec = t(c.s).requires_grad_(), t(c.x).requires_grad_(), t(c.vec).requires_grad_()
        h = po._mlp(s, po.cast(p, dtype), "scalar_mlp")
        out = pc.message_ref(s, x, h, vec, torch.tensor(el.edge_index), t(c.w), t(c.b), "bessel", "cosine", c.spec["rbf_params"], 5.0)
        g = torch.autograd.grad(out, [s, x, vec], [t(c.g_s), t(c.g_x)])
        return dict(zip(("s_out", "x_out", "g_s_in", "g_x_in", "g_vec"), [o.detach() for o in out] + list(g)))

    ref, ref32 = reference(torch.float64), reference(torch.float32)
    with gb.guard_allocations():
        s, x, vec = (v.float().to(DEV).requires_grad_() for v in (c.s, c.x, c.vec))
        with torch.enable_grad():
            out = painn.MessageFn.apply(s, x, vec, mod, graph, rbf, env, None, False)
            g = torch.autograd.grad(out, [s, x, vec], [c.g_s.float().to(DEV), c.g_x.float().to(DEV)])
        torch.cuda.synchronize()
    got = dict(zip(("s_out", "x_out", "g_s_in", "g_x_in", "g_vec"), [o.detach().cpu() for o in out] + [v.cpu() for v in g]))
    _compare("message_wrapper", F, list_kind, got, ref, ref32, tuple(got))
