"""The update kernels at every admitted layout and row form, against the f64 reference of tests/update_cases.py:
  xeq_update_uv_fwd / _bwd (csrc/xeq_update.hip) through the C ABI at all 33 layouts (+ four layouts at node_dim 4, 36, 100, 128), in the
  32-row and the few-row form, the reverse fused, split 32-row and split few-row; through fused.UpdateBlock at every layout;
  the chain kernels of csrc/xeq_node.hip on both sides of their form switches, f32 and f64; xeq_norm_param_grad (csrc/xeq_train.hip).

Entry level: every input sits between guard bands, every output is handed over holding the never-written pattern between bands of its
own, each call once with finite-garbage bands and once with NaN bands (tests/guard_bands.py): the bands are compared bit for bit, the n
rows hold no never-written word, spare rows hold nothing else, and the two runs give the same bits.

Bound per output tensor and row group (ordinary rows, the all-zero row, the row scaled by 1e3): max(1e-4 max(1, max|ref|), 1.5 err32).
tests/test_update_cases_host.py shows that every defect of its list leaves that bound.  Every figure is printed before it is asserted
(``update-kernels ...`` lines: profiles/update_layouts.txt is their summary)."""
import copy
import math

import pytest
import torch

from tests import guard_bands as gb, update_cases as uc
from tests.test_gpu_small_rows import _forms
from xequinet_amd import lib
from xequinet_amd.lib import call, mul3, ptr, stream
from xequinet_amd.nn import fused

pytestmark = pytest.mark.gpu

DEV = "cuda"
SPARE_ROWS = 3
FILLS = ("finite", "nan")
FORM_LIMIT = {"rows32": 0, "few": 1 << 40}
CONFIG_IDS = [uc.config_id(*c) for c in uc.CONFIGS]


def _in(t, fill):
    return gb.guarded_copy(torch.as_tensor(t).to(torch.float32).to(DEV).contiguous(), fill)


def _out(shape, fill, dtype=torch.float32):
    return gb.guarded(shape, dtype, DEV, fill=fill, body="unwritten")


def _finish(inputs, outputs, n, flat=()):
    torch.cuda.synchronize()
    gb.check(*[t for t in inputs if t is not None], *outputs, *flat)
    for t in outputs:
        assert not bool(gb.unwritten(t[:n]).any()), ("unwritten", tuple(t.shape), int(gb.unwritten(t[:n]).sum()))
        assert bool(gb.unwritten(t[n:]).all()), ("a row past n was written", tuple(t.shape))
    for t in flat:
        assert not bool(gb.unwritten(t).any()), ("unwritten", tuple(t.shape), int(gb.unwritten(t).sum()))


_PACKS = {}


def _packs(mul, F, fill):
    """The [W_U | W_V] / sqrt(mul) blocks in fragment order as fused._packed_uv_frag makes them, between bands:
    -> (forward packs with the bias group, forward packs without, reverse packs), one entry per l (None: absent)."""
    key = (mul, F, fill)
    if key not in _PACKS:
        m = uc.master(mul, F)
        floats = lambda n_out, k_in: int(lib.load().xeq_mlp_packed_floats(n_out, k_in))
        with_b, without, rev, off = [None] * 3, [None] * 3, [None] * 3, 0
        made, ins = [], []
        bias = _in(torch.cat([m.bu, m.bv]), fill) if mul[0] > 0 else None
        for l, k in enumerate(mul):
            if k == 0:
                continue
            wu = m.wu[off:off + k * k].view(k, k).float().to(DEV)
            wv = m.wv[off:off + k * k].view(k, k).float().to(DEV)
            off += k * k
            W = _in((torch.cat([wu, wv], dim=1) / math.sqrt(k)).contiguous(), fill)        # [k_in = mul][n_out = 2 mul], as _packed_uv
            ins.append(W)
            without[l] = _out(floats(2 * k, k), fill)
            call("xeq_mlp_pack", ptr(W), None, 2 * k, k, 1, ptr(without[l]), stream())
            with_b[l] = without[l]
            if l == 0:
                with_b[l] = _out(floats(2 * k, k), fill)
                call("xeq_mlp_pack", ptr(W), ptr(bias), 2 * k, k, 1, ptr(with_b[l]), stream())
                made.append(with_b[l])
            rev[l] = _out(floats(k, 2 * k), fill)
            call("xeq_mlp_pack", ptr(W), None, k, 2 * k, 0, ptr(rev[l]), stream())
            made += [without[l], rev[l]]
        _finish(ins + [bias], [], 0, flat=made)
        _PACKS[key] = (with_b, without, rev)
    return _PACKS[key]


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---------------------------------------------------------------------------------------------------------------- entry level: forward
_FWD = {}


def _forward(mul, F, form, do_norm, has_bias, n):
    """xeq_update_uv_fwd on the first n rows, with both band fills -> cat, p, uv (flat BT), stats on the CPU."""
    key = (mul, F, form, do_norm, has_bias, n)
    if key in _FWD:
        return _FWD[key]
    D, C = uc.dims(mul)
    n_master = uc.ROWS_MASTER if n <= uc.ROWS_MASTER else max(uc.THRESHOLD_ROWS)
    m = uc.master(mul, F, n_master)
    res = {}
    for fill in FILLS:
        pk = _packs(mul, F, fill)[0 if has_bias else 1]
        s, x = _in(m.s[:n], fill), _in(m.x[:n], fill)
        prm = [_in(getattr(m, k), fill) if (do_norm and getattr(m, k).numel()) else None for k in ("lnw", "lnb", "eqw", "eqb")]
        # (l = 0 absent: affine_bias is empty and its pointer NULL, as the module's is)
        cat, p, stats = _out((n + SPARE_ROWS, F + C), fill), _out((n + SPARE_ROWS, C), fill), _out((n + SPARE_ROWS, 4), fill)
        uv = _out(2 * n * D, fill)
        with _forms(FORM_LIMIT[form]):
            call("xeq_update_uv_fwd", ptr(s), ptr(x), ptr(prm[0]), ptr(prm[1]), ptr(prm[2]), ptr(prm[3]), n, F, mul3(mul), do_norm,
                 ptr(pk[0]), ptr(pk[1]), ptr(pk[2]), int(has_bias), uc.EPS, ptr(cat), F + C, ptr(p), ptr(uv), ptr(stats), stream())
        _finish([s, x, *prm, *[q for q in pk if q is not None]], [cat, p, stats], n, flat=[uv])
        res[fill] = {"cat": cat[:n].cpu(), "p": p[:n].cpu(), "uv": uv.cpu(), "stats": stats[:n].cpu()}
    for k in uc.FWD_OUTPUTS:
        assert torch.isfinite(res["nan"][k]).all(), (k, "not finite with NaN bands")
        assert _same_bits(res["finite"][k], res["nan"][k]), (k, "depends on what lies behind a buffer")
    _FWD[key] = res["nan"]
    return _FWD[key]


class _Record:
    """Worst case per (output, row group) of one test: printed as the record, asserted at the end."""

    def __init__(self, tag):
        self.tag, self.worst, self.failed = tag, {}, []

    def add(self, res, what):
        for k, grp, err, err32, bnd in res:
            w = self.worst.get((k, grp))
            if w is None or err / bnd > w[0] / w[2]:
                self.worst[(k, grp)] = (err, err32, bnd, what)
            if not err <= bnd:
                self.failed.append((k, grp, what, err, err32, bnd))

    def close(self):
        for (k, grp), (err, err32, bnd, what) in sorted(self.worst.items()):
            print(f"update-kernels {self.tag} {k} {grp}: err {err:.3e} err32 {err32:.3e} bound {bnd:.3e} ({what})")
        assert not self.failed, (self.tag, self.failed)


def _rows(got, names, n, mul):
    return {k: uc.rows_of(k, got[k], n, mul) for k in names}


def _fwd_variants(mul):
    return [(dn, hb) for dn in (0, 1) for hb in ((0, 1) if mul[0] > 0 else (0,))]


@pytest.mark.parametrize("form", ["rows32", "few"])
@pytest.mark.parametrize("mul,F", uc.CONFIGS, ids=CONFIG_IDS)
def test_forward_against_the_f64_reference(mul, F, form):
    """cat = [shat | v], p, the U|V pair buffer and stats, with and without the norms, with and without the l = 0 bias group, at row
    counts around the 16- and 32-row edges, one row, more than one tile."""
    rec = _Record(f"{uc.config_id(mul, F)} fwd {form}")
    for do_norm, has_bias in _fwd_variants(mul):
        for n in uc.ROWS:
            c = uc.case(mul, F, n, do_norm, has_bias)
            got = _rows(_forward(mul, F, form, do_norm, has_bias, n), uc.FWD_OUTPUTS, n, mul)
            rec.add(uc.judge(c.ref, c.ref32, got, uc.FWD_OUTPUTS, n), f"norm {do_norm} bias {has_bias} n {n}")
    rec.close()


@pytest.mark.parametrize("mul,F", uc.CONFIGS, ids=CONFIG_IDS)
def test_forward_forms_and_batches_change_no_bit(mul, F):
    """The few-row form gives the bits of the 32-row form; a row alone gives the bits it has inside the 65-row batch."""
    for do_norm, has_bias in _fwd_variants(mul):
        for n in uc.ROWS:
            a, b = _forward(mul, F, "rows32", do_norm, has_bias, n), _forward(mul, F, "few", do_norm, has_bias, n)
            for k in uc.FWD_OUTPUTS:
                assert torch.equal(a[k], b[k]), (k, do_norm, has_bias, n, float((a[k] - b[k]).abs().max()))
        for form in FORM_LIMIT:
            one = _rows(_forward(mul, F, form, do_norm, has_bias, 1), uc.FWD_OUTPUTS, 1, mul)
            many = _rows(_forward(mul, F, form, do_norm, has_bias, 65), uc.FWD_OUTPUTS, 65, mul)
            for k in uc.FWD_OUTPUTS:
                assert torch.equal(one[k][0], many[k][0]), (k, form, do_norm, has_bias)


# ---------------------------------------------------------------------------------------------------------------- entry level: reverse
_BWD = {}
BWD_FORMS = {"fused": None, "split32": 0, "splitfew": 1 << 40}


def _reverse(mul, F, form, do_norm, gx, n, explicit_zero=False):
    """xeq_update_uv_bwd on the first n rows, reading the pair buffer and the statistics the forward kernel wrote (32-row form, bias
    group present where l = 0 is) -> fused: g_s, g_x; split: g_xhat (flat BT) and g_s, g_x of xeq_norm_bwd behind it."""
    key = (mul, F, form, do_norm, gx, n, explicit_zero)
    if key in _BWD:
        return _BWD[key]
    D, C = uc.dims(mul)
    has_bias = int(mul[0] > 0)
    n_master = uc.ROWS_MASTER if n <= uc.ROWS_MASTER else max(uc.THRESHOLD_ROWS)
    m = uc.master(mul, F, n_master)
    fwd = _forward(mul, F, "rows32", do_norm, has_bias, n)
    res = {}
    for fill in FILLS:
        pk = _packs(mul, F, fill)[2]
        uv, stats = _in(fwd["uv"], fill), _in(fwd["stats"], fill)
        s, x, g_p, g_cat, g_s_out, a = (_in(getattr(m, k)[:n], fill) for k in ("s", "x", "g_p", "g_cat", "g_s_out", "a"))
        g_x_out = _in(torch.zeros(n, D) if explicit_zero else m.g_x_out[:n], fill) if (gx or explicit_zero) else None
        lnw, eqw = (_in(m.lnw, fill), _in(m.eqw, fill)) if do_norm else (None, None)
        ins = [uv, stats, s, x, g_p, g_cat, g_s_out, a, g_x_out, lnw, eqw, *[q for q in pk if q is not None]]
        out = {}
        if form == "fused":
            g_s, g_x = _out((n + SPARE_ROWS, F), fill), _out((n + SPARE_ROWS, D), fill)
            call("xeq_update_uv_bwd", ptr(uv), ptr(g_p), ptr(g_cat), F + C, ptr(g_x_out), ptr(g_s_out), ptr(a), C + 2 * F, ptr(s), ptr(x),
                 ptr(stats), ptr(lnw), ptr(eqw), n, F, mul3(mul), do_norm, ptr(pk[0]), ptr(pk[1]), ptr(pk[2]), uc.EPS, ptr(g_s), ptr(g_x),
                 None, stream())
            _finish(ins, [g_s, g_x], n)
        else:
            g_xhat = _out(n * D, fill)
            with _forms(BWD_FORMS[form]):
                call("xeq_update_uv_bwd", ptr(uv), ptr(g_p), ptr(g_cat), F + C, ptr(g_x_out), ptr(g_s_out), ptr(a), C + 2 * F, None, None,
                     None, None, None, n, F, mul3(mul), do_norm, ptr(pk[0]), ptr(pk[1]), ptr(pk[2]), uc.EPS, None, None, ptr(g_xhat),
                     stream())
            _finish(ins, [], n, flat=[g_xhat])
            g_s, g_x = _out((n + SPARE_ROWS, F), fill), _out((n + SPARE_ROWS, D), fill)
            call("xeq_norm_bwd", lib.XEQ_F32, ptr(s), ptr(x), ptr(lnw), ptr(eqw), ptr(stats), n, F, mul3(mul), do_norm, ptr(g_cat), F + C,
                 ptr(g_xhat), ptr(g_s_out), ptr(g_x_out), ptr(g_s), ptr(g_x), stream())
            _finish(ins + [g_xhat], [g_s, g_x], n)
            out["g_xhat"] = g_xhat.cpu()
        out.update(g_s=g_s[:n].cpu(), g_x=g_x[:n].cpu())
        res[fill] = out
    for k in res["nan"]:
        assert torch.isfinite(res["nan"][k]).all(), (k, "not finite with NaN bands")
        assert _same_bits(res["finite"][k], res["nan"][k]), (k, "depends on what lies behind a buffer")
    _BWD[key] = res["nan"]
    return _BWD[key]


@pytest.mark.parametrize("form", list(BWD_FORMS))
@pytest.mark.parametrize("mul,F", uc.CONFIGS, ids=CONFIG_IDS)
def test_reverse_against_the_f64_reference(mul, F, form):
    """g_s, g_x of the fused form; g_xhat of the split forms and g_s, g_x of xeq_norm_bwd behind them; with g_x_out given and NULL,
    with and without the norms.  g_x_out = NULL gives the bits of an explicit zero."""
    rec = _Record(f"{uc.config_id(mul, F)} bwd {form}")
    names = ("g_s", "g_x") if form == "fused" else uc.BWD_OUTPUTS
    for do_norm in (0, 1):
        for gx in (1, 0):
            for n in uc.ROWS:
                c = uc.case(mul, F, n, do_norm, int(mul[0] > 0), gx)
                got = _reverse(mul, F, form, do_norm, gx, n)
                rec.add(uc.judge(c.ref, c.ref32, _rows(got, names, n, mul), names, n), f"norm {do_norm} g_x_out {gx} n {n}")
                if not gx and n in (1, 17, 33, 65):
                    zero = _reverse(mul, F, form, do_norm, gx, n, explicit_zero=True)
                    for k in names:
                        assert torch.equal(got[k], zero[k]), (k, do_norm, n, "NULL g_x_out is not an explicit zero")
    rec.close()


@pytest.mark.parametrize("mul,F", uc.CONFIGS, ids=CONFIG_IDS)
def test_reverse_split_forms_change_no_bit(mul, F):
    for do_norm in (0, 1):
        for gx in (1, 0):
            for n in uc.ROWS:
                a, b = _reverse(mul, F, "split32", do_norm, gx, n), _reverse(mul, F, "splitfew", do_norm, gx, n)
                for k in uc.BWD_OUTPUTS:
                    assert torch.equal(a[k], b[k]), (k, do_norm, gx, n, float((a[k] - b[k]).abs().max()))


def test_default_layout_runs_its_own_instantiation_and_the_generic_one_to_the_same_bound():
    """(128, 64, 32) / 128 is the one layout with template instantiations of its own: do_norm = 1 takes them, do_norm = 0 takes the
    layout-generic ones.  Both against the same reference under the same rule, every forward and reverse form, named side by side."""
    mul, F = (128, 64, 32), 128
    rec = _Record("128-64-32/128 instantiations")
    for do_norm in (1, 0):
        for form in FORM_LIMIT:
            for n in (17, 65):
                c = uc.case(mul, F, n, do_norm, 1)
                got = _rows(_forward(mul, F, form, do_norm, 1, n), uc.FWD_OUTPUTS, n, mul)
                rec.add(uc.judge(c.ref, c.ref32, got, uc.FWD_OUTPUTS, n), f"fwd {form} norm {do_norm} n {n}")
        for form in BWD_FORMS:
            names = ("g_s", "g_x") if form == "fused" else uc.BWD_OUTPUTS
            c = uc.case(mul, F, 65, do_norm, 1)
            rec.add(uc.judge(c.ref, c.ref32, _rows(_reverse(mul, F, form, do_norm, 1, 65), names, 65, mul), names, 65), f"bwd {form} norm {do_norm}")
    rec.close()


@pytest.mark.parametrize("n", uc.THRESHOLD_ROWS)
@pytest.mark.parametrize("mul", uc.THRESHOLD_LAYOUTS, ids=[uc.config_id(m, uc.default_node_dim(m)) for m in uc.THRESHOLD_LAYOUTS])
def test_tile_split_thresholds(mul, n):
    """32-row forms where TileSplit changes how it deals row tiles to workgroups: all tiles split (4096), none (4097, 8192), a split
    short last round (8200)."""
    F = uc.default_node_dim(mul)
    rec = _Record(f"{uc.config_id(mul, F)} thresholds n {n}")
    c = uc.case(mul, F, n, 1, 1)
    rec.add(uc.judge(c.ref, c.ref32, _rows(_forward(mul, F, "rows32", 1, 1, n), uc.FWD_OUTPUTS, n, mul), uc.FWD_OUTPUTS, n), "fwd")
    for form in ("fused", "split32"):
        names = ("g_s", "g_x") if form == "fused" else uc.BWD_OUTPUTS
        rec.add(uc.judge(c.ref, c.ref32, _rows(_reverse(mul, F, form, 1, 1, n), names, n, mul), names, n), f"bwd {form}")
    for cache in (_FWD, _BWD):      # (tens of MB per entry at these row counts)
        for key in [k for k in cache if k[5] > uc.ROWS_MASTER]:
            del cache[key]
    rec.close()


# ---------------------------------------------------------------------------------------------------------------- block level
def _block(mul, F, layer_norm):
    from xequinet_amd.nn.xpainn import XPainnUpdate

    m = uc.master(mul, F)
    torch.manual_seed(sum(mul) + F)
    blk = XPainnUpdate(node_dim=F, node_irreps=m.irreps, layer_norm=layer_norm).requires_grad_(False)
    with torch.no_grad():
        blk.update_U.weight.copy_(m.wu), blk.update_V.weight.copy_(m.wv), blk.update_U.bias.copy_(m.bu), blk.update_V.bias.copy_(m.bv)
        if layer_norm:
            blk.norm.weight.copy_(m.lnw), blk.norm.bias.copy_(m.lnb)
            blk.o3norm.affine_weight.copy_(m.eqw), blk.o3norm.affine_bias.copy_(m.eqb)
        for seq in (blk.update_mlp[0], blk.update_mlp[2]):
            seq.bias.add_(0.5 * torch.randn_like(seq.bias))
    return m, blk


def _oracle_block(m, blk, layer_norm, dtype, n):
    from oracle.xpainn_oracle import XPaiNNOracle

    sd = {"mods.update_0." + k: v.detach().to(dtype) for k, v in blk.state_dict().items()}
    orc = XPaiNNOracle(sd, node_dim=m.F, node_irreps=m.irreps, layer_norm=layer_norm)
    s, x = m.s[:n].to(dtype).requires_grad_(), m.x[:n].to(dtype).requires_grad_()
    data = orc.update(0, {"node_invariant": s, "node_equivariant": x})
    s_out, x_out = data["node_invariant"], data["node_equivariant"]
    g = torch.autograd.grad((s_out * m.g_s_out[:n].to(dtype)).sum() + (x_out * m.g_x_out[:n].to(dtype)).sum(), [s, x])
    return {"s_out": s_out.detach(), "x_out": x_out.detach(), "dL/ds": g[0], "dL/dx": g[1]}


BLOCK_OUTPUTS = ("s_out", "x_out", "dL/ds", "dL/dx")


@pytest.mark.parametrize("fuse_max", ["as_shipped", "zero", "every_size"])
@pytest.mark.parametrize("mul", uc.LAYOUTS, ids=[uc.config_id(m, uc.default_node_dim(m)) for m in uc.LAYOUTS])
def test_update_block_against_the_oracle_at_every_layout(monkeypatch, mul, fuse_max):
    """fused.UpdateBlock on an XPainnUpdate of the layout against XPaiNNOracle.update and its autograd at 33 rows, with and without
    layer norms; the reverse with UV_BWD_FUSE_NORM_MAX_NODES as shipped, at 0 (split form) and above every size (fused form).  The matrix-core
    front and its reverse must have run: at EVERY layout."""
    F, n = uc.default_node_dim(mul), 33
    if fuse_max != "as_shipped":
        monkeypatch.setattr(fused, "UV_BWD_FUSE_NORM_MAX_NODES", 0 if fuse_max == "zero" else 1 << 40)
    rec = _Record(f"{uc.config_id(mul, F)} block {fuse_max}")
    for layer_norm in (True, False):
        m, blk = _block(mul, F, layer_norm)
        ref, ref32 = _oracle_block(m, blk, layer_norm, torch.float64, n), _oracle_block(m, blk, layer_norm, torch.float32, n)
        dev = copy.deepcopy(blk).to(DEV).eval()
        s, x = m.s[:n].float().to(DEV).requires_grad_(), m.x[:n].float().to(DEV).requires_grad_()
        first = lib.launch_count()
        with torch.enable_grad():
            so, xo = fused.UpdateBlock.apply(s, x, dev)
            g = torch.autograd.grad([so, xo], [s, x], [m.g_s_out[:n].float().to(DEV), m.g_x_out[:n].float().to(DEV)])
        names = lib.launch_names(first)
        assert "xeq_update_uv_fwd" in names and "xeq_update_uv_bwd" in names, (mul, layer_norm, names)
        split = fuse_max == "zero" or (fuse_max == "as_shipped" and n > _SHIPPED_FUSE_MAX)
        assert ("xeq_norm_bwd" in names) == split, (fuse_max, names)      # the split form leaves the norms' reverse to xeq_norm_bwd
        got = dict(zip(BLOCK_OUTPUTS, (so.detach().cpu(), xo.detach().cpu(), g[0].cpu(), g[1].cpu())))
        rec.add(uc.judge(ref, ref32, got, BLOCK_OUTPUTS, n), f"layer_norm {layer_norm}")
    rec.close()


_SHIPPED_FUSE_MAX = fused.UV_BWD_FUSE_NORM_MAX_NODES


# ---------------------------------------------------------------------------------------------------------------- chain kernels
# (irreps, node_dim, do_norm): both sides of every form switch of csrc/xeq_node.hip
CHAIN = [("128x0e+64x1o+32x2e", 128, 1), ("128x0e+64x1o+32x2e", 132, 1),          # row-in-registers norms: node_dim 128 | 132
         ("8x0e+3x1o+99x2e", 64, 1), ("4x0e+4x1o+100x2e", 64, 1),                  # ... D 512 | 516
         ("128x0e+64x1o+64x2e", 128, 1), ("128x0e+64x1o+68x2e", 128, 1),           # column kernels: C 256 | 260
         ("128x0e+64x1o+32x2e", 128, 0),                                           # identity norms: the slow norm kernels
         ("8x0e+4x1o+2x2e", 8, 1), ("16x1o", 16, 1), ("64x1o+32x2e", 36, 1)]       # multiplicities off 32, l = 0 absent
CHAIN_SWITCH = ("8x0e+4x1o+2x2e", 8, 1)      # n = 8191 | 8192: node_npb and the nodes per wave
_GUARD_ROWS = 65


def _chain_run(c, tdt, guard):
    """The six chain kernels on the case -> name -> CPU tensor (entry-point layouts)."""
    n, F, mul = c.n, c.F, c.mul
    D, C = uc.dims(mul)
    A = C + 2 * F
    out = {}
    for fill in (FILLS if guard else ("nan",)):
        if guard:
            inp = lambda t: gb.guarded_copy(t.to(tdt).to(DEV).contiguous(), fill)
            new = lambda *shape: gb.guarded(shape, tdt, DEV, fill=fill, body="unwritten")
        else:
            inp = lambda t: t.to(tdt).to(DEV).contiguous()
            new = lambda *shape: torch.full(shape, float("nan"), dtype=tdt, device=DEV)
        dc = lib.XEQ_F32 if tdt == torch.float32 else lib.XEQ_F64
        s, x, g_cat, g_p, g_s_out, g_x_out, a, ip = (inp(getattr(c, k)) for k in ("s", "x", "g_cat", "g_p", "g_s_out", "g_x_out", "a", "ip"))
        prm = [inp(getattr(c, k)) if (c.do_norm and getattr(c, k).numel()) else None for k in ("lnw", "lnb", "eqw", "eqb")]
        uv, g_xh = inp(uc.to_bt(c.U_in, mul, pair=c.V_in)), inp(uc.to_bt(c.g_xh, mul))
        shat, xhat, stats = new(n, F), new(n * D), new(n, 4)
        call("xeq_norm_fwd", dc, ptr(s), ptr(x), ptr(prm[0]), ptr(prm[1]), ptr(prm[2]), ptr(prm[3]), n, F, mul3(mul), c.do_norm, ptr(shat), F,
             ptr(xhat), ptr(stats), stream())
        nb_g_s, nb_g_x = new(n, F), new(n, D)
        call("xeq_norm_bwd", dc, ptr(s), ptr(x), ptr(prm[0]), ptr(prm[2]), ptr(stats), n, F, mul3(mul), c.do_norm, ptr(g_cat), F + C, ptr(g_xh),
             ptr(g_s_out), ptr(g_x_out), ptr(nb_g_s), ptr(nb_g_x), stream())
        cat, p = new(n, F + C), new(n, C)
        call("xeq_uv_reduce_fwd", dc, ptr(uv), n, mul3(mul), uc.EPS, ptr(cat), F + C, F, ptr(p), stream())
        g_uv = new(2 * n * D)
        call("xeq_uv_reduce_bwd", dc, ptr(uv), ptr(g_p), ptr(g_cat), F + C, F, n, mul3(mul), uc.EPS, ptr(g_x_out), ptr(a), ptr(g_uv), stream())
        s_out, x_out = new(n, F), new(n, D)
        call("xeq_update_out_fwd", dc, ptr(s), ptr(x), ptr(uv), ptr(a), ptr(ip), n, F, mul3(mul), ptr(s_out), ptr(x_out), stream())
        g_a, g_ip = new(n, A), new(n, F)
        call("xeq_update_out_bwd", dc, ptr(g_s_out), ptr(g_x_out), ptr(uv), ptr(a), ptr(ip), n, F, mul3(mul), ptr(g_a), ptr(g_ip), None, stream())
        torch.cuda.synchronize()
        outs = dict(shat=shat, xhat=xhat, **({"stats": stats} if c.do_norm else {}), nb_g_s=nb_g_s, nb_g_x=nb_g_x, p=p, g_uv=g_uv, s_out=s_out, x_out=x_out, g_a=g_a, g_ip=g_ip)
        if guard:
            gb.check(s, x, g_cat, g_p, g_s_out, g_x_out, a, ip, uv, g_xh, *[q for q in prm if q is not None], cat, *outs.values())
            for k, t in outs.items():
                assert not bool(gb.unwritten(t).any()), (k, "unwritten", int(gb.unwritten(t).sum()))
            assert not bool(gb.unwritten(cat[:, F:]).any()) and bool(gb.unwritten(cat[:, :F]).all())     # xeq_uv_reduce_fwd writes v only
        res = {k: t.cpu() for k, t in outs.items()}
        res["v"] = cat[:, F:].cpu()
        out[fill] = res
    if guard:
        for k in out["nan"]:
            assert torch.isfinite(out["nan"][k]).all(), (k, "not finite with NaN bands")
            assert torch.equal(out["finite"][k], out["nan"][k]), (k, "depends on what lies behind a buffer")
    return out["nan"]


def _chain_check(irreps, F, do_norm, n, tdt, tag, guard=True):
    mul = uc.mul_of(irreps)
    c = uc.master(mul, F, n, do_norm)
    ref, ref32 = uc.evaluate_chain(c, torch.float64), uc.evaluate_chain(c, torch.float32)
    got = _chain_run(c, tdt, guard)
    names = [k for k in uc.CHAIN_OUTPUTS if do_norm or k != "stats"]      # identity norms: xeq_norm_fwd leaves stats alone, nothing reads them
    rows = lambda d: {k: uc.rows_of(k, d[k], n, mul) for k in names}
    rec = _Record(tag)
    rec.add(uc.judge(rows(ref), rows(ref32), rows(got), names, n), f"n {n}")
    rec.close()


@pytest.mark.parametrize("tdt", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("irreps,F,do_norm", CHAIN, ids=[f"{i}/{f}/norm{d}" for i, f, d in CHAIN])
def test_chain_kernels_against_the_f64_reference(irreps, F, do_norm, tdt):
    """xeq_norm_fwd / _bwd, xeq_uv_reduce_fwd / _bwd, xeq_update_out_fwd / _bwd from independent inputs, between guard bands, on both
    sides of their form switches; f32 and f64 against the same reference and bound."""
    _chain_check(irreps, F, do_norm, 33, tdt, f"chain {irreps}/{F} norm {do_norm} {'f32' if tdt == torch.float32 else 'f64'}")


@pytest.mark.parametrize("tdt", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("n", [8191, 8192])
def test_chain_kernels_across_the_nodes_per_workgroup_switch(n, tdt):
    irreps, F, do_norm = CHAIN_SWITCH
    _chain_check(irreps, F, do_norm, n, tdt, f"chain {irreps}/{F} n {n} {'f32' if tdt == torch.float32 else 'f64'}")


# ---------------------------------------------------------------------------------------------------------------- xeq_norm_param_grad
PARAM_GRAD = [((128, 64, 32), 128, (1, 16, 17, 300)), ((0, 64, 32), 36, (1, 16, 17, 300)), ((64, 32, 64), 128, (1, 16, 17, 300)),
              ((32, 0, 0), 4, (65537,))]


@pytest.mark.parametrize("mul,F,rows", PARAM_GRAD, ids=[uc.config_id(m, f) for m, f, _ in PARAM_GRAD])
def test_norm_param_grads_against_the_f64_sums(mul, F, rows):
    """fused._norm_param_grads (one xeq_norm_param_grad launch + the sum over its row chunks) against autograd in f64; at 65 537 rows
    the chunk count is capped and a chunk holds more than 16 rows.  Repeatable bit for bit."""
    D, C = uc.dims(mul)
    rec = _Record(f"{uc.config_id(mul, F)} norm_param_grad")
    for n in rows:
        c = uc.master(mul, F, n)
        ref, ref32 = uc.norm_param_grads(c, torch.float64), uc.norm_param_grads(c, torch.float32)
        s, x, g_cat = (getattr(c, k).float().to(DEV) for k in ("s", "x", "g_cat"))
        g_xh = uc.to_bt(c.g_xh, mul).float().to(DEV)
        lnw, lnb, eqw = c.lnw.float().to(DEV), c.lnb.float().to(DEV), c.eqw.float().to(DEV)
        eqb = c.eqb.float().to(DEV) if mul[0] > 0 else None
        shat, xhat, stats = torch.empty(n, F, device=DEV), torch.empty(n * D, device=DEV), torch.empty(n, 4, device=DEV)
        call("xeq_norm_fwd", lib.XEQ_F32, ptr(s), ptr(x), ptr(lnw), ptr(lnb), ptr(eqw), ptr(eqb), n, F, mul3(mul), 1, ptr(shat), F,
             ptr(xhat), ptr(stats), stream())
        first = lib.launch_count()
        chunks = int(lib.load().xeq_norm_param_grad_chunks(n))
        assert chunks == min((n + 15) // 16, 4096) and (n <= 16 * 4096 or -(-n // chunks) > 16)
        runs = []
        for _ in range(2):
            with gb.guard_allocations(fill="nan") as net:
                g = fused._norm_param_grads(s, x, stats, g_cat[:, :F], g_xh, F, mul)
            assert net.count > 0
            runs.append(torch.cat([t.reshape(-1) for t in g if t is not None]).cpu())
        assert "xeq_norm_param_grad" in lib.launch_names(first)
        assert torch.equal(runs[0], runs[1]), "not repeatable"
        assert runs[0].numel() == 2 * F + C + mul[0] and torch.isfinite(runs[0]).all()
        err, err32, bnd = float((runs[0].double() - ref).abs().max()), float((ref32.double() - ref).abs().max()), uc.bound(ref, ref32)
        rec.add([("d_params", "all", err, err32, bnd)], f"n {n}")
    rec.close()
