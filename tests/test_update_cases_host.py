"""Host side of the update kernels' cases (tests/update_cases.py): the layout table against xeq_update_uv_supported of the built
library, the refusals of both entry points, that the restatement composes to XPaiNNOracle.update and its autograd, and the POWER of
the comparison tests/test_gpu_update_kernels.py makes -- the f64 reference evaluated a second time with one deliberate defect must
move every output the defect touches beyond that output's bound, on every layout it applies to, or the bound could hide a wrong
kernel.  No GPU: the predicate and the argument checks are host logic of the built library (a refused call launches nothing)."""
import itertools

import pytest
import torch

from oracle.xpainn_oracle import XPaiNNOracle
from tests import update_cases as uc
from xequinet_amd import lib


def _supported(f64, node_dim, mul):
    return int(lib.load().xeq_update_uv_supported(lib.XEQ_F64 if f64 else lib.XEQ_F32, node_dim, lib.mul3(mul)))


def test_layout_table_is_the_predicate():
    cand = list(itertools.product(uc.MULS, repeat=3))
    assert len(cand) == 64
    assert tuple(m for m in cand if _supported(0, uc.default_node_dim(m), m)) == uc.LAYOUTS
    assert len(uc.LAYOUTS) == 33
    for mul, f in uc.CONFIGS:
        assert _supported(0, f, mul) == 1 and uc.admitted(f, mul), (mul, f)
    assert len(set(uc.CONFIGS)) == len(uc.CONFIGS) == 33 + 4 * 4
    for mul in uc.LAYOUTS:      # node_dim is independent of the layout: every multiple of 4 up to 128
        assert all(_supported(0, f, mul) == (1 if f % 4 == 0 else 0) for f in range(1, 129)), mul
    assert max(uc.dims(m)[0] for m in uc.LAYOUTS) == uc.D_MAX == uc.dims((64, 32, 64))[0]


@pytest.mark.parametrize("what,f64,node_dim,mul", uc.REFUSED, ids=[r[0] for r in uc.REFUSED])
def test_refused_rows_are_refused_by_predicate_and_entry_points(what, f64, node_dim, mul):
    assert _supported(f64, node_dim, mul) == 0 and not uc.admitted(node_dim, mul, f64=bool(f64))
    if f64:
        return   # the entry points are f32 by signature: the dtype is the predicate's argument only
    L = lib.load()
    first = lib.launch_count()
    z, m3 = None, lib.mul3(mul)
    fwd = (z, z, z, z, z, z, 4, node_dim, m3, 1, z, z, z, 1, 1e-5, z, 1024, z, z, z, None)
    bwd = (z, z, z, 1024, z, z, z, 1024, z, z, z, z, z, 4, node_dim, m3, 1, z, z, z, 1e-5, z, z, z, None)
    for name, args in (("xeq_update_uv_fwd", fwd), ("xeq_update_uv_bwd", bwd)):
        assert getattr(L, name)(*args) != 0, (what, name)
        msg = L.xeq_last_error().decode()
        assert msg.startswith(name + ": unsupported layout") and f"node_dim {node_dim}" in msg, (what, msg)
        with pytest.raises(RuntimeError, match=name):
            lib.call(name, *args)
    assert lib.launch_count() == first


COMPOSE = [((128, 64, 32), 128), ((0, 64, 32), 36), ((32, 0, 64), 32), ((128, 32, 0), 100), ((0, 128, 0), 4), ((64, 128, 0), 128)]


@pytest.mark.parametrize("layer_norm", [True, False])
@pytest.mark.parametrize("mul,node_dim", COMPOSE, ids=[uc.config_id(*c) for c in COMPOSE])
def test_restatement_composes_to_the_oracle_update_and_its_autograd(mul, node_dim, layer_norm):
    """evaluate() -> update_mlp, dot_lin -> evaluate_out() and back is XPaiNNOracle.update(0, .) with the state dict of an
    XPainnUpdate(...).double(), to 1e-12 relative to the largest element -- special rows included."""
    from xequinet_amd.nn.xpainn import XPainnUpdate

    n = 17
    m = uc.take(uc.master(mul, node_dim), n)
    torch.manual_seed(3)
    blk = XPainnUpdate(node_dim=node_dim, node_irreps=m.irreps, layer_norm=layer_norm).double().requires_grad_(False)
    with torch.no_grad():
        blk.update_U.weight.copy_(m.wu), blk.update_V.weight.copy_(m.wv), blk.update_U.bias.copy_(m.bu), blk.update_V.bias.copy_(m.bv)
        if layer_norm:
            blk.norm.weight.copy_(m.lnw), blk.norm.bias.copy_(m.lnb)
            blk.o3norm.affine_weight.copy_(m.eqw), blk.o3norm.affine_bias.copy_(m.eqb)
    sd = {"mods.update_0." + k: v for k, v in blk.state_dict().items()}
    orc = XPaiNNOracle(sd, node_dim=node_dim, node_irreps=m.irreps, layer_norm=layer_norm)
    s, x = m.s.clone().requires_grad_(), m.x.clone().requires_grad_()
    data = orc.update(0, {"node_invariant": s, "node_equivariant": x})
    s_out, x_out = data["node_invariant"], data["node_equivariant"]
    g_s, g_x = torch.autograd.grad((s_out * m.g_s_out).sum() + (x_out * m.g_x_out).sum(), [s, x])
    # the restatement, stage by stage
    fwd = uc.evaluate(m, torch.float64, int(layer_norm), 1)
    cat, p = fwd["cat"].clone().requires_grad_(), fwd["p"].clone().requires_grad_()
    a, ip = blk.update_mlp(cat), blk.dot_lin(p)
    out = uc.evaluate_out(uc.take(m, n, a=a.detach(), ip=ip.detach()), torch.float64, U=fwd["_U"])
    g_cat, g_p = torch.autograd.grad((a * out["g_a"]).sum() + (ip * out["g_ip"]).sum(), [cat, p])
    bwd = uc.evaluate(uc.take(m, n, a=a.detach(), g_cat=g_cat, g_p=g_p), torch.float64, int(layer_norm), 1)
    for name, got, want in (("s_out", out["s_out"], s_out), ("x_out", out["x_out"], x_out), ("g_s", bwd["g_s"], g_s), ("g_x", bwd["g_x"], g_x)):
        want = want.detach()
        assert torch.isfinite(want).all(), name
        assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max())), name


def test_bt_layout_is_the_one_of_the_block_front():
    from xequinet_amd.nn.fused import _bt_blocks

    mul, n = (32, 64, 32), 5
    D = uc.dims(mul)[0]
    x = torch.arange(n * D, dtype=torch.float64).reshape(n, D)
    buf = uc.to_bt(x, mul)
    off = 0
    for l, m, blk in _bt_blocks(buf, n, mul, 1):
        d = 2 * l + 1
        assert torch.equal(blk.view(n, d, m), x[:, off:off + m * d].view(n, m, d).transpose(1, 2))
        off += m * d
    pair = uc.to_bt(x, mul, pair=-x)
    for (l, m, blk), (_, _, one) in zip(_bt_blocks(pair, n, mul, 2), _bt_blocks(buf, n, mul, 1)):
        assert torch.equal(blk[:, :m], one) and torch.equal(blk[:, m:], -one)
    assert torch.equal(uc.from_bt(buf, n, mul)[2], uc.from_bt(uc.to_bt(x[2:3], mul), 1, mul)[0])


def test_a_case_is_the_first_rows_of_its_master():
    a, b = uc.case((64, 32, 32), 64, 17), uc.case((64, 32, 32), 64, 65)
    for k in uc.FWD_OUTPUTS + uc.BWD_OUTPUTS:
        assert torch.equal(a.ref[k], b.ref[k][:17]) and a.ref[k].dtype == torch.float64 and a.ref32[k].dtype == torch.float32
    m = uc.master((64, 32, 32), 64)
    assert not m.s[uc.ZERO_ROW].any() and not m.x[uc.ZERO_ROW].any() and float(m.x[uc.BIG_ROW].abs().max()) > 1e3
    long = uc.master((32, 0, 0), 32, 8200)      # a longer draw starts with the rows of the shorter one
    assert all(torch.equal(getattr(long, k)[:65], getattr(uc.master((32, 0, 0), 32), k)) for k in uc.INPUTS)
    assert all(torch.equal(getattr(long, k), getattr(uc.master((32, 0, 0), 32), k)) for k in uc.PARAMS)


DEFECTS = [(mul, mut) for mul in uc.LAYOUTS for mut in sorted(uc.MUTATIONS) if uc.MUTATIONS[mut][1](mul)]


@pytest.mark.parametrize("mul,mutation", DEFECTS, ids=[f"{uc.config_id(m, uc.default_node_dim(m))}-{k}" for m, k in DEFECTS])
def test_every_defect_leaves_the_bound(mul, mutation):
    """On the committed inputs at 17 and 33 rows: at least one of the outputs the defect touches moves beyond that output's bound in one
    of its row groups.  (eps^2: judged on the zero row, without norms and bias -- V = 0 there, so only eps^2 keeps g_V finite.)"""
    f = uc.default_node_dim(mul)
    do_norm, has_bias = (0, 0) if mutation == "no_eps2" else (1, 1)
    names = uc.MUTATIONS[mutation][0]
    for n in (17, 33):
        c = uc.case(mul, f, n, do_norm, has_bias)
        bad = uc.evaluate(uc.take(c, n), torch.float64, do_norm, has_bias, 1, mutation)
        bad = {k: uc.rows_of(k, bad[k], n, mul) for k in names}
        res = uc.judge(c.ref, c.ref32, bad, names, n)
        if mutation == "no_eps2":
            res = [r for r in res if r[1] == "zero"]
        assert any(err > bnd for _, _, err, _, bnd in res), (mul, n, mutation, res)
        # and every output listed for the defect is one it moves: the list is not padded
        moved = {k for k, _, err, _, bnd in res if err > bnd}
        assert moved == set(names), (mul, n, mutation, sorted(set(names) - moved))
