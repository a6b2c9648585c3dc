"""Host side of the training pass's node-kernel cases (tests/train_node_cases.py): the restatement against torch's layer norm,
nn.training.equivariant_layer_norm / the oracle's and the formulas of nn.training.update's tensor form; the properties the case list
claims; the condition of the f32 inputs; and the POWER of the comparison tests/test_gpu_train_node.py makes -- the f64 restatement
evaluated a second time with one deliberate defect must leave the GPU test's widest bound (the f32 one) in every output the defect
names, and stay inside the tightest (the f64 one) in every other.  No GPU."""
import pytest
import torch
import torch.nn.functional as tf

from oracle import xpainn_oracle as xo
from tests import train_node_cases as tc
from tests import update_cases as uc

AGAINST = [(128, (128, 64, 32)), (96, (96, 33, 7)), (32, (0, 16, 8))]


def _close(got, want, what):
    assert got.shape == want.shape, what
    assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max())), what


@pytest.mark.parametrize("F,mul", AGAINST, ids=[tc.config_id(*c) for c in AGAINST])
def test_restatement_is_the_modules_arithmetic(F, mul):
    """norm = F.layer_norm and the oracle's / nn.training's equivariant layer norm; uv and out = the formulas of nn.training.update's
    tensor form on the e3nn rows; special rows included."""
    from xequinet_amd import o3
    from xequinet_amd.nn import training
    from xequinet_amd.nn.o3layer import EquivariantLayerNorm

    c = tc.master(F, mul)
    D, C = uc.dims(mul)
    o_s, o_x = tc.norm(c.s, c.x, c.lnw, c.lnb, c.eqw, c.eqb, F, mul, tc.EPS_LN, tc.EPS_EQ)
    _close(o_s, tf.layer_norm(c.s, (F,), c.lnw, c.lnb, tc.EPS_LN), "layer norm")
    _close(o_x, xo.equivariant_layer_norm(uc.irreps_of(mul), c.x, c.eqw, c.eqb), "oracle's equivariant layer norm")
    _close(o_x, uc._eq_layer_norm(uc.irreps_of(mul), mul, c.x, c.eqw, c.eqb)[0], "update_cases' equivariant layer norm")
    eq = EquivariantLayerNorm(o3.Irreps(uc.irreps_of(mul))).double().requires_grad_(False)
    eq.affine_weight.copy_(c.eqw), eq.affine_bias.copy_(c.eqb)
    if mul[0] > 0:      # (the tensor form divides by the number of 0e channels: without any, the oracle alone is the reference)
        _close(o_x, training.equivariant_layer_norm(eq, c.x), "nn.training's equivariant layer norm")
    per_row = tc.norm(c.s, c.x, *[tc._per_row(getattr(c, k), c.n) for k in tc.PARAMS], F, mul, tc.EPS_LN, tc.EPS_EQ)
    assert torch.equal(per_row[0], o_s) and torch.equal(per_row[1], o_x)          # a copy of the parameters per row changes nothing
    # nn.training.update, tensor form: v_norm, the channel dot, U (x) a_vv, a_sv inner + a_ss
    ir = uc.irreps_of(mul)
    uvs = tc.uv_list(c.U, c.V, mul)
    vd = tc.uv(*uvs, mul, tc.EPS_INV)
    _close(vd[:, :C], xo.invariant(ir, c.V, eps=tc.EPS_INV), "Invariant")
    _close(vd[:, C:], xo.equivariant_dot(ir, c.U, c.V), "channel dot")
    d_s, d_x = tc.out(*uvs, c.a, c.inner, F, mul)
    a_vv, a_sv, a_ss = torch.split(c.a, [C, F, F], -1)
    _close(d_s, a_sv * c.inner + a_ss, "a_sv inner + a_ss")
    _close(d_x, xo.elementwise_tp(ir, c.U, a_vv), "U (x) a_vv")
    # the uv tensors are the blocks of the BT pair buffer (nn/fused.py::_bt_blocks)
    assert torch.equal(torch.cat([t.reshape(-1) for t in uvs]), uc.to_bt(c.U, mul, pair=c.V))
    assert torch.equal(tc.uv_rows(uvs, c.n), uc.from_bt(uc.to_bt(c.U, mul, pair=c.V), c.n, mul, 2))
    rows = tc.uv_rows(tc.uv_list(torch.zeros_like(c.U), torch.ones_like(c.V), mul), c.n)
    assert torch.equal(rows[0] == 1, tc.v_half(mul))


@pytest.mark.parametrize("F,mul", AGAINST, ids=[tc.config_id(*c) for c in AGAINST])
def test_written_reverse_and_its_tangents_are_autograds(F, mul):
    """eq_norm_reverse (the body the two tangent defects are restated on) is autograd's J^T g, and its tangent along u, like the
    tangent of eq_norm, is what three_orders returns for the second order."""
    from torch.autograd.functional import jvp

    n = 17
    c = tc.take(tc.master(F, mul), n)
    ref = tc.evaluate("norm0", c, torch.float64)
    ew, eb = tc._per_row(c.eqw, n), tc._per_row(c.eqb, n)
    d_x, d_ew = tc.eq_norm_reverse(c.x, c.g_x, ew, mul, tc.EPS_EQ)
    C = sum(mul)
    for got, want, what in ((d_x, ref["d_x"], "d_x"), (d_ew, ref["rows"][:, 2 * F:2 * F + C], "d eq_w")):
        for idx in tc.groups(n).values():
            _close(got[idx], want[idx], what)
    dd_x, dd_ew = jvp(lambda v: tc.eq_norm_reverse(v, c.g_x, ew, mul, tc.EPS_EQ), c.x, c.u_x)[1]
    dg_x = jvp(lambda v: tc.eq_norm(v, ew, eb, mul, tc.EPS_EQ), c.x, c.u_x)[1]
    for got, want, what in ((dd_x, ref["dd_x"], "dd_x"), (dd_ew, ref["dd_rows"][:, 2 * F:2 * F + C], "tangent of d eq_w"), (dg_x, ref["dg_x"], "dg_x")):
        for idx in tc.groups(n).values():
            assert float((got[idx] - want[idx]).abs().max()) <= 1e-11 * max(1.0, float(want[idx].abs().max())), what
    # the parameter cotangents carry no tangent, and nothing depends on V in ``out``
    assert not ref["dd_rows"][:, F:2 * F].any() and not ref["dd_rows"][:, 2 * F + C:].any()
    o = tc.evaluate("out", c, torch.float64)
    assert not o["d_uv"][:, tc.v_half(mul)].any() and not o["dd_uv"][:, tc.v_half(mul)].any()


def test_layout_one_is_layout_zero_re_laid():
    F, mul, n = 96, (96, 33, 7), 5
    c = tc.take(tc.master(F, mul), n)
    a, b = tc.evaluate("norm0", c, torch.float64), tc.evaluate("norm1", c, torch.float64)
    relay = lambda v: uc.from_bt(uc.to_bt(v, mul), n, mul)
    for k in tc.outputs("norm0"):
        want = relay(a[k]) if k in ("o_x", "dg_x") else a[k]
        _close(b[k], want, k)
    assert not torch.equal(relay(a["o_x"]), a["o_x"])


def test_case_list_has_the_properties_it_claims():
    muls = [m for _, m in tc.CONFIGS]
    for l in range(3):
        assert any(m[l] == 0 for m in muls) and any(m[l] > 0 for m in muls), l
    assert any(sum(m) < F for F, m in tc.CONFIGS) and any(sum(m) > F for F, m in tc.CONFIGS)
    assert any(F % 64 and uc.dims(m)[0] % 64 and F > 64 for F, m in tc.CONFIGS)          # a partial last lane round after whole ones
    assert max(uc.dims(m)[0] for _, m in tc.CONFIGS) == 608 == 9 * 64 + 32                # ten lane rounds, the last one half full
    assert any(len({m[0], m[1], m[2]}) == 3 and all(m) for _, m in tc.CONFIGS)            # BT blocks of three different widths
    assert any(n < 4 for n in tc.ROWS) and 4 in tc.ROWS and any(n > 4 and n % 4 for n in tc.ROWS)
    for F, m in tc.CONFIGS + (tc.LONG,):
        C = sum(m)
        assert (257 * C) % 256 and (257 * max(C, F)) % 256, (F, m)                        # a partial last block of k_uv and k_out
    assert tc.LONG_ROWS > tc.GRID_ROWS == 4 * 4096 and (tc.LONG_ROWS - tc.GRID_ROWS) % 4      # a second round with a partial last block
    assert tc.LONG[0] + uc.dims(tc.LONG[1])[0] == 152                                         # floats of (s, x) per row
    assert set(tc.FUNCTION_CONFIGS) <= set(tc.CONFIGS)
    assert max(tc.NEAR_ROWS) < 63 and not {uc.ZERO_ROW, uc.BIG_ROW} & set(tc.NEAR_ROWS)
    assert uc.ZERO_ROW < 63 and uc.BIG_ROW < 63


def test_a_case_is_the_first_rows_of_its_master_and_f32_representable():
    F, mul = tc.LONG
    long, short = tc.master(F, mul, tc.LONG_ROWS), tc.master(F, mul)
    for k in tc.ROW_TENSORS:
        assert torch.equal(getattr(long, k)[:tc.ROWS_MASTER], getattr(short, k)), k
        assert torch.equal(getattr(long, k).float().double(), getattr(long, k)), k
    for k in tc.PARAMS:
        assert torch.equal(getattr(long, k), getattr(short, k)), k
    for k in tc.SPECIAL:
        assert not getattr(short, k)[uc.ZERO_ROW].any() and float(getattr(short, k)[uc.BIG_ROW].abs().max()) > 1e3
    a, b = tc.case("uv", F, mul, 63), tc.case("uv", F, mul, 257)
    for k in tc.outputs("uv"):
        assert torch.equal(a.ref[k], b.ref[k][:63]) and a.ref[k].dtype == torch.float64 and a.ref32[k].dtype == torch.float32


def test_f32_inputs_keep_the_scalar_channels_of_v_away_from_zero():
    """Both facts about the drawn inputs: every f32 case has |V_0| >= 0.5 (the zero row apart: V = 0 exactly there, and the second
    derivative is 1 / eps whatever the rounding); the near-zero values are in the f64-only variant.  And the reason, on 4096 x 128
    entries of N(0, 1): with unbounded V the f32 chain's own second-order error is 1e-2, on entries up to 1e4 ... 1e5 -- a thousand times
    the 4-ulp floor the other entries of the output would have, so such a draw either fails or, through its largest entry, hides every
    other entry behind a floor of 1e-2; with the bound the error is 2e-6, below that floor."""
    for F, mul in tc.CONFIGS + (tc.LONG,):
        n = tc.LONG_ROWS if (F, mul) == tc.LONG else tc.ROWS_MASTER
        v0 = tc.master(F, mul, n).V[:, :mul[0]]
        keep = [r for r in range(n) if r != uc.ZERO_ROW]
        assert mul[0] == 0 or float(v0[keep].abs().min()) >= tc.V0_MIN, (F, mul)
        near = tc.master(F, mul, tc.ROWS_MASTER, True).V[:, :mul[0]]
        for r, val in zip(tc.NEAR_ROWS, tc.NEAR_VALUES):
            assert bool((near[r] == torch.tensor(val, dtype=torch.float32).double()).all())
        assert torch.equal(near[[r for r in range(tc.ROWS_MASTER) if r not in tc.NEAR_ROWS]], v0[[r for r in range(tc.ROWS_MASTER) if r not in tc.NEAR_ROWS]])
    g = torch.Generator().manual_seed(0)
    V, u, gv = (torch.randn(4096, 128, generator=g, dtype=torch.float64).float().double() for _ in range(3))

    def second(V, dtype):
        V = V.to(dtype).requires_grad_()
        (d,) = torch.autograd.grad(torch.sqrt(V * V + tc.EPS_INV ** 2) - tc.EPS_INV, V, gv.to(dtype), create_graph=True)
        return torch.autograd.grad(d, V, u.to(dtype))[0].double()

    free, top = float((second(V, torch.float32) - second(V, torch.float64)).abs().max()), float(second(V, torch.float64).abs().max())
    Vb = torch.sign(V) * (tc.V0_MIN + V.abs())
    bounded = float((second(Vb, torch.float32) - second(Vb, torch.float64)).abs().max())
    print(f"second derivative of Invariant, f32 against f64: unbounded V {free:.2e} on entries up to {top:.2e}, |V| >= {tc.V0_MIN} {bounded:.2e}")
    floor = tc.F32_FACTOR * tc.EPS32 * 20.0         # 4 ulp of the largest second-order entry of uv's ordinary rows (about 20)
    assert free > 100 * floor and top > 1e3 and bounded < floor


def _moved(res, which):
    return {k for k, _, err, _, bnd in res if not err <= bnd}


@pytest.mark.parametrize("mutation", sorted(tc.MUTATIONS))
def test_every_defect_leaves_the_bound(mutation):
    """At its smallest applicable case: every output the defect names leaves the f32 bound (the widest the GPU test applies) in one of
    its row groups, every other output stays inside the f64 bound (the tightest), and the unmutated f32 restatement is inside both
    precisions' rule where it applies to it."""
    kind, names, (F, mul, n) = tc.MUTATIONS[mutation]
    c = tc.case(kind, F, mul, n)
    bad = tc.evaluate(kind, tc.take(c, n), torch.float64, mutation)
    every = tc.outputs(kind)
    wide = tc.judge(c.ref, c.ref32, bad, every, n, f64=False)
    tight = tc.judge(c.ref, c.ref32, bad, every, n, f64=True)
    assert _moved(wide, "f32") == set(names), (mutation, sorted(_moved(wide, "f32") ^ set(names)), wide)
    assert _moved(tight, "f64") == set(names), (mutation, sorted(_moved(tight, "f64") ^ set(names)))
    own = tc.judge(c.ref, c.ref32, {k: v.double() for k, v in c.ref32.items()}, every, n, f64=False)
    assert not _moved(own, "f32"), own


@pytest.mark.parametrize("kind", tc.KINDS)
def test_unmutated_f32_restatement_is_inside_every_bound(kind):
    for F, mul in tc.CONFIGS:
        for n in (5, 257):
            c = tc.case(kind, F, mul, n)
            res = tc.judge(c.ref, c.ref32, {k: v.double() for k, v in c.ref32.items()}, tc.outputs(kind), n, f64=False)
            assert not _moved(res, "f32"), (kind, F, mul, n, [r for r in res if not r[2] <= r[4]])
            assert all(torch.isfinite(v).all() for v in c.ref.values()) and all(torch.isfinite(v).all() for v in c.ref32.values())


def test_near_zero_rows_are_a_group_of_their_own_in_f64():
    """The f64-only group: the second order through Invariant at V_0 = 0 ... 1e-3 is finite and of the order 1 / eps = 1e5, a thousand
    times the ordinary rows' largest entry -- judged with them it would set their bound."""
    F, mul, n = 128, (128, 64, 32), 63
    c = tc.case("uv", F, mul, n, near=True)
    grp = tc.groups(n, True)
    assert grp["near"] == list(tc.NEAR_ROWS) and not set(grp["near"]) & set(grp["ordinary"])
    top, ordinary = float(c.ref["dd_uv"][grp["near"]].abs().max()), float(c.ref["dd_uv"][grp["ordinary"]].abs().max())
    assert torch.isfinite(c.ref["dd_uv"]).all() and 1e4 < top < 1e7 and top > 1e3 * ordinary
    assert "near" not in tc.groups(n, False) and "near" not in tc.groups(5, True)
