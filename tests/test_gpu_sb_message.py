"""The scalar-broadcast message kernels (csrc/xeq_message_sb.hip: forward, reverse, their few-row form, the second-order pair and
product kernels) through the public ops under XEQ_MESSAGE_IMPL=sb at every basis count the family admits and at the channel layouts of
tests/sb_message_cases.py, against the f64 references of that module.

The basis count picks the instantiation (records of 8, 16, 20 or 32 operands per filter); f32 with at most 512 nodes and 9 .. 20 basis
functions stages its records in LDS (the few-row form, one instantiation of 20 operands), so every f32 case runs twice -- few-row forms
forced off, and the default -- and the two must agree bit for bit at every count.  (They did not at 5 .. 8 while the few-row form was
admitted there: x_out differed in its last bits between the 20-operand staged kernel and the general 8-operand one, so a system of 512
and one of 513 nodes got different results.  The dispatch now leaves those counts to the general form, as it does 1 .. 4.)  The degrees list holds segments on both sides of
one and of two groups of 64 edges; the walk list runs the persistent walk at every form of its grid and chunk.

Bounds (tests/wq_message_cases.py::bound): 2e-5 max(1, max|ref|) in f32, widened only to 1.5 x the CPU f32 restatement's own error --
which tests/test_sb_message_cases_host.py shows takes effect for no tensor of any case -- and 1e-11 max(1, max|ref|) in f64.  Every
error is printed with its bound; the worst ratio per (instantiation, dtype, form) goes to the parity record."""
import contextlib

import numpy as np
import pytest
import torch

from tests import guard_bands, parity_record
from tests import sb_message_cases as sc
from tests import wq_message_cases as wc
from tests.test_gpu_small_rows import _forms
from xequinet_amd import lib

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, F64 = torch.float32, torch.float64
RUNS, RUN_IDS = [(F32, True), (F32, False), (F64, False)], ["f32-general", "f32-default", "f64"]
WORST = {}   # (operands per filter, dtype, form) -> (err / bound, err, bound, tensor, case)


@pytest.fixture(scope="module", autouse=True)
def _parity_records():
    yield
    for (mb, dt, form), (ratio, err, bnd, name, case) in sorted(WORST.items()):
        print(f"sb worst MAXB={mb} {dt} {form}: err {err:.3e} bound {bnd:.3e} ({ratio:.3f} of it) {name} {case}")
        parity_record.add({"test": f"sb:message:MAXB={mb}:{dt}:{form}", "err": err, "bound": bnd, "err_over_bound": ratio, "output": name, "case": case})


@pytest.fixture(autouse=True)
def _sb(monkeypatch):
    monkeypatch.setenv("XEQ_MESSAGE_IMPL", "sb")
    monkeypatch.delenv("XEQ_SMALL_ROWS", raising=False)


def _form(general):
    """the few-row forms forced off, or the library's default"""
    return _forms(0) if general else contextlib.nullcontext()


def _staged(c, dtype, general):
    """whether this run takes the few-row form (csrc/xeq_message_sb.hip, sb_stage_form), from the sizes alone"""
    return dtype == F32 and not general and 9 <= c.B <= 20 and c.n <= sc.FEW_ROW_NODES


def _key(c, dtype, general, what=""):
    staged = _staged(c, dtype, general)
    return (20 if staged else sc.maxb(c.B), "f32" if dtype == F32 else "f64", what + ("few-row" if staged else "general"))


def _bound(c, k, dtype):
    ref = c.ref[k]
    if dtype == F64:
        return sc.TOL_F64 * max(1.0, float(ref.abs().max()))
    return wc.bound(ref, c.ref32[k], sc.TOL_F32)


def _compare(c, got, names, dtype, key, tag="", ref=None, ref32=None):
    """``ref`` / ``ref32``: a restated reference (f64, and in f32) in place of the case's own"""
    failed = []
    for k in names:
        want = c.ref[k] if ref is None else ref[k]
        g = got[k].detach().cpu().double()
        assert g.shape == want.shape and torch.isfinite(g).all(), (c.id, k)
        if want.numel() == 0:
            continue
        err = float((g - want).abs().max())
        if ref is None:
            bnd = _bound(c, k, dtype)
        else:
            bnd = sc.TOL_F64 * max(1.0, float(want.abs().max())) if dtype == F64 else wc.bound(want, ref32[k], sc.TOL_F32)
        print(f"{c.id}{tag} {key[1]} {key[2]} {k}: err {err:.3e} bound {bnd:.3e}")
        if key not in WORST or err / bnd > WORST[key][0]:
            WORST[key] = (err / bnd, err, bnd, k, c.id + tag)
        if not err <= bnd:
            failed.append((k, err, bnd))
    assert not failed, (c.id + tag, key, failed)


def _dev(t, dtype):
    return None if t is None else t.to(dtype).to(DEV).contiguous()


def _graph(c):
    from xequinet_amd import ops

    return ops.EdgeGraph(torch.tensor(c.edges.edge_index, device=DEV), c.n)


def _run(c, dtype, layout=0, general=False):
    """message_forward + message_backward of a case -> results by reference name, on the device (the BT layout undone on dL/dxhat);
    ``general``: the few-row forms forced off"""
    from xequinet_amd import ops

    with _form(general):
        graph = _graph(c)
        cfg = (c.rbf_kind, c.cutoff_kind, c.B, c.cutoff, c.F, c.mul, layout)
        xhat = _dev(c.xhat if layout == 0 else wc.to_bt(c.xhat, c.mul), dtype)
        n0 = lib.launch_count()
        s_out, x_out, saved, impl = ops.message_forward(_dev(c.h, dtype), xhat, _dev(c.vec, dtype), _dev(c.s, dtype), _dev(c.x, dtype), _dev(c.W, dtype),
                                                        _dev(c.b, dtype), _dev(c.p0, dtype), _dev(c.p1, dtype), graph, cfg, want_backward=True)
        assert impl == "sb"
        g_h, g_xhat, g_vec, gs_in, gx_in = ops.message_backward(saved, graph, cfg, impl, _dev(c.g_s, dtype), _dev(c.g_x, dtype))
        names = lib.launch_names(n0)
    assert names.count("xeq_message_fwd_sb") == 1 and names.count("xeq_message_bwd_sb") == 1 and not any("_wq" in n for n in names), names
    g_xhat = g_xhat.reshape(c.n, c.D) if layout == 0 else wc.from_bt(g_xhat.reshape(-1), c.mul, c.n)
    torch.cuda.synchronize()
    return dict(zip(sc.OUTPUTS, (s_out, x_out, g_h, g_xhat, g_vec, gs_in, gx_in)))


def _check_exact(c, got, dtype, degrees_list=True):
    """What must hold to the bit: the residual rows of nodes without a walked edge, zero node gradients for nodes nobody lists, and
    zero dL/dvec on every edge at or beyond the cutoff."""
    el = c.edges
    fwd_empty, rev_empty = torch.tensor(np.diff(el.c_rowptr) == 0), torch.tensor(np.diff(el.n_rowptr) == 0)
    if degrees_list:
        assert int(fwd_empty.sum()) >= 3 and bool(fwd_empty[-1]) and int(rev_empty.sum()) >= 3 and bool(rev_empty[-1]) and int(c.beyond.sum()) >= 3
    s_out, x_out = got["s_out"].cpu(), got["x_out"].cpu()
    assert torch.equal(s_out[fwd_empty], c.s.to(dtype)[fwd_empty]) and torch.equal(x_out[fwd_empty], c.x.to(dtype)[fwd_empty])
    if (~fwd_empty).any() and not bool(c.beyond.all()):
        assert not torch.equal(s_out[~fwd_empty], c.s.to(dtype)[~fwd_empty])
    if rev_empty.any():
        assert float(got["grad_h"].cpu()[rev_empty].abs().max()) == 0.0 and float(got["grad_xhat"].cpu()[rev_empty].abs().max()) == 0.0
    if c.beyond.any():
        assert float(got["grad_vec"].cpu()[c.beyond].abs().max()) == 0.0


def _both_forms_and_f64(c, layout=0, tag=""):
    """f32 with the few-row forms off and by default (bit-equal), f64; all seven outputs against the reference, and the exact properties"""
    runs = {(F32, True): _run(c, F32, layout, general=True), (F32, False): _run(c, F32, layout), (F64, False): _run(c, F64, layout)}
    for k in sc.OUTPUTS:
        assert torch.equal(runs[(F32, True)][k], runs[(F32, False)][k]), (c.id, k, "the few-row form against the general form")
    for (dtype, general), got in runs.items():
        _compare(c, got, sc.OUTPUTS, dtype, _key(c, dtype, general), tag=tag)
        _check_exact(c, got, dtype)


# ------------------------------------------------------------------------------------------------------- every case of the table
@pytest.mark.parametrize("row", sc.TABLE, ids=[sc.case_id(*r) for r in sc.TABLE])
def test_every_case_of_the_table(row):
    """Directed degrees list.  At 9 .. 20 basis functions the default f32 run is the few-row form and the bit-equality is form against
    form.  At 1 .. 4 the few-row form would read four filter operands behind its record of 16 floats -- for a group's last edge an LDS
    slot nobody staged -- with zero weights: the dispatch leaves these counts (and 5 .. 8, see above) to the general form
    (sb_stage_form), so both f32 runs are the same kernel there.  Were that undone at 1 .. 4, this comparison would catch the read only
    when the stale words are not finite (0 x NaN); finite stale words leave no trace, and nothing here tries to force the other kind."""
    _both_forms_and_f64(sc.message_case(*row))


@pytest.mark.parametrize("B", sc.KIND_COUNTS)
@pytest.mark.parametrize("kind", sc.LIST_KINDS[1:])
def test_other_list_kinds(kind, B):
    """Unsorted centers (a permuted forward walk), the long segments on the reverse walk (transpose), both walks (symmetric)"""
    _both_forms_and_f64(sc.message_case(*sc.MAIN, B, list_kind=kind))


@pytest.mark.parametrize("B", sc.KIND_COUNTS)
def test_bt_layout_of_xhat(B):
    _both_forms_and_f64(sc.message_case(*sc.MAIN, B), layout=1, tag=" BT")


@pytest.mark.parametrize("n", [512, 513])
def test_few_row_limit(n):
    """The last node count that takes the few-row form and the first that does not (isolated nodes appended): the bits of the forced
    general run, and the reference's values."""
    c = sc.message_case(*sc.MAIN, 20, extra_isolated=n - sc.N_NODES)
    assert c.n == n and (n <= sc.FEW_ROW_NODES) == _staged(c, F32, False)
    general, default = _run(c, F32, general=True), _run(c, F32)
    for k in sc.OUTPUTS:
        assert torch.equal(general[k], default[k]), k
    _compare(c, default, sc.OUTPUTS, F32, _key(c, F32, False))
    _check_exact(c, default, F32)


# -------------------------------------------------------------------------------------------------------------- the walk list
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("n", sc.WALK_NODES)
def test_persistent_walk(n, dtype):
    """Every allocation of the ops between guard bands, outputs pre-filled with the never-written pattern: a node the walk does not
    visit shows as unwritten rows, a store outside a buffer as a changed band; values against the reference."""
    c = sc.walk_case(n)
    with guard_bands.guard_allocations() as guards:
        got = _run(c, dtype)
        torch.cuda.synchronize()
    assert guards.count >= 7
    for k in sc.OUTPUTS[:5]:
        assert not bool(guard_bands.unwritten(got[k]).any()), (k, int(guard_bands.unwritten(got[k]).any(-1).sum()))
    _compare(c, got, sc.OUTPUTS, dtype, _key(c, dtype, False, what="walk "))
    _check_exact(c, got, dtype, degrees_list=False)


# ---------------------------------------------------------------------------------------------------------------------- flags
def _raw_inputs(c, dtype):
    from xequinet_amd import ops

    graph = _graph(c)
    t = {k: _dev(getattr(c, k), dtype) for k in ("h", "xhat", "vec", "s", "x", "W", "b", "g_s", "g_x")}
    basis, dbasis = ops.edge_basis(t["vec"], graph, c.rbf_kind, c.cutoff_kind, c.B, c.cutoff, _dev(c.p0, dtype).reshape(-1), None if c.p1 is None else _dev(c.p1, dtype).reshape(-1))
    return graph, t, basis, dbasis


def _raw_bwd(c, graph, t, basis, dbasis, grad_vec, flags):
    p = lib.ptr
    g_h, g_xhat = torch.empty_like(t["h"]), torch.empty_like(t["xhat"])
    lib.call("xeq_message_bwd_sb", lib.dtype_code(t["h"]), c.n, c.edges.n_edges, p(graph.n_rowptr), p(graph.n_perm), p(graph.edge_index[0]), p(basis), p(dbasis),
             p(t["h"]), p(t["xhat"]), p(t["g_s"]), p(t["g_x"]), p(t["W"]), p(t["b"]), c.B, c.F, lib.mul3(c.mul), p(g_h), p(g_xhat), p(grad_vec), flags, lib.stream())
    return g_h, g_xhat


@pytest.mark.parametrize("dtype,general", RUNS, ids=RUN_IDS)
@pytest.mark.parametrize("B", [4, 8, 20, 32])
@pytest.mark.parametrize("kind", ["directed", "transpose"])
def test_accumulating_edge_gradient(kind, B, dtype, general):
    """XEQ_SB_ACCUM_VEC: the kernel adds its dL/dvec to what the buffer holds -- one addition per element, so the result is torch's
    g0 + plain to the bit -- and the node gradients do not depend on the flag."""
    c = sc.message_case(*sc.MAIN, B, list_kind=kind)
    with _form(general):
        graph, t, basis, dbasis = _raw_inputs(c, dtype)
        plain = torch.empty_like(t["vec"])
        g_h, g_xhat = _raw_bwd(c, graph, t, basis, dbasis, plain, 0)
        g0 = torch.randn(c.edges.n_edges, 3, generator=torch.Generator().manual_seed(B), dtype=torch.float64).to(dtype).to(DEV) * 3.0
        buf = g0.clone()
        a_h, a_xhat = _raw_bwd(c, graph, t, basis, dbasis, buf, lib.SB_ACCUM_VEC)
        torch.cuda.synchronize()
    assert torch.equal(buf, g0 + plain) and torch.equal(a_h, g_h) and torch.equal(a_xhat, g_xhat)
    assert torch.equal(buf[c.beyond.to(DEV)], g0[c.beyond.to(DEV)])            # dead edges add an exact zero
    _compare(c, {"grad_vec": plain, "grad_h": g_h, "grad_xhat": g_xhat}, ("grad_vec", "grad_h", "grad_xhat"), dtype, _key(c, dtype, general), tag=" raw")


@pytest.mark.parametrize("dtype,general", RUNS, ids=RUN_IDS)
@pytest.mark.parametrize("B", [4, 20, 32])
@pytest.mark.parametrize("layout", [sc.MAIN, (16, (0, 16, 0)), (7, (5, 0, 3))], ids=["main", "l1-only", "no-l1"])
def test_forward_flags(layout, B, dtype, general):
    """XEQ_SB_Y0_ZERO: the forward with the l = 0 harmonic counted as 0 (no trace on a layout without l = 0 channels);
    s_in = x_in = NULL: the aggregate alone, with and without the flag."""
    c = sc.message_case(*layout, B)
    p = lib.ptr
    with _form(general):
        graph, t, basis, _ = _raw_inputs(c, dtype)
        for y0_zero, residual in ((True, True), (True, False), (False, False)):
            s_out, x_out = torch.empty_like(t["s"]), torch.empty_like(t["x"])
            lib.call("xeq_message_fwd_sb", lib.dtype_code(t["h"]), c.n, c.edges.n_edges, p(graph.c_rowptr), p(graph.c_perm), p(graph.edge_index[1]), p(basis),
                     p(t["h"]), p(t["xhat"]), p(t["s"]) if residual else None, p(t["x"]) if residual else None, p(t["W"]), p(t["b"]), c.B, c.F,
                     lib.mul3(c.mul), p(s_out), p(x_out), lib.SB_Y0_ZERO if y0_zero else 0, lib.stream())
            torch.cuda.synchronize()
            want = sc.message_eval(c, torch.float64, y00=0.0 if y0_zero else None, residual=residual)
            want32 = sc.message_eval(c, torch.float32, y00=0.0 if y0_zero else None, residual=residual)
            if y0_zero:         # what the flag is worth in this case: nothing without l = 0 channels, far above any bound with them
                moved = float((want["x_out"] - sc.message_eval(c, torch.float64, residual=residual)["x_out"]).abs().max())
                assert moved == 0.0 if c.mul[0] == 0 else moved > 1.0
            _compare(c, {"s_out": s_out, "x_out": x_out}, ("s_out", "x_out"), dtype, _key(c, dtype, general), tag=f" y0_zero={int(y0_zero)} residual={int(residual)}", ref=want, ref32=want32)


# --------------------------------------------------------------------------------------------------------------- second order
@pytest.mark.parametrize("B", sc.DIFF_COUNTS)
@pytest.mark.parametrize("layout", sc.DIFF_LAYOUTS, ids=["main", "256"])
def test_second_order_at_width(layout, B):
    """ops.DiffMessage at 576 and 768 filter rows (the second and third channel slot of xeq_message_q_wgrad's threads) on the degrees
    list: f64 against the CPU f64 reference, f32 against f64 -- values, first-order gradients of a quadratic in them, second-order
    gradients of a quadratic in those."""
    from xequinet_amd import ops

    c = sc.diff_case(*layout, B)
    E = c.edges.n_edges
    n_chunks = int(lib.load().xeq_message_q_wgrad_chunks(E))
    assert c.H > 512 and n_chunks >= 3 and E % 512 != 0 and n_chunks == -(-E // 512)          # a ragged last chunk
    graph = ops.EdgeGraph(torch.tensor(c.edges.edge_index, device=DEV), c.n)
    cfg = (c.B, c.F, c.mul)
    for dtype in (F64, F32):
        leaves = [_dev(v, dtype).requires_grad_() for v in (c.h, c.xhat, c.rec, c.w, c.b)]
        assert ops.diff_message_supported(leaves[0], graph, cfg)
        ops.KERNEL_TIMER.reset(True)
        try:
            got = sc.diff_triple(lambda *a: ops.DiffMessage.apply(*a, graph, cfg), leaves)
            launched = ops.KERNEL_TIMER.summary()
        finally:
            ops.KERNEL_TIMER.reset(False)
        assert {"xeq_message_fwd_sb", "xeq_message_bwd_sbq", "xeq_message_fwd_sb_pair", "xeq_message_bwd_sbq_pair", "xeq_message_q_wgrad"} <= set(launched), launched
        _compare(c, got, sc.DIFF_NAMES, dtype, (sc.maxb(B), "f32" if dtype == F32 else "f64", "second order"))
