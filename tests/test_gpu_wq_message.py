"""The wave / quad matrix-core message kernels (csrc/xeq_message_wq.hip: records, packed weights, forward, reverse, edge gradients) and
the matrix-core filter-gradient kernel (csrc/xeq_train.hip) through the public ops at every basis count and channel layout that
``xeq_message_wq_supported`` admits, against the f64 references of tests/wq_message_cases.py.

The basis count decides the form of the code: the number of exact-f32 tail steps (1, 3, 4, 5 .. 8, of which the kernels are instantiated
for 1, 3, 4 and 8 -- 24 .. 29 basis functions run the 8-step kernels on zero-filled tail positions), a bf16 tail block up to 20, and
records of 40 floats up to 23 and 48 above.  The table holds every step count, both sides of every boundary, both record widths, and
six more channel layouts (scalars only, no l = 1, no l = 2, widths above 128, five units per l) at one count per instantiation.

Bounds (tests/wq_message_cases.py::bound): 2e-5 max(1, max|ref|) for outputs and first-order gradients, 3e-5 for filter gradients --
the constants of tests/test_gpu_parity.py for this function -- widened only to 1.5 x the f32 restatement's own error, which
tests/test_wq_message_cases_host.py shows never takes effect.  The worst error per instantiation goes to the parity record.

``xeq_message_fwd_wq`` / ``_bwd_wq`` without XEQ_WQ_PACKED_WEIGHTS (the kernels' own staging of W) have no caller in the tree -- both
fronts pack once per weight version -- so that path is not run here."""
import functools

import numpy as np
import pytest
import torch

from oracle import xpainn_oracle as orc
from tests import parity_record, wq_message_cases as wc
from xequinet_amd import lib
from xequinet_amd.data import synthetic as syn

pytestmark = pytest.mark.gpu

DEV = "cuda"
MAIN = wc.MUL_MAIN
FIRST_AND_MIRROR_COUNTS = (8, 20, 22, 26, 31)
WORST = {}   # (instantiated KS, "out" | "param") -> (err / bound, err, bound, tensor, case)


def _instantiation(B):
    """the KS the kernels are instantiated for at this basis count, from the count alone"""
    tail = max(B - 16, 0) + 1
    return 1 if tail <= 1 else 3 if tail <= 5 else 4 if tail <= 8 else 8


@pytest.fixture(scope="module", autouse=True)
def _parity_records():
    yield
    for (ks, what), (ratio, err, bnd, name, case) in sorted(WORST.items()):
        print(f"wq worst KS={ks} {what}: err {err:.3e} bound {bnd:.3e} ({ratio:.3f} of it) {name} {case}")
        parity_record.add({"test": f"wq:message:KS={ks}:{what}", "err": err, "bound": bnd, "err_over_bound": ratio, "output": name, "case": case})


@pytest.fixture(autouse=True)
def _wq(monkeypatch):
    monkeypatch.setenv("XEQ_MESSAGE_IMPL", "wq")
    monkeypatch.delenv("XEQ_WQ_EDGES_PER_STREAM", raising=False)
    monkeypatch.delenv("XEQ_WQ_LONG_MULT", raising=False)


def _stream_length(monkeypatch, eps):
    if eps is not None:
        monkeypatch.setenv("XEQ_WQ_EDGES_PER_STREAM", eps)


def _compare(c, got, names, tol, what="out", tag=""):
    failed = []
    for k in names:
        if c.ref[k] is None:
            assert got[k] is None, k
            continue
        g = got[k].detach().cpu().double()
        assert g.shape == c.ref[k].shape and torch.isfinite(g).all(), (c.id, k)
        err, bnd = float((g - c.ref[k]).abs().max()), wc.bound(c.ref[k], c.ref32[k], tol)
        print(f"{c.id}{tag} {k}: err {err:.3e} bound {bnd:.3e}")
        key = (_instantiation(c.B), what)
        if key not in WORST or err / bnd > WORST[key][0]:
            WORST[key] = (err / bnd, err, bnd, k, c.id + tag)
        if not err <= bnd:
            failed.append((k, err, bnd))
    assert not failed, (c.id + tag, failed)


def _dev(t):
    return None if t is None else t.float().to(DEV).contiguous()


def _cfg(c, flags=0):
    return (c.rbf_kind, c.cutoff_kind, c.B, c.cutoff, c.F, c.mul, flags)


def _graph(c, **kw):
    from xequinet_amd import ops

    return ops.EdgeGraph(torch.tensor(c.edges.edge_index, device=DEV), c.n, **kw)


def _run(c, layout=0, hint=0, node_grads=True, graph=None, param_grads=False):
    """message_forward + message_backward (+ message_param_grad) of a case -> dict of results by reference name, on the device; the
    BT layout (layout 1) is undone on dL/dxhat"""
    from xequinet_amd import ops

    graph = _graph(c) if graph is None else graph
    cfg = _cfg(c, layout | hint)
    xhat = _dev(c.xhat) if layout == 0 else _dev(wc.to_bt(c.xhat, c.mul))
    s, x, g_s, g_x = _dev(c.s), _dev(c.x), _dev(c.g_s), _dev(c.g_x)
    s_out, x_out, saved, impl = ops.message_forward(_dev(c.h), xhat, _dev(c.vec), s, x, _dev(c.W), _dev(c.b), _dev(c.p0), _dev(c.p1), graph, cfg,
                                                    want_backward=True)
    assert impl == "wq"
    g_h, g_xhat, g_vec, gs_in, gx_in = ops.message_backward(saved, graph, cfg, impl, g_s, g_x, node_grads=node_grads)
    if g_xhat is not None:
        g_xhat = g_xhat.reshape(c.n, c.D) if layout == 0 else wc.from_bt(g_xhat.reshape(-1), c.mul, c.n)
    out = dict(zip(wc.OUTPUTS, (s_out, x_out, g_h, g_xhat, g_vec, gs_in, gx_in)))
    if param_grads:
        out.update(zip(wc.PARAM_GRADS, ops.message_param_grad(saved, graph, cfg, g_s, g_x)))
    torch.cuda.synchronize()
    return out


def _check_exact(c, got):
    """What must hold to the bit: the residual rows of nodes without a walked edge, zero node gradients for nodes nobody lists, and
    zero dL/dvec on every edge at or beyond the cutoff."""
    el = c.edges
    fwd_empty, rev_empty = torch.tensor(np.diff(el.c_rowptr) == 0), torch.tensor(np.diff(el.n_rowptr) == 0)
    assert int(fwd_empty.sum()) >= 3 and bool(fwd_empty[-1]) and int(rev_empty.sum()) >= 3 and bool(rev_empty[-1])
    s_out, x_out = got["s_out"].cpu(), got["x_out"].cpu()
    assert torch.equal(s_out[fwd_empty], c.s.float()[fwd_empty]) and torch.equal(x_out[fwd_empty], c.x.float()[fwd_empty])
    assert not torch.equal(s_out[~fwd_empty], c.s.float()[~fwd_empty])
    assert float(got["grad_h"].cpu()[rev_empty].abs().max()) == 0.0 and float(got["grad_xhat"].cpu()[rev_empty].abs().max()) == 0.0
    assert int(c.beyond.sum()) >= 3 and float(got["grad_vec"].cpu()[c.beyond].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------ every case, both stream lengths
@pytest.mark.parametrize("eps", ["16", None], ids=["eps16", "epsdefault"])
@pytest.mark.parametrize("row", wc.TABLE, ids=[wc.case_id(*r) for r in wc.TABLE])
def test_every_case_of_the_table(row, eps, monkeypatch):
    """Directed list.  With 16 edges per stream the segments of 17 .. 48 edges cross stream boundaries."""
    _stream_length(monkeypatch, eps)
    c = wc.message_case(*row)
    got = _run(c)
    _compare(c, got, wc.OUTPUTS, wc.TOL_OUT, tag="" if eps is None else " eps16")
    _check_exact(c, got)


@pytest.mark.parametrize("eps", ["16", None], ids=["eps16", "epsdefault"])
@pytest.mark.parametrize("B", wc.PER_INSTANTIATION)
@pytest.mark.parametrize("kind", wc.LIST_KINDS[1:])
def test_other_list_kinds(kind, B, eps, monkeypatch):
    """Unsorted centers (a permuted forward walk), the transposed degrees on the reverse walk, the symmetric list without its
    promise (a reverse plan of its own)."""
    _stream_length(monkeypatch, eps)
    c = wc.message_case(MAIN, B, list_kind=kind)
    got = _run(c)
    _compare(c, got, wc.OUTPUTS, wc.TOL_OUT, tag="" if eps is None else " eps16")
    _check_exact(c, got)


@pytest.mark.parametrize("B", wc.PER_INSTANTIATION)
def test_bt_layout_of_xhat(B):
    c = wc.message_case(MAIN, B)
    got = _run(c, layout=1)
    _compare(c, got, wc.OUTPUTS, wc.TOL_OUT, tag=" BT")
    _check_exact(c, got)


# ------------------------------------------------------------------------------------------------------- first-block form
@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("B", FIRST_AND_MIRROR_COUNTS)
def test_first_block_form(B, layout):
    """XEQ_XHAT_HIGHER_L_ZERO on an xhat that is zero on the l > 0 columns: the forward kernel's bits are those of the unhinted kernel
    (as tests/test_gpu_parity.py::test_wq_first_block_hint_changes_nothing requires); forward and dL/dvec of the reverse kernel
    without node gradients also against the f64 reference."""
    c = wc.message_case(MAIN, B, first_block=True)
    plain = _run(c, layout=layout)
    hinted = _run(c, layout=layout, hint=lib.XHAT_HIGHER_L_ZERO, node_grads=False)
    assert hinted["grad_h"] is None and hinted["grad_xhat"] is None
    assert torch.equal(plain["s_out"], hinted["s_out"]) and torch.equal(plain["x_out"], hinted["x_out"])
    _compare(c, plain, wc.OUTPUTS, wc.TOL_OUT, tag=f" first plain layout {layout}")
    _compare(c, hinted, ("s_out", "x_out", "grad_vec"), wc.TOL_OUT, tag=f" first hinted layout {layout}")
    assert float(hinted["grad_vec"].cpu()[c.beyond].abs().max()) == 0.0
    full = _run(c, layout=layout, hint=lib.XHAT_HIGHER_L_ZERO)        # with node gradients wanted the hint does not apply to the reverse kernel
    for k in ("grad_h", "grad_xhat", "grad_vec"):
        assert torch.equal(full[k], plain[k]), k


# ------------------------------------------------------------------------------------------------------------ mirror walk
@pytest.mark.parametrize("B", FIRST_AND_MIRROR_COUNTS)
def test_mirror_walk(B):
    """Symmetric center-sorted list with the builder's promise: the reverse kernel walks the forward plan and records.  The same bits
    as the reverse-plan walk (tests/test_gpu_parity.py::test_wq_reverse_mirror_walk_is_the_reverse_plan_bit_for_bit at 20), and the
    reference's values."""
    c = wc.message_case(MAIN, B, list_kind="symmetric")
    res = {}
    for mirror in (True, False):
        graph = _graph(c, center_sorted=True, symmetric=True)
        assert graph.mirror_walk and torch.equal(graph.mirror_map.cpu(), torch.tensor(c.edges.n_perm))
        graph.mirror_walk = mirror
        res[mirror] = _run(c, layout=1, graph=graph)
        assert any(key[0] for key in graph._wq) == (not mirror)          # no reverse plan under the mirror walk
    for k in wc.OUTPUTS:
        assert torch.equal(res[True][k], res[False][k]), k
    _compare(c, res[True], wc.OUTPUTS, wc.TOL_OUT, tag=" mirror")
    _check_exact(c, res[True])


# ---------------------------------------------------------------------------------------------------------- record buffer
def test_record_floats_are_those_of_the_header():
    f = lib.load().xeq_message_wq_record_floats_for
    assert [int(f(B)) for B in range(1, 32)] == [40] * 23 + [48] * 8
    assert int(lib.load().xeq_message_wq_record_floats()) == 40


@pytest.mark.parametrize("B", [23, 24])
def test_records_on_both_sides_of_the_width_change_under_guard_bands(B):
    """The widest 40-float record and the narrowest 48-float one (written for 5 tail steps, read by the 8-step kernels), every
    allocation of the ops between guard bands, as tests/test_gpu_guard_bands.py::test_message_fwd_bwd_guarded: bands intact, no
    output element left unwritten, nothing behind a buffer reaches a result -- and the reference's values."""
    from tests.test_gpu_guard_bands import _banded
    from xequinet_amd import ops

    c = wc.message_case(MAIN, B)
    W, b, p0, cfg = _dev(c.W), _dev(c.b), _dev(c.p0), _cfg(c)
    ops.wq_packed_weights(W, b, c.B, c.F, c.mul)
    widths = []

    def run(h, xhat, vec, s, x, ei, g_s, g_x):
        graph = ops.EdgeGraph(ei, c.n)
        s_out, x_out, saved, used = ops.message_forward(h, xhat, vec, s, x, W, b, p0, None, graph, cfg, want_backward=True)
        assert used == "wq"
        g_h, g_xhat, g_vec, _, _ = ops.message_backward(saved, graph, cfg, used, g_s, g_x)
        widths.extend(int(rec.shape[1]) for plan in graph._wq.values() for rec in plan["records"][2:] if rec is not None)
        return s_out, x_out, g_h, g_xhat, g_vec

    ins = [_dev(t) for t in (c.h, c.xhat, c.vec, c.s, c.x)] + [torch.tensor(c.edges.edge_index, device=DEV), _dev(c.g_s), _dev(c.g_x)]
    out = _banded(run, ins)
    assert widths and set(widths) == {40 if B <= 23 else 48}
    got = dict(zip(("s_out", "x_out", "grad_h", "grad_xhat", "grad_vec"), out))
    _compare(c, got, tuple(got), wc.TOL_OUT, tag=" guarded")


# -------------------------------------------------------------------------------------------------------- filter gradients
def _matrix_core_form_expected(rbf_kind, B):
    """Bessel 12 .. 27 and Gaussian 8 .. 18: the counts at which the per-edge row of the filter-gradient kernel (table, derivative
    columns and harmonics) is exactly 64 columns"""
    return (rbf_kind == "bessel" and 12 <= B <= 27) or (rbf_kind == "gaussian" and 8 <= B <= 18)


@pytest.mark.parametrize("row", [r for r in wc.TABLE if r[2] in ("bessel", "gaussian")], ids=[wc.case_id(*r) for r in wc.TABLE if r[2] in ("bessel", "gaussian")])
def test_filter_gradients(row):
    """dL/dW, dL/db, dL/dp0, dL/dp1 behind the wq forward: the matrix-core form inside its admission range, the node-walk form just
    outside (the launch-name trace says which ran).  The wq kernels admit more than 256 irrep channels ((160, 96, 64) and (256, 32, 32)
    have 320), the node-walk form does not: outside the matrix-core range such a layout is refused, which is pinned here."""
    c = wc.message_case(*row)
    mc = _matrix_core_form_expected(c.rbf_kind, c.B)
    if not mc and (c.C > 256 or c.F > 256):
        # The node-walk form maps a workgroup's 256 threads to the channels and refuses more of them (csrc/xeq_message.hip, check_msg), so a
        # layout wider than that has filter gradients only where the matrix-core form is admitted: an error here, not a number.
        with pytest.raises(RuntimeError, match="exceed the 256-channel workgroup mapping"):
            _run(c, param_grads=True)
        return
    n0 = lib.launch_count()
    got = _run(c, param_grads=True)
    names = lib.launch_names(n0)
    assert names.count("xeq_message_param_grad_mc") == (1 if mc else 0) and names.count("xeq_message_param_grad") == (0 if mc else 1), names
    assert any(n.startswith("xeq_message_fwd_wq") for n in names)
    _compare(c, got, wc.PARAM_GRADS, wc.TOL_PARAM, what="param", tag=" mc" if mc else " node walk")


def test_filter_gradients_of_the_exponential_bases_are_refused():
    """expnorm / expbern have no filter-gradient kernel (the differentiable tensor form takes them): an error, not a wrong number."""
    rows = [r for r in wc.TABLE if r[2] in ("expnorm", "expbern")]
    assert rows
    with pytest.raises(RuntimeError, match="are not built"):
        _run(wc.message_case(*rows[0]), param_grads=True)


# ------------------------------------------------------------------------------------------------------------ whole model
@functools.lru_cache(maxsize=None)
def _model_and_batch(num_basis):
    from tests import test_gpu_parity as P

    model, oracle = P._build(torch.float32, num_basis=num_basis)
    pos, z, ptr = syn.synth_qm9_batch(40, seed=21)
    ei = orc.radius_graph_canonical(pos.astype(np.float32), ptr, 5.0)
    return model, oracle, pos, z, ptr, ei


@pytest.mark.parametrize("front", ["python", "native"])
@pytest.mark.parametrize("num_basis", [23, 26])
def test_whole_model(num_basis, front, monkeypatch):
    """f32 model with a basis count of the 4-step and of the zero-filled 8-step instantiation on 40 QM9-shape molecules: energies and
    forces against XPaiNNOracle in f64 under the bounds of tests/test_gpu_parity.py::_check_model, through the Python modules and
    through xeq::xpainn_eval (the same kernel sequence, written a second time in C++)."""
    from tests import test_gpu_parity as P

    model, oracle, pos, z, ptr, ei = _model_and_batch(num_basis)
    assert model.cutoff_radius == 5.0
    n0 = lib.launch_count()
    if front == "python":
        P._check_model(model, oracle, pos, z, ptr, ei, torch.float32, label=f"wq model num_basis={num_basis}")
    else:
        from xequinet_amd.interface.scripted import XPaiNNNative

        monkeypatch.delenv("XEQ_MESSAGE_IMPL")          # the operator follows the automatic selection: these sizes take wq
        batch = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
        ref_in = {"pos": torch.tensor(pos, dtype=torch.float64), "atomic_numbers": torch.tensor(z.astype(np.int64)),
                  "edge_index": torch.tensor(ei), "batch": torch.tensor(batch), "ptr": torch.tensor(ptr)}
        want = oracle(ref_in, compute_forces=True)
        out = XPaiNNNative(model)(P._t(pos, torch.float32), P._t(z.astype(np.int32)), P._t(ei), P._t(ptr), None, None, True, True, True, False)
        E, Eref = out[0].detach().cpu().double().numpy(), want["energy"].numpy()
        Fg, Fref = out[2].detach().cpu().double().numpy(), want["forces"].numpy()
        dE, dF = np.abs(E - Eref), np.abs(Fg - Fref)
        b_max, b_p99, e32_max, e32_p99 = P.f32_force_bounds(oracle, ref_in, Fref)
        print(f"native num_basis={num_basis}: max|dE| {dE.max():.3e} max|dF| {dF.max():.3e} (bound {b_max:.3e}) p99 {np.quantile(dF, 0.99):.3e} (bound {b_p99:.3e})")
        assert np.all(dE <= 1e-5 * np.abs(Eref) + 1e-4), (E - Eref)
        assert dF.max() <= b_max, (dF.max(), b_max, e32_max)
        assert np.quantile(dF, 0.99) <= b_p99, (np.quantile(dF, 0.99), b_p99, e32_p99)
    names = lib.launch_names(n0)
    assert sum(n.startswith("xeq_message_fwd_wq") for n in names) >= 3 and not any(n.startswith("xeq_message_fwd_sb") for n in names), names
