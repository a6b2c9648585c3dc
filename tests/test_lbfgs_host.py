"""CPU checks of the device-resident L-BFGS minimiser (xequinet_amd/optimize.py: LBFGS, csrc/xeq_lbfgs.hip): the oracle the GPU suite
compares against (tests/lbfgs_oracle.py) against the plain vector two-loop recursion of ASE's optimize.LBFGS, its ring and its rejected
pairs, the C entries' argument checks and the driver's refusals."""
import ctypes

import numpy as np
import pytest
import torch

from tests import hessian_cases as hc
from tests import lbfgs_oracle as lo


def _ase_direction(s, y, g, alpha):
    """ASE's LBFGS.step, written from the algorithm alone: pairs from oldest to newest, H0 = 1 / alpha; -> the step direction p = -z."""
    rho = [1.0 / np.vdot(yi, si) for si, yi in zip(s, y)]
    q = g.copy()
    a = [0.0] * len(s)
    for i in range(len(s) - 1, -1, -1):
        a[i] = rho[i] * np.vdot(s[i], q)
        q = q - a[i] * y[i]
    z = q / alpha
    for i in range(len(s)):
        b = rho[i] * np.vdot(y[i], z)
        z = z + s[i] * (a[i] - b)
    return -z


def _quadratic(dim=30, seed=5):
    """A random SPD matrix M M^T / dim + 1 (condition number about 4), its eigenvalues and a start.  Without a line search the rule has
    no finite termination on a quadratic: the unit steps converge superlinearly at a rate set by the condition number.  This matrix
    reaches |g| < 1e-8 |g_0| at about iteration 22 of 31; one with eigenvalues spread over 1 .. 40 reaches 4e-5 in 31 (the plain vector
    form of ASE does the same, so that is the rule's, not the coefficient form's)."""
    rng = np.random.default_rng(seed)
    m = rng.standard_normal((dim, dim))
    A = m @ m.T / dim + np.eye(dim)
    return A, np.linalg.eigvalsh(A), rng.standard_normal(dim)


def _run_quadratic(A, x, memory, alpha, n_iter, reference=None):
    """The oracle's back / front on f = -A x for one graph of dim / 3 atoms without a step clamp; ``reference``: called with the
    history in age order, g and the oracle's direction."""
    n = len(x) // 3
    ptr = np.array([0, n])
    st = lo.new_state(n, 1, memory)
    par = dict(memory=memory, alpha=alpha, maxstep=1e30, damping=1.0)
    frc = np.zeros((n, 3))
    x = x.reshape(n, 3).copy()
    norms = []
    for it in range(n_iter + 1):
        f = -(A @ x.reshape(-1)).reshape(n, 3)
        st, frc, _ = lo.back(st, f, frc, [0.0], None, ptr, it, fmax_tol=1e-300, **par)
        norms.append(np.sqrt((f**2).sum()))
        x_new, st["pending"], _, _ = lo.front(st, x, frc, None, None, ptr, **par)
        if reference is not None:
            order = lo.ring_order(int(st["count"][0]), int(st["head"][0]), memory)
            reference([st["hist_s"][j].reshape(-1) for j in order], [st["hist_y"][j].reshape(-1) for j in order], -frc.reshape(-1),
                      (x_new - x).reshape(-1))
        x = x_new
    return norms, st


@pytest.mark.parametrize("memory", [1, 3, 16])
def test_coefficient_space_direction_is_the_vector_two_loop(memory):
    A, w, x0 = _quadratic()
    seen = []

    def check(s, y, g, p):
        want = _ase_direction(s, y, g, w[-1])
        assert np.abs(p - want).max() <= 1e-10 * np.abs(want).max()
        seen.append(len(s))

    _run_quadratic(A, x0, memory, w[-1], 12, check)
    assert max(seen) == min(memory, 12) and seen[0] == 0          # from the fresh move to a full ring


def test_quadratic_converges_with_the_full_history():
    A, w, x0 = _quadratic()
    norms, st = _run_quadratic(A, x0, 32, w[-1], 31)
    assert min(norms) < 1e-8 * norms[0]
    assert st["dropped"][0] == 0


def test_ring_that_wraps_twice_keeps_the_newest_pairs_in_age_order():
    memory, n = 3, 4
    rng = np.random.default_rng(2)
    A = np.diag(np.linspace(1.0, 3.0, 3 * n))
    ptr = np.array([0, n])
    st = lo.new_state(n, 1, memory)
    st["status"][0] = lo.ACTIVE
    frc = rng.standard_normal((n, 3))
    fed = []
    for it in range(1, 2 * memory + 3):
        s = 0.1 * rng.standard_normal((n, 3))
        st["pending"] = s
        f_new = frc - (A @ s.reshape(-1)).reshape(n, 3)                # y = f_prev - f = A s: accepted
        fed.append(s)
        st, frc, info = lo.back(st, f_new, frc, [0.0], None, ptr, it, fmax_tol=1e-300, memory=memory, alpha=70.0)
        assert info["accepted"][0] is True
        order = lo.ring_order(int(st["count"][0]), int(st["head"][0]), memory)
        assert len(order) == min(it, memory)
        for age, slot in enumerate(order):
            assert np.array_equal(st["hist_s"][slot], fed[len(fed) - len(order) + age])
            assert np.abs(st["hist_y"][slot] - (A @ st["hist_s"][slot].reshape(-1)).reshape(n, 3)).max() < 1e-14
    assert st["head"][0] == (2 * memory + 2) % memory and st["count"][0] == memory and st["dropped"][0] == 0


def test_rejected_pair_is_dropped_and_counted():
    memory, n = 4, 3
    rng = np.random.default_rng(4)
    ptr = np.array([0, n])
    st = lo.new_state(n, 1, memory)
    st["status"][0] = lo.ACTIVE
    frc = rng.standard_normal((n, 3))
    s = 0.1 * rng.standard_normal((n, 3))
    st["pending"] = s
    st1, frc1, info = lo.back(st, frc - 2.0 * s, frc, [0.0], None, ptr, 1, fmax_tol=1e-300, memory=memory, alpha=70.0)
    assert info["accepted"][0] is True and st1["count"][0] == 1 and st1["dropped"][0] == 0
    st1["pending"] = s
    st2, frc2, info = lo.back(st1, frc1 + 2.0 * s, frc1, [0.0], None, ptr, 2, fmax_tol=1e-300, memory=memory, alpha=70.0)      # y = -2 s
    assert info["accepted"][0] is False and info["sy"][0] < 0.0
    assert st2["count"][0] == 1 and st2["head"][0] == 1 and st2["dropped"][0] == 1
    assert np.array_equal(st2["hist_s"], st1["hist_s"]) and np.array_equal(st2["hist_y"], st1["hist_y"])
    st2["pending"] = np.zeros((n, 3))                                                                                        # s.y = 0
    st3, _, info = lo.back(st2, frc2 + 0.5, frc2, [0.0], None, ptr, 3, fmax_tol=1e-300, memory=memory, alpha=70.0)
    assert info["accepted"][0] is False and st3["dropped"][0] == 2 and st3["status"][0] == lo.ACTIVE
    # the direction still uses the pair that was kept
    assert st3["delta"][0, 0] != 0.0 and st3["delta"][0, 1] == 0.0


def test_fixed_atoms_and_converged_graphs_are_left_alone():
    memory = 2
    rng = np.random.default_rng(3)
    ptr = np.array([0, 4, 4, 9, 10])
    n, G = 10, 4
    st = lo.new_state(n, G, memory)
    st["status"][:] = [lo.ACTIVE, lo.ACTIVE, lo.CONVERGED, lo.FRESH]
    st["pending"] = 0.1 * rng.standard_normal((n, 3))
    x, f = rng.standard_normal((n, 3)), rng.standard_normal((n, 3))
    fixed = np.zeros(n, bool)
    fixed[1] = True
    f[1] = 40.0
    f[9] = 0.0
    new, frc, _ = lo.back(st, f, np.full((n, 3), 7.0), np.arange(4.0), fixed, ptr, 5, fmax_tol=0.05, memory=memory, alpha=70.0)
    assert new["status"].tolist() == [lo.ACTIVE, lo.CONVERGED, lo.CONVERGED, lo.CONVERGED] and new["converged_at"].tolist() == [-1, 5, -1, 5]
    assert np.array_equal(frc[4:9], np.full((5, 3), 7.0)) and np.array_equal(frc[1], np.zeros(3)) and np.array_equal(frc[0], f[0])
    assert abs(new["gram"][0, 2 * memory, 2 * memory] - (f[[0, 2, 3]] ** 2).sum()) < 1e-13                # the fixed atom's force is in no sum
    assert new["fmax"][0] < 40.0
    x2, pend, _, _ = lo.front(new, x, frc, None, fixed, ptr, maxstep=0.2, damping=1.0, memory=memory)
    assert np.array_equal(x2[4:], x[4:]) and np.array_equal(x2[1], x[1]) and not np.array_equal(x2[0], x[0])
    assert np.array_equal(pend[0], x2[0] - x[0]) and np.array_equal(pend[4:], new["pending"][4:])
    assert np.sqrt(((x2 - x) ** 2).sum(axis=1).max()) <= 0.2 * (1 + 1e-12)


def test_curvature_scaling_with_the_units():
    from xequinet_amd import optimize

    assert optimize.curvature_factor("eV", "Angstrom") == 1.0
    bohr, hartree = 0.529177210903, 27.211386245988
    assert abs(optimize.curvature_factor("Hartree", "Bohr") / (bohr**2 / hartree) - 1.0) < 1e-6
    # the reason for the factor: a fresh move f / alpha is the same length in either unit system
    f_ev = 0.37
    k = optimize.curvature_factor("Hartree", "Bohr")
    assert abs((f_ev / hartree * bohr) / (70.0 * k) * bohr - f_ev / 70.0) < 1e-9


def test_entries_exist_with_their_signatures():
    from xequinet_amd import lib

    L = lib.load()
    assert "xeq_lbfgs_front" in lib.EXPORTS and "xeq_lbfgs_back" in lib.EXPORTS
    assert L.xeq_lbfgs_front.argtypes == lib._PROTOS["xeq_lbfgs_front"] and L.xeq_lbfgs_back.argtypes == lib._PROTOS["xeq_lbfgs_back"]
    assert (lib.LBFGS_FRESH, lib.LBFGS_ACTIVE, lib.LBFGS_CONVERGED) == (lo.FRESH, lo.ACTIVE, lo.CONVERGED)
    header = open(__file__.replace("tests/test_lbfgs_host.py", "include/xeq.h")).read()
    assert f"#define XEQ_LBFGS_MAX_MEMORY {lib.LBFGS_MAX_MEMORY}\n" in header
    assert "enum { XEQ_LBFGS_FRESH = 0, XEQ_LBFGS_ACTIVE = 1, XEQ_LBFGS_CONVERGED = 2 };" in header
    from xequinet_amd.csrc import build

    assert "xeq_lbfgs.hip" in build.SOURCES and "xeq_lbfgs.hip" not in build.MFMA_SOURCES
    assert "-ffp-contract=off" in build.EXTRA_FLAGS["xeq_lbfgs.hip"]          # the double expressions are the ones written


def test_entries_report_argument_errors_without_a_gpu():
    from xequinet_amd import lib

    L = lib.load()
    ref, fill = ctypes.byref, lib.fill
    one = 8                                                          # a pointer that is not NULL and is never followed
    first = lib.launch_count()

    def system(dtype=0, n=4, g=1, c=1, cell=None, pbc=None):
        return ref(fill(lib.ResSystem(), dtype=dtype, n=n, n_graphs=g, n_chunks=c, cell=cell, pbc=pbc))

    def params(buf, **members):
        """The parameter record with every buffer but ``fixed`` at ``buf``."""
        state = "hist_s hist_y pending_s gram delta count head status dropped converged_at epot fmax ticket"
        return ref(fill(lib.LbfgsParams(), **dict.fromkeys(state.split(), buf), **members))

    def front(memory=4, most=1, maxstep=0.2, damping=1.0, sys=None, chunks=True, buf=None, record=True):
        rec = params(buf, memory=memory, max_graph_chunks=most, maxstep=maxstep, damping=damping) if record else None
        return L.xeq_lbfgs_front(sys or system(), ref(lib.ResChunks()) if chunks else None, rec, None)

    assert front(sys=system(dtype=2)) == 1 and b"dtype" in L.xeq_last_error()
    assert front(sys=system(n=-1)) == 1 and b"atoms" in L.xeq_last_error()
    assert front(sys=system(g=-1)) == 1 and b"graphs" in L.xeq_last_error()
    assert front(sys=system(g=0)) == 1 and b"no graph" in L.xeq_last_error()
    assert front(sys=system(n=600, c=2)) == 1 and b"cannot hold" in L.xeq_last_error()
    assert front(memory=0) == 1 and b"memory 0" in L.xeq_last_error()
    assert front(memory=33) == 1 and b"memory 33" in L.xeq_last_error()
    assert front(most=-1) == 1 and b"chunks in a graph" in L.xeq_last_error()
    assert front(maxstep=0.0) == 1 and b"maxstep" in L.xeq_last_error()
    assert front(maxstep=float("nan")) == 1
    assert front(damping=-1.0) == 1 and b"damping" in L.xeq_last_error()
    assert front() == 1 and b"null state buffer" in L.xeq_last_error()
    assert front(chunks=False) == 1 and b"null argument record" in L.xeq_last_error()
    assert front(record=False) == 1 and b"null argument record" in L.xeq_last_error()
    assert L.xeq_lbfgs_front(None, ref(lib.ResChunks()), params(None, memory=4, max_graph_chunks=1, maxstep=0.2, damping=1.0), None) == 1
    assert b"record" in L.xeq_last_error()
    sing = (ctypes.c_double * 9)(1, 0, 0, 1, 0, 0, 0, 0, 1)
    assert front(sys=system(cell=sing, pbc=(ctypes.c_int32 * 3)(1, 1, 1))) == 1 and b"singular" in L.xeq_last_error()
    assert front(sys=system(n=0, c=0), most=0) == 0                                          # nothing to do: no launch

    def back(memory=4, most=1, fmax=0.05, alpha=70.0, sys=None, step=True, every=0, buf=None, record=True):
        rec = params(buf, memory=memory, max_graph_chunks=most, fmax_tol=fmax, alpha=alpha) if record else None
        return L.xeq_lbfgs_back(sys or system(), ref(lib.ResStep()) if step else None, ref(lib.ResChunks()), rec,
                                ref(fill(lib.ResRecorder(), every=every)), None)

    assert back(sys=system(dtype=-1)) == 1 and b"dtype" in L.xeq_last_error()
    assert back(sys=system(g=-1)) == 1 and b"graphs" in L.xeq_last_error()
    assert back(sys=system(n=2, c=3)) == 1 and b"cannot hold" in L.xeq_last_error()
    assert back(memory=0) == 1 and b"memory 0" in L.xeq_last_error()
    assert back(memory=33) == 1 and b"XEQ_LBFGS_MAX_MEMORY" in L.xeq_last_error()
    assert back(fmax=0.0) == 1 and b"fmax" in L.xeq_last_error()
    assert back(fmax=float("inf")) == 1
    assert back(alpha=0.0) == 1 and b"alpha" in L.xeq_last_error()
    assert back(alpha=-70.0) == 1 and b"alpha" in L.xeq_last_error()
    assert back(every=-2) == 1 and b"recorder" in L.xeq_last_error()
    assert back(step=False) == 1 and b"null argument record" in L.xeq_last_error()
    assert back(record=False) == 1 and b"null argument record" in L.xeq_last_error()
    assert back() == 1 and b"null" in L.xeq_last_error()
    assert back(buf=one, sys=ref(fill(lib.ResSystem(), n=4, n_graphs=1, n_chunks=1, book=one))) == 1 and b"null" in L.xeq_last_error()      # the records' buffers
    assert lib.launch_count() == first


def _tiny(n=3):
    pos = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.1, 0.0]])[:n]
    return pos, torch.tensor([8, 1, 1])[:n]


def test_lbfgs_has_no_cpu_fallback_and_refuses_bad_arguments():
    from xequinet_amd import optimize
    from xequinet_amd.nn import resolve_model

    pos, z = _tiny()
    model = resolve_model("xpainn", **hc.SMALL)
    open_ = dict(ptr=torch.tensor([0, 3]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        optimize.LBFGS(model, pos, z, fmax=0.05, **open_)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        optimize.LBFGS(model, pos, z, cell=10.0 * torch.eye(3), edge_capacity=64, fmax=0.05)
    data = {"pos": pos, "atomic_numbers": z, "ptr": torch.tensor([0, 3])}
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        optimize.minimize(model, data, 0.05, method="lbfgs")
    with pytest.raises(ValueError, match="method 'nope'"):
        optimize.minimize(model, data, 0.05, method="nope")
    for name, value in (("fmax", 0.0), ("fmax", -1.0), ("fmax", float("nan")), ("alpha", 0.0), ("alpha", -70.0), ("maxstep", 0.0),
                        ("damping", 0.0), ("memory", 0), ("memory", 33), ("memory", 2.5)):
        with pytest.raises(ValueError, match="LBFGS: " + name + " "):
            optimize.LBFGS(model, pos, z, **open_, **dict({"fmax": 0.05}, **{name: value}))
    with pytest.raises(ValueError, match="ONE graph"):
        optimize.LBFGS(model, pos, z, ptr=torch.tensor([0, 1, 3]), cell=10.0 * torch.eye(3), fmax=0.05)
    with pytest.raises(ValueError, match="fixed"):
        optimize.LBFGS(model, pos, z, fixed=torch.zeros(4, dtype=torch.bool), fmax=0.05, **open_)
    with pytest.raises(ValueError, match="ptr must rise"):
        optimize.LBFGS(model, pos, z, ptr=torch.tensor([0, 2]), fmax=0.05)


@pytest.mark.parametrize("kind", ["painn", "ewald", "charge"])
@pytest.mark.parametrize("periodic", [False, True])
def test_lbfgs_refuses_what_the_step_classes_refuse(kind, periodic):
    from xequinet_amd import optimize, runtime
    from xequinet_amd.nn import resolve_model

    model = {"painn": lambda: resolve_model("painn"),
             "ewald": lambda: resolve_model("xpainn-ewald", use_pbc=False, node_dim=32, node_irreps="32x0e + 16x1o", action_blocks=1, hidden_dim=16,
                                            ewald_blocks=1),
             "charge": lambda: resolve_model("xpainn", charge_embed=True, **hc.SMALL)}[kind]()
    pos, z = _tiny()
    try:
        runtime.GraphedStepPBC(model, 3, 64) if periodic else runtime.GraphedStep(model, (3, 1, 6))
        raise AssertionError("the step class took the model")
    except (ValueError, NotImplementedError) as e:
        expected = e
    kw = dict(cell=10.0 * torch.eye(3), edge_capacity=64) if periodic else dict(ptr=torch.tensor([0, 3]))
    with pytest.raises(type(expected)) as got:
        optimize.LBFGS(model, pos, z, fmax=0.05, **kw)
    assert str(got.value) == str(expected)


@pytest.mark.parametrize("name", ["ragged", "qm9 seed 9", "water box"])
def test_host_minimiser_decisions_are_clear_of_their_thresholds(name):
    """What tests/test_gpu_lbfgs.py rests its comparison of decisions on, for the 12 iterations it compares (memory 4: the ring wraps)."""
    r = lo.host_run(name, np.float64, 12, 0.05, memory=4)
    offered = 0
    for it in range(13):
        for g, acc in enumerate(r["accepted"][it]):
            if acc is not None:
                offered += 1
                assert (r["cos"][it][g] > 1e-6) if acc else (r["cos"][it][g] < -1e-6), (it, g)
            if r["longest"][it][g] is not None:
                assert abs(r["longest"][it][g] / 0.2 - 1.0) > 1e-6, (it, g)
            if r["status"][it][g] != lo.CONVERGED:
                assert abs(r["fmax"][it][g] / 0.05 - 1.0) > 1e-6, (it, g)
    assert offered > 0 and r["count"][-1].max() == 4                     # 12 pairs offered to a ring of 4: it wrapped
