"""CPU checks of the device-resident FIRE minimiser (xequinet_amd/optimize.py, csrc/xeq_md.hip): the host minimiser the GPU suite compares
against (tests/fire_oracle.py) against a plain restatement of ASE's loop, its convergence on the suite's systems, the unit scaling of the
time step, the C entries' argument checks and the driver's refusals."""
import numpy as np
import pytest
import torch

from tests import fire_oracle as fo
from tests import hessian_cases as hc
from tests import md_oracle as mo

FMAX = 0.05


def _ase_fire(sd, pos, z, ptr, fmax, n_iter, dt=0.1, maxstep=0.2, dtmax=1.0, n_min=5, f_inc=1.1, f_dec=0.5, alpha_start=0.1, f_alpha=0.99):
    """ASE's optimize.FIRE.step around its run loop, for ONE system, written from the algorithm alone: ``v is None`` at the start, the
    whole system's np.vdot sums, the direct norm of dr.  -> (positions per evaluation, decisions per move, dt per move, moves done)."""
    x = np.array(pos, dtype=np.float64)
    v, a, n_pos = None, alpha_start, 0
    xs, decisions, dts = [x.copy()], [], []
    for _ in range(n_iter):
        _, f = mo.evaluate(sd, x, z, ptr, None, None, torch.float64)
        if (f**2).sum(axis=1).max() < fmax**2:
            break
        if v is None:
            v = np.zeros_like(x)
            decisions.append("start")
        else:
            vf = np.vdot(f, v)
            if vf > 0.0:
                v = (1.0 - a) * v + a * f / np.sqrt(np.vdot(f, f)) * np.sqrt(np.vdot(v, v))
                if n_pos > n_min:
                    dt = min(dt * f_inc, dtmax)
                    a *= f_alpha
                n_pos += 1
                decisions.append("up")
            else:
                v[:] *= 0.0
                a = alpha_start
                dt *= f_dec
                n_pos = 0
                decisions.append("down")
        v += dt * f
        dr = dt * v
        normdr = np.sqrt(np.vdot(dr, dr))
        if normdr > maxstep:
            dr = maxstep * dr / normdr
        x = x + dr
        xs.append(x.copy())
        dts.append(dt)
    return xs, decisions, dts


def test_host_minimiser_is_ases_loop_for_one_graph():
    p, z, ptr, _ = fo.case("qm9 seed 9")
    a, b = int(ptr[0]), int(ptr[1])
    p, z, ptr = p[a:b], z[a:b], np.array([0, b - a])
    sd = hc.model_case("well")[1]
    n_iter = 40
    xs, decisions, dts = _ase_fire(sd, p, z, ptr, FMAX, n_iter)
    got = fo.minimize(sd, p, z, ptr, fmax=FMAX, n_iter=n_iter)
    assert len(xs) == n_iter + 1 and "down" in decisions and "up" in decisions and max(dts) > 0.1        # the run met every branch and a grown dt
    mine = []
    for it in range(n_iter):
        was, s = got["was"][it][0], got["P"][it][0]
        mine.append("start" if was == fo.FRESH else "up" if s > 0.0 else "down")
        assert got["dt"][it][0] == dts[it], it                                                            # exactly: the same products
    assert mine == decisions
    scale = np.abs(xs[-1]).max()
    for it in range(n_iter + 1):
        assert np.abs(got["pos"][it] - xs[it]).max() <= 1e-12 * scale, it
    assert np.abs(xs[-1] - xs[0]).max() > 0.05


@pytest.mark.parametrize("name,want", [("ragged", [127, 0, 0, 12]), ("qm9 seed 9", [93, 79]), ("water box", [106])])
def test_host_minimiser_converges_with_the_defaults(name, want):
    r = fo.host_run(name, np.float64, 200, FMAX, stop=True)
    assert r["converged_at"].tolist() == want
    assert np.all(r["state"]["status"] == fo.CONVERGED) and np.all(r["fmax"][-1] < FMAX)
    assert np.all(r["epot"][-1] <= r["epot"][0])
    # a converged graph is frozen: the lone atom and the far pair of "ragged" never move, the bonded pair not behind evaluation 12
    if name == "ragged":
        ptr = fo.case(name)[2]
        assert np.array_equal(r["pos"][-1][ptr[1]:ptr[3]], r["pos"][0][ptr[1]:ptr[3]])
        assert np.array_equal(r["pos"][-1][ptr[3]:], r["pos"][12][ptr[3]:]) and not np.array_equal(r["pos"][12][ptr[3]:], r["pos"][0][ptr[3]:])


def test_oracle_kernels_leave_fixed_atoms_and_converged_graphs_alone():
    rng = np.random.default_rng(3)
    ptr = np.array([0, 4, 4, 9, 10])
    n, G = 10, 4
    st = fo.new_state(G, 0.1, 0.1)
    st["status"][:] = [fo.ACTIVE, fo.ACTIVE, fo.CONVERGED, fo.FRESH]
    x, v, f = rng.standard_normal((n, 3)), 0.1 * rng.standard_normal((n, 3)), rng.standard_normal((n, 3))
    fixed = np.zeros(n, bool)
    fixed[1] = True
    v[1] = 0.0
    f[9] = 0.0                                                      # the lone atom: ff = 0
    new, frc, s = fo.back(st, v, f, np.full((n, 3), 7.0), np.arange(4.0), fixed, ptr, 5, fmax_tol=FMAX, **fo.DEFAULTS)
    assert new["status"].tolist() == [fo.ACTIVE, fo.CONVERGED, fo.CONVERGED, fo.CONVERGED] and new["converged_at"].tolist() == [-1, 5, -1, 5]
    assert np.array_equal(frc[4:9], np.full((5, 3), 7.0)) and np.array_equal(frc[1], np.zeros(3)) and np.array_equal(frc[0], f[0])
    assert abs(s["ff"][0] - (f[[0, 2, 3]] ** 2).sum()) < 1e-13                                            # the fixed atom's force is in no sum
    x2, v2, _ = fo.front(new, x, v, frc, None, fixed, ptr)
    assert np.array_equal(x2[4:], x[4:]) and np.array_equal(v2[4:], v[4:]) and np.array_equal(x2[1], x[1]) and np.array_equal(v2[1], v[1])
    assert not np.array_equal(x2[0], x[0])
    cv, cf, d = new["coef"][0]
    assert np.array_equal(v2[0], cv * v[0] + cf * f[0]) and np.array_equal(x2[0], x[0] + d * (cv * v[0] + cf * f[0]))
    # the clamp: |d v'| of the graph is maxstep when dt |v'| is larger, from the three sums alone
    big, _, _ = fo.back(st, v, 100.0 * f, np.zeros((n, 3)), np.zeros(4), fixed, ptr, 0, fmax_tol=FMAX, **fo.DEFAULTS)
    cv, cf, d = big["coef"][0]
    vn = cv * np.where(fixed[:4, None], 0, v[:4]) + cf * np.where(fixed[:4, None], 0, 100.0 * f[:4])
    assert abs(np.sqrt(((d * vn) ** 2).sum()) - 0.2) < 1e-13


def test_time_step_scaling_with_the_units():
    from xequinet_amd import optimize

    assert optimize.time_step_factor("eV", "Angstrom") == 1.0
    ev_per_kcalmol = 4184.0 / (6.02214076e23 * 1.602176634e-19)
    assert abs(optimize.time_step_factor("kcal/mol", "Angstrom") / np.sqrt(ev_per_kcalmol) - 1.0) < 1e-9
    bohr = 0.529177210903                                            # Angstrom (CODATA 2018)
    hartree = 27.211386245988                                        # eV
    assert abs(optimize.time_step_factor("Hartree", "Bohr") / np.sqrt(hartree / bohr**2) - 1.0) < 1e-6
    # the reason for the factor: a fresh move x += dt^2 f is the same length in either unit system
    k = optimize.time_step_factor("kcal/mol", "Angstrom")
    f_ev = 0.37
    assert abs((0.1 * k) ** 2 * (f_ev / ev_per_kcalmol) - 0.1**2 * f_ev) < 1e-12


def test_fire_entries_exist_with_their_signatures():
    from xequinet_amd import lib

    L = lib.load()
    assert "xeq_fire_front" in lib.EXPORTS and "xeq_fire_back" in lib.EXPORTS
    # (the records these take, member for member against include/xeq.h: tests/test_resident_records_host.py)
    assert L.xeq_fire_front.argtypes == lib._PROTOS["xeq_fire_front"] and L.xeq_fire_back.argtypes == lib._PROTOS["xeq_fire_back"]
    assert (lib.FIRE_FRESH, lib.FIRE_ACTIVE, lib.FIRE_CONVERGED) == (fo.FRESH, fo.ACTIVE, fo.CONVERGED)


def test_fire_entries_report_argument_errors_without_a_gpu():
    import ctypes

    from xequinet_amd import lib

    L = lib.load()
    N = None

    ref, fill = ctypes.byref, lib.fill

    def front(dtype=0, n=4, g=1, cell=None, pbc=None):
        return L.xeq_fire_front(ref(fill(lib.ResSystem(), dtype=dtype, n=n, n_graphs=g, cell=cell, pbc=pbc)), ref(lib.FireParams()), N)

    assert front(dtype=2) == 1 and b"dtype" in L.xeq_last_error()
    assert front(n=-1) == 1 and b"atoms" in L.xeq_last_error()
    assert front(g=0) == 1 and b"no graph" in L.xeq_last_error()
    assert front() == 1 and b"null state buffer" in L.xeq_last_error()
    sing = (ctypes.c_double * 9)(1, 0, 0, 1, 0, 0, 0, 0, 1)
    assert front(cell=sing, pbc=(ctypes.c_int32 * 3)(1, 1, 1)) == 1 and b"singular" in L.xeq_last_error()
    assert front(n=0) == 0                                          # nothing to do: no launch

    def back(dtype=0, n=4, g=1, c=1, fmax=0.05, maxstep=0.2, dtmax=1.0, n_min=5, f_inc=1.1, f_dec=0.5, a0=0.1, fa=0.99, every=0):
        fire = fill(lib.FireParams(), fmax_tol=fmax, maxstep=maxstep, dtmax=dtmax, n_min=n_min, f_inc=f_inc, f_dec=f_dec, alpha_start=a0, f_alpha=fa)
        return L.xeq_fire_back(ref(fill(lib.ResSystem(), dtype=dtype, n=n, n_graphs=g, n_chunks=c)), ref(lib.ResStep()), ref(lib.ResChunks()), ref(fire),
                               ref(fill(lib.ResRecorder(), every=every)), N)

    assert back(dtype=-1) == 1 and b"dtype" in L.xeq_last_error()
    assert back(g=-1) == 1 and b"graphs" in L.xeq_last_error()
    assert back(g=0) == 1 and b"no graph" in L.xeq_last_error()
    assert back(n=600, c=2) == 1 and b"cannot hold" in L.xeq_last_error()
    assert back(n=2, c=3) == 1 and b"cannot hold" in L.xeq_last_error()
    assert back(fmax=0.0) == 1 and b"fmax" in L.xeq_last_error()
    assert back(fmax=float("nan")) == 1
    assert back(maxstep=-1.0) == 1 and b"maxstep" in L.xeq_last_error()
    assert back(dtmax=0.0) == 1 and b"dtmax" in L.xeq_last_error()
    assert back(f_inc=0.9) == 1 and b"mixing" in L.xeq_last_error()
    assert back(f_dec=1.0) == 1 and b"mixing" in L.xeq_last_error()
    assert back(every=-2) == 1 and b"recorder" in L.xeq_last_error()
    assert back() == 1 and b"null" in L.xeq_last_error()


def _tiny(n=3):
    pos = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.1, 0.0]])[:n]
    return pos, torch.tensor([8, 1, 1])[:n]


def test_fire_has_no_cpu_fallback_and_refuses_bad_arguments():
    import xequinet_amd
    from xequinet_amd import optimize
    from xequinet_amd.nn import resolve_model

    assert xequinet_amd.optimize is optimize
    pos, z = _tiny()
    model = resolve_model("xpainn", **hc.SMALL)
    open_ = dict(ptr=torch.tensor([0, 3]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        optimize.FIRE(model, pos, z, fmax=0.05, **open_)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        optimize.FIRE(model, pos, z, cell=10.0 * torch.eye(3), edge_capacity=64, fmax=0.05)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        optimize.minimize(model, {"pos": pos, "atomic_numbers": z, "ptr": torch.tensor([0, 3])}, 0.05)
    for name, value in (("fmax", 0.0), ("fmax", -1.0), ("fmax", float("nan")), ("dt", 0.0), ("dtmax", -1.0), ("maxstep", 0.0), ("f_dec", 0.0),
                        ("f_dec", 1.0), ("f_inc", 0.99)):
        with pytest.raises(ValueError, match="FIRE: " + name + " "):
            optimize.FIRE(model, pos, z, **open_, **dict({"fmax": 0.05}, **{name: value}))
    with pytest.raises(ValueError, match="ONE graph"):
        optimize.FIRE(model, pos, z, ptr=torch.tensor([0, 1, 3]), cell=10.0 * torch.eye(3), fmax=0.05)
    with pytest.raises(ValueError, match="fixed"):
        optimize.FIRE(model, pos, z, fixed=torch.zeros(4, dtype=torch.bool), fmax=0.05, **open_)
    with pytest.raises(ValueError, match="ptr must rise"):
        optimize.FIRE(model, pos, z, ptr=torch.tensor([0, 2]), fmax=0.05)


@pytest.mark.parametrize("kind", ["painn", "ewald", "charge"])
@pytest.mark.parametrize("periodic", [False, True])
def test_fire_refuses_what_the_step_classes_refuse(kind, periodic):
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
        optimize.FIRE(model, pos, z, fmax=0.05, **kw)
    assert str(got.value) == str(expected)
