"""CPU checks of the constant-pressure dynamics (xequinet_amd/md.py ensemble "npt_berendsen", csrc/xeq_md.hip): the numpy barostat the
GPU suite compares against (tests/npt_oracle.py), the pressure unit, the new C entries' argument checks and the driver's refusals."""
import ctypes

import numpy as np
import pytest
import torch

from tests import hessian_cases as hc
from tests import md_oracle as mo
from tests import npt_oracle as no


def test_mu_is_one_at_the_target_pressure_and_without_compressibility():
    for p in (0.0, 1.0e-4, -3.7e-3, 0.62415, 17.0):
        assert no.mu_of(p, p, 0.37) == 1.0
        assert no.mu_of(p, 2.0 * p + 1.0, 0.0) == 1.0
    cell = np.array([[9.1, 0.0, 0.0], [0.7, 8.3, 0.0], [-0.4, 1.2, 10.5]])
    w = np.array([[0.3, 0.01, 0.0], [0.01, -0.2, 0.02], [0.0, 0.02, 0.5]])
    p = no.pressure(0.41, w, cell)
    assert p == (2.0 * 0.41 + ((0.3 + -0.2) + 0.5)) / (3.0 * abs(no.det(cell))) and abs(no.det(cell) - np.linalg.det(cell)) < 1e-12 * 800
    for dtype in (np.float32, np.float64):
        c = cell.astype(dtype).astype(np.float64)
        pc = no.pressure(0.41, w, c)
        at_target, stiff = no.box_back(0.41, w, c, 0.2, pc, dtype), no.box_back(0.41, w, c, 0.0, pc + 1.0, dtype)
        for b in (at_target, stiff):
            assert b["mu"] == 1.0 and not b["bad"] and np.array_equal(b["cell_next"], c)
    # above the target the box grows, below it shrinks; a scale factor that is not positive is refused and leaves the box
    assert no.box_back(0.41, w, cell, 0.2, p - 0.01, np.float64)["mu"] > 1.0 > no.box_back(0.41, w, cell, 0.2, p + 0.01, np.float64)["mu"]
    refused = no.box_back(0.41, w, cell, 1.0e6, p + 1.0, np.float64)
    assert refused["bad"] and refused["mu"] == 1.0 and np.array_equal(refused["cell_next"], cell)


def test_pressure_unit_against_hand_computed_codata():
    from xequinet_amd import md

    # 1 GPa = 1e9 J / m^3; 1 eV = 1.602176634e-19 J; 1 A^3 = 1e-30 m^3
    assert abs(no.GPA_EV_A3 / 6.241509074460763e-3 - 1.0) < 1e-15
    assert abs(md.unit_factors("eV", "Angstrom")["GPa"] / 6.241509074460763e-3 - 1.0) < 1e-12
    # 1 kcal / mol = 4184 J / N_A
    assert abs(md.unit_factors("kcal/mol", "Angstrom")["GPa"] / (1.0e9 * 1.0e-30 * 6.02214076e23 / 4184.0) - 1.0) < 1e-12
    assert abs(1.0 / no.GPA_EV_A3 - 160.21766339999998) < 1e-9                         # the familiar 1 eV / A^3 = 160.2 GPa


def test_oracle_virial_trace_is_minus_3v_de_dv():
    """tr W = -3 V dE/dV under uniform scaling of the water box: the f64 oracle's virial against central differences (five points) of
    its energy on a neighbour list rebuilt for every scaled box; 1e-6 relative, the project's finite-difference bound."""
    sd = hc.model_case("well")[1]
    h = hc.host_case("water box")
    x, z, cell = h["pos"].numpy(), h["atomic_numbers"].numpy(), h["cell"].numpy().reshape(3, 3)
    _, _, w, _ = no.evaluate(sd, x, z, cell, torch.float64)
    assert np.abs(w - w.T).max() <= 1e-12 * np.abs(w).max()
    d = 2.0e-4
    e = {k: no.energy(sd, (1.0 + k * d) * x, z, (1.0 + k * d) * cell) for k in (-2, -1, 1, 2)}
    de_ds = (8.0 * (e[1] - e[-1]) - (e[2] - e[-2])) / (12.0 * d)            # dE/ds at s = 1; V = s^3 V0: dE/dV = dE/ds / (3 V)
    want, got = -de_ds, float(np.trace(w))
    print(f"npt parity: tr W {got:.12e}, -3 V dE/dV by differences {want:.12e}, relative {abs(got - want) / abs(want):.3e}")
    assert abs(want) > 1e-3 and abs(got - want) <= 1e-6 * abs(want)


def test_host_npt_without_compressibility_is_the_berendsen_thermostat():
    sd = hc.model_case("well")[1]
    h = hc.host_case("water box")
    x, z, cell = h["pos"].numpy(), h["atomic_numbers"].numpy(), h["cell"].numpy().reshape(3, 3)
    m = mo.masses_of(z)
    v0 = 0.01 * np.random.default_rng(3).standard_normal(x.shape)
    kw = dict(dt=mo.DT_FS, n_steps=2, accel=ACCEL, kB=KB, v0=v0)
    a = mo.integrate(sd, x, z, np.array([0, len(x)]), m, ensemble="berendsen", temperature=300.0, taut=20.0, cell=cell, **kw)
    b = no.integrate(sd, x, z, m, cell, gpa=no.GPA_EV_A3, temperature=300.0, taut=20.0, pressure_GPa=0.5, taup=100.0, compressibility_per_GPa=0.0, **kw)
    for k in ("pos", "vel", "ekin", "epot"):
        assert np.array_equal(a[k][-1], b[k][-1]), k
    assert np.array_equal(b["cell"][-1], cell) and b["mu"][-1] == 1.0
    c = no.integrate(sd, x, z, m, cell, gpa=no.GPA_EV_A3, temperature=300.0, taut=20.0, pressure_GPa=b["pressure"][0] + 1.0, taup=100.0,
                     compressibility_per_GPa=0.05, **kw)
    assert c["mu"][0] < 1.0 and c["volume"][-1] < c["volume"][0] and abs(c["volume"][1] / c["volume"][0] - c["mu"][0] ** 3) < 1e-12


ACCEL, KB = 9.648533212331002e-3, 8.617333262145179e-5


def test_npt_entries_report_argument_errors_without_a_gpu():
    from xequinet_amd import lib

    L = lib.load()
    N = None
    i3 = lambda *v: (ctypes.c_int32 * 3)(*v)

    def tables(dtype=0, cell=1, out=1, reps=(1, 1, 1), pbc=(1, 1, 1), cutoff=5.0, count=6 * 27 + 12):
        # (the two non-null pointers are never followed: every check here fails before the launch)
        return L.xeq_pbc_tables_device(dtype, cell, i3(*reps), i3(*pbc), cutoff, out, count, N, N)

    assert tables(dtype=2) == 1 and b"dtype" in L.xeq_last_error()
    assert tables(cell=None) == 1 and b"null" in L.xeq_last_error()
    assert tables(out=None) == 1 and b"null" in L.xeq_last_error()
    assert tables(cutoff=0.0) == 1 and b"cutoff" in L.xeq_last_error()
    assert tables(reps=(1, -1, 1)) == 1 and b"images per axis" in L.xeq_last_error()
    assert tables(reps=(65, 0, 0), count=6 * 131 + 12) == 1 and b"images per axis" in L.xeq_last_error()
    assert tables(count=6 * 27) == 1 and b"need 174" in L.xeq_last_error()

    ref, fill = ctypes.byref, lib.fill

    def front(dtype=0, n=4, dt=0.5, r=0.1, t0=300.0, box=1, cell=1):
        return L.xeq_npt_front(ref(fill(lib.ResSystem(), dtype=dtype, n=n)), ref(fill(lib.MdParams(), dt_over_tau=r, t0=t0)),
                               ref(fill(lib.NptParams(), box=box, step_cell=cell)), dt, N)

    assert front(dtype=3) == 1 and b"dtype" in L.xeq_last_error()
    assert front(n=-1) == 1 and b"atoms" in L.xeq_last_error()
    assert front(dt=-0.1) == 1 and b"time step" in L.xeq_last_error()
    assert front(dt=float("nan")) == 1
    assert front(r=-1.0) == 1 and b"berendsen" in L.xeq_last_error()
    assert front(box=None) == 1 and b"box record" in L.xeq_last_error()
    assert front() == 1 and b"null state buffer" in L.xeq_last_error()
    assert front(n=0) == 0                                                          # nothing to do: no launch

    def back(dtype=0, n=4, c=1, half_dt=0.25, kappa=0.0, p0=0.0, unit=160.2, every=0, box=1, needed=None):
        system = fill(lib.ResSystem(), dtype=dtype, n=n, n_chunks=c, book=1)
        step = fill(lib.ResStep(), n_edges_step=1, virial_step=1, reps_needed=needed)
        return L.xeq_npt_back(ref(system), ref(step), ref(lib.ResChunks()), ref(fill(lib.MdParams(), half_dt=half_dt)),
                              ref(fill(lib.NptParams(), box=box, virial=1, kappa=kappa, p0=p0, p_unit=unit)), ref(fill(lib.ResRecorder(), every=every)), 1, N)

    assert back(dtype=-1) == 1 and b"dtype" in L.xeq_last_error()
    assert back(n=0) == 1 and b"atoms" in L.xeq_last_error()
    assert back(n=600, c=2) == 1 and b"cannot hold" in L.xeq_last_error()
    assert back(half_dt=-1.0) == 1 and b"half time step" in L.xeq_last_error()
    assert back(kappa=-1.0) == 1 and b"barostat" in L.xeq_last_error()
    assert back(p0=float("inf")) == 1 and b"barostat" in L.xeq_last_error()
    assert back(every=-2) == 1 and b"recorder" in L.xeq_last_error()
    assert back(box=None) == 1 and b"box record" in L.xeq_last_error()
    assert back(needed=1) == 1 and b"image counts" in L.xeq_last_error()
    assert back() == 1 and b"null per-atom" in L.xeq_last_error()


def _tiny():
    pos = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.1, 0.0]])
    return pos, torch.tensor([8, 1, 1]), torch.tensor([15.999, 1.008, 1.008])


def test_npt_dynamics_refusals():
    from xequinet_amd import md
    from xequinet_amd.nn import resolve_model

    pos, z, m = _tiny()
    model = resolve_model("xpainn", **hc.SMALL)
    cell = 10.0 * torch.eye(3)
    full = dict(timestep_fs=0.5, ensemble="npt_berendsen", temperature_K=300.0, taut_fs=20.0, pressure_GPa=0.1, taup_fs=100.0,
                compressibility_per_GPa=0.05)

    def without(*names, **extra):
        return dict({k: v for k, v in full.items() if k not in names}, **extra)

    with pytest.raises(ValueError, match="a cell and no ptr"):
        md.Dynamics(model, pos, z, m, **full)
    with pytest.raises(ValueError, match="a cell and no ptr"):
        md.Dynamics(model, pos, z, m, ptr=torch.tensor([0, 3]), **full)
    with pytest.raises(ValueError, match="a cell and no ptr"):
        md.Dynamics(model, pos, z, m, ptr=torch.tensor([0, 3]), cell=cell, **full)
    with pytest.raises(ValueError, match=r"all three axes periodic \(pbc is open along \[1\]\)"):
        md.Dynamics(model, pos, z, m, cell=cell, pbc=[True, False, True], **full)
    with pytest.raises(ValueError, match="taup_fs"):
        md.Dynamics(model, pos, z, m, cell=cell, **without("taup_fs"))
    with pytest.raises(ValueError, match="pressure_GPa"):
        md.Dynamics(model, pos, z, m, cell=cell, **without("pressure_GPa"))
    with pytest.raises(ValueError, match="compressibility_per_GPa"):
        md.Dynamics(model, pos, z, m, cell=cell, **without("compressibility_per_GPa"))
    with pytest.raises(ValueError, match="compressibility_per_GPa"):
        md.Dynamics(model, pos, z, m, cell=cell, **without(compressibility_per_GPa=-1.0))
    with pytest.raises(ValueError, match="taut_fs"):
        md.Dynamics(model, pos, z, m, cell=cell, **without("taut_fs"))
    with pytest.raises(ValueError, match="temperature_K"):
        md.Dynamics(model, pos, z, m, cell=cell, **without("temperature_K"))
    # the barostat's keywords belong to its ensemble; with everything in place the refusal left is the missing GPU
    with pytest.raises(ValueError, match="belong to ensemble 'npt_berendsen'"):
        md.Dynamics(model, pos, z, m, cell=cell, timestep_fs=0.5, ensemble="berendsen", temperature_K=300.0, taut_fs=20.0, taup_fs=100.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        md.Dynamics(model, pos, z, m, cell=cell, edge_capacity=64, **full)
    with pytest.raises(ValueError, match="ensemble"):
        md.Dynamics(model, pos, z, m, cell=cell, timestep_fs=0.5, ensemble="npt")


def test_step_class_keywords_are_checked_on_the_host():
    from xequinet_amd import runtime
    from xequinet_amd.nn import resolve_model

    model = resolve_model("xpainn", **hc.SMALL)
    with pytest.raises(ValueError, match="min_images"):
        runtime.GraphedStepPBC(model, 3, 64, min_images=[1, 1])
    with pytest.raises(ValueError, match="min_images"):
        runtime.GraphedStepPBC(model, 3, 64, min_images=[1, -1, 1])
    step = runtime.GraphedStepPBC(model, 3, 64, compute_virial=True, min_images=[1, 2, 3])
    assert step.compute_virial and not step.device_cell and step.min_images == [1, 2, 3] and step.reps is None
    with pytest.raises(ValueError, match="no cell was loaded"):
        step.grow_images([1, 1, 1])
