"""CPU checks of the device-resident dynamics (xequinet_amd/md.py, csrc/xeq_md.hip): the host generator and integrator the GPU suite
compares against (tests/md_oracle.py), the unit factors, the C entries' argument checks and the driver's refusals."""
import ctypes

import numpy as np
import pytest
import torch

from tests import hessian_cases as hc
from tests import md_oracle as mo


def _hex(a):
    return " ".join("%08x" % int(x) for x in a)


def test_philox_known_answers():
    assert _hex(mo.philox4x32_10([0, 0, 0, 0], [0, 0])) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    assert _hex(mo.philox4x32_10([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2)) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    assert _hex(mo.philox4x32_10([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0])) == "d16cfe09 94fdcceb 5001e420 24126ea1"


def test_counter_layout_separates_its_fields():
    from xequinet_amd import md

    base = mo.counter_of([7], 3, 0)[0]
    assert base.tolist() == [7, 0, 3, 0]
    assert mo.counter_of([7 | (5 << 32)], 3, 0)[0].tolist() == [7, 5, 3, 0]
    assert mo.counter_of([7], 2**32 + 5, 1)[0].tolist() == [7, 0, 5, 1 | (1 << 30)]
    assert mo.counter_of([7], 2**62 - 1, 0)[0].tolist() == [7, 0, 0xFFFFFFFF, 0x3FFFFFFF]
    ref = mo.words(11, 0, 3, [7])[0]
    for other in (mo.words(11, 0, 3, [8]), mo.words(11, 0, 3, [7 | (1 << 32)]), mo.words(11, 0, 4, [7]), mo.words(11, 0, 3 + 2**32, [7]),
                  mo.words(11, 1, 3, [7]), mo.words(12, 0, 3, [7]), mo.words(11 + 2**32, 0, 3, [7])):
        assert not np.array_equal(ref, other[0])
    # the default ids: index within the graph below, graph index above -- a graph's first atom has the id a lone molecule's has
    ids = md.default_rng_id([0, 3, 3, 5])
    assert ids.tolist() == [0, 1, 2, 0 | (2 << 32), 1 | (2 << 32)]
    a0, cn, gp = md.chunk_tables([0, 3, 3, 600], chunk=256)
    assert a0.tolist() == [0, 3, 259, 515] and cn.tolist() == [3, 256, 256, 85] and gp.tolist() == [0, 1, 1, 4]


def test_box_muller_moments_of_the_gpu_suites_seed():
    """The seed of tests/test_gpu_md.py's moment check, on the host generator first: |mean| <= 5 / sqrt(n), |var - 1| <= 5 sqrt(2 / n)."""
    ids = np.arange(4097, dtype=np.int64)
    z = np.concatenate([mo.normals(2024, 0, s, ids) for s in range(8)]).reshape(-1)
    n = z.size
    assert n == 4097 * 3 * 8 and np.isfinite(z).all()
    assert abs(z.mean()) <= 5.0 / np.sqrt(n) and abs(z.var() - 1.0) <= 5.0 * np.sqrt(2.0 / n)


def test_unit_factors_against_hand_computed_codata():
    from xequinet_amd import md

    f = md.unit_factors("eV", "Angstrom")
    # e N_A 1e3 (kg / (g/mol)) 1e-30 (s^2 / fs^2) / 1e-20 (m^2 / A^2); k_B / e
    assert abs(f["accel"] / 9.648533212331002e-3 - 1.0) < 1e-12
    assert abs(f["kB"] / 8.617333262145179e-5 - 1.0) < 1e-12
    g = md.unit_factors("kcal/mol", "Angstrom")
    assert abs(g["accel"] / 4.184e-4 - 1.0) < 1e-12                                   # 4184 J/mol * 1e3 * 1e-30 / 1e-20
    assert abs(g["kB"] / (1.380649e-23 * 6.02214076e23 / 4184.0) - 1.0) < 1e-12       # R in kcal / (mol K)


def _pair():
    sd = hc.model_case("well")[1]
    pos = np.array([[0.0, 0.0, 0.0], [1.1, 0.2, 0.0]])
    z = np.array([6, 8])
    return sd, pos, z, np.array([0, 2]), mo.masses_of(z)


ACCEL, KB = 9.648533212331002e-3, 8.617333262145179e-5


def test_host_nve_is_time_reversible():
    sd, pos, z, ptr, m = _pair()
    fwd = mo.integrate(sd, pos, z, ptr, m, dt=0.5, n_steps=10, accel=ACCEL, kB=KB)
    bwd = mo.integrate(sd, fwd["pos"][-1], z, ptr, m, dt=0.5, n_steps=10, accel=ACCEL, kB=KB, v0=-fwd["vel"][-1])
    disp = np.abs(fwd["pos"][-1] - pos).max()
    assert disp > 1e-3
    assert np.abs(bwd["pos"][-1] - pos).max() <= 1e-12 * disp
    assert np.abs(bwd["vel"][-1]).max() <= 1e-12 * np.abs(fwd["vel"][-1]).max()


def test_host_berendsen_at_the_target_temperature_scales_by_one():
    ke, tfac = np.array([0.0371, 1.25, 3.0e-7]), np.array([212.3, 11.7, 4000.1])
    for g in range(3):
        assert mo.berendsen_lambda(ke[g : g + 1], tfac[g : g + 1], float(ke[g] * tfac[g]), 0.37)[0] == 1.0
    assert mo.berendsen_lambda([1.0], [100.0], 300.0, 0.5)[0] == 1.1 and mo.berendsen_lambda([1.0], [100.0], 1.0, 0.5)[0] == 0.9
    assert mo.berendsen_lambda([0.0], [100.0], 300.0, 0.5)[0] == 1.0


def test_host_langevin_without_friction_is_nve_bit_for_bit():
    sd, pos, z, ptr, m = _pair()
    v0 = np.array([[0.01, -0.02, 0.005], [-0.003, 0.004, 0.01]])
    a = mo.integrate(sd, pos, z, ptr, m, dt=0.4, n_steps=4, accel=ACCEL, kB=KB, v0=v0)
    b = mo.integrate(sd, pos, z, ptr, m, dt=0.4, n_steps=4, ensemble="langevin", friction=0.0, temperature=300.0, seed=5, accel=ACCEL, kB=KB, v0=v0)
    for k in ("pos", "vel", "ekin", "epot"):
        assert np.array_equal(a[k][-1], b[k][-1]), k


def test_time_step_of_the_gpu_suite_resolves_the_stiffest_mode():
    """md_oracle.DT_FS (the GPU suite's time step) against the largest frequency of its stiffest case (the water box), from the f64 oracle Hessian."""
    host = hc.host_case("water box")
    w = mo.largest_omega(hc.reference_hessian("well", "water box").numpy(), mo.masses_of(host["atomic_numbers"].numpy()), ACCEL)
    assert 0.3 < w and w * mo.DT_FS < 0.2, w


def test_inverse_cell_matches_the_oracles():
    from xequinet_amd import lib

    L = lib.load()
    cell = np.array([[9.1, 0.0, 0.0], [0.7, 8.3, 0.0], [-0.4, 1.2, 10.5]])
    inv = (ctypes.c_double * 9)()
    assert L.xeq_md_inverse_cell(cell.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), inv) == 0
    assert np.array_equal(np.array(inv).reshape(3, 3), mo.inverse_cell(cell))
    assert np.abs(mo.inverse_cell(cell) @ cell - np.eye(3)).max() < 1e-15 * 20
    flat = (ctypes.c_double * 9)(1, 0, 0, 2, 0, 0, 0, 0, 1)
    assert L.xeq_md_inverse_cell(flat, inv) == 1 and b"singular" in L.xeq_last_error()


def test_md_entries_report_argument_errors_without_a_gpu():
    from xequinet_amd import lib

    L = lib.load()
    N = None
    assert L.xeq_md_inverse_cell(None, None) == 1 and b"null" in L.xeq_last_error()
    assert L.xeq_md_normals(2, 0, 0, 0, N, 1, N, N, N) == 1 and b"dtype" in L.xeq_last_error()
    assert L.xeq_md_normals(0, 0, 2, 0, N, 1, N, N, N) == 1 and b"purpose" in L.xeq_last_error()
    assert L.xeq_md_normals(0, 0, 0, 2**62, N, 1, N, N, N) == 1 and b"62 bits" in L.xeq_last_error()
    assert L.xeq_md_normals(0, 0, 0, 0, N, 4, N, N, N) == 1 and b"null buffer" in L.xeq_last_error()
    assert L.xeq_md_normals(0, 0, 0, 0, N, -1, N, N, N) == 1
    assert L.xeq_md_normals(0, 0, 0, 0, N, 0, N, N, N) == 0                        # nothing to do: no launch

    ref, fill = ctypes.byref, lib.fill

    def front(dtype=0, ens=0, n=4, g=1, dt=0.5, c1=1.0, noise2=0.0, r=0.0, t0=0.0, cell=None, pbc=None):
        system = fill(lib.ResSystem(), dtype=dtype, n=n, n_graphs=g, cell=cell, pbc=pbc)          # (every buffer NULL)
        return L.xeq_md_front(ref(system), ref(fill(lib.MdParams(), ensemble=ens, c1=c1, noise2=noise2, dt_over_tau=r, t0=t0)), dt, N)

    assert front(dtype=3) == 1 and b"dtype" in L.xeq_last_error()
    assert front(ens=3) == 1 and b"ensemble" in L.xeq_last_error()
    assert front(n=-1) == 1 and b"atoms" in L.xeq_last_error()
    assert front(dt=-0.1) == 1 and b"time step" in L.xeq_last_error()
    assert front(dt=float("nan")) == 1
    assert front(ens=1, c1=1.5) == 1 and b"langevin" in L.xeq_last_error()
    assert front(ens=2, r=-1.0) == 1 and b"berendsen" in L.xeq_last_error()
    assert front() == 1 and b"null state buffer" in L.xeq_last_error()
    sing = (ctypes.c_double * 9)(1, 0, 0, 1, 0, 0, 0, 0, 1)
    assert front(cell=sing, pbc=(ctypes.c_int32 * 3)(1, 1, 1)) == 1 and b"singular" in L.xeq_last_error()
    assert front(n=0) == 0

    def back(dtype=0, n=4, g=1, c=1, half_dt=0.25, every=0, start=0, rows=0):
        system = fill(lib.ResSystem(), dtype=dtype, n=n, n_graphs=g, n_chunks=c)
        return L.xeq_md_back(ref(system), ref(lib.ResStep()), ref(lib.ResChunks()), ref(fill(lib.MdParams(), half_dt=half_dt)),
                             ref(fill(lib.ResRecorder(), every=every, start=start, rows=rows)), 1, N)

    assert back(dtype=-1) == 1 and b"dtype" in L.xeq_last_error()
    assert back(g=-1) == 1 and b"graphs" in L.xeq_last_error()
    assert back(n=600, c=2) == 1 and b"cannot hold" in L.xeq_last_error()
    assert back(n=2, c=3) == 1 and b"cannot hold" in L.xeq_last_error()
    assert back(half_dt=-1.0) == 1 and b"half time step" in L.xeq_last_error()
    assert back(every=-2) == 1 and b"recorder" in L.xeq_last_error()
    assert back() == 1 and b"null" in L.xeq_last_error()
    assert L.xeq_md_back(ref(lib.ResSystem()), N, N, N, N, 1, N) == 1 and b"null argument record" in L.xeq_last_error()


def _tiny(n=3):
    pos = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.1, 0.0]])[:n]
    return pos, torch.tensor([8, 1, 1])[:n], torch.tensor([15.999, 1.008, 1.008])[:n]


def test_dynamics_has_no_cpu_fallback():
    from xequinet_amd import md
    from xequinet_amd.nn import resolve_model

    import xequinet_amd

    assert xequinet_amd.md is md
    pos, z, m = _tiny()
    model = resolve_model("xpainn", **hc.SMALL)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        md.Dynamics(model, pos, z, m, ptr=torch.tensor([0, 3]), timestep_fs=0.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        md.Dynamics(model, pos, z, m, cell=10.0 * torch.eye(3), timestep_fs=0.5, edge_capacity=64)
    with pytest.raises(ValueError, match="ensemble"):
        md.Dynamics(model, pos, z, m, ptr=torch.tensor([0, 3]), timestep_fs=0.5, ensemble="npt")
    with pytest.raises(ValueError, match="temperature_K"):
        md.Dynamics(model, pos, z, m, ptr=torch.tensor([0, 3]), timestep_fs=0.5, ensemble="langevin", friction_per_fs=0.01)
    with pytest.raises(ValueError, match="taut_fs"):
        md.Dynamics(model, pos, z, m, ptr=torch.tensor([0, 3]), timestep_fs=0.5, ensemble="berendsen", temperature_K=300.0)


@pytest.mark.parametrize("kind", ["painn", "ewald", "charge"])
@pytest.mark.parametrize("periodic", [False, True])
def test_dynamics_refuses_what_the_step_classes_refuse(kind, periodic):
    from xequinet_amd import md, runtime
    from xequinet_amd.nn import resolve_model

    model = {"painn": lambda: resolve_model("painn"),
             "ewald": lambda: resolve_model("xpainn-ewald", use_pbc=False, node_dim=32, node_irreps="32x0e + 16x1o", action_blocks=1, hidden_dim=16,
                                            ewald_blocks=1),
             "charge": lambda: resolve_model("xpainn", charge_embed=True, **hc.SMALL)}[kind]()
    pos, z, m = _tiny()
    try:
        runtime.GraphedStepPBC(model, 3, 64) if periodic else runtime.GraphedStep(model, (3, 1, 6))
        raise AssertionError("the step class took the model")
    except (ValueError, NotImplementedError) as e:
        expected = e
    kw = dict(cell=10.0 * torch.eye(3), edge_capacity=64) if periodic else dict(ptr=torch.tensor([0, 3]))
    with pytest.raises(type(expected)) as got:
        md.Dynamics(model, pos, z, m, timestep_fs=0.5, **kw)
    assert str(got.value) == str(expected)
