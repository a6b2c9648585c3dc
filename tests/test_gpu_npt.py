"""Constant-pressure dynamics on the device (xequinet_amd/md.py ensemble "npt_berendsen", csrc/xeq_md.hip: xeq_npt_front / xeq_npt_back,
xeq_pbc_tables_device; runtime.GraphedStepPBC(compute_virial, device_cell, min_images)) on the MI355X against the numpy barostat of
tests/npt_oracle.py.  System: the 24-atom water box of tests/hessian_cases.py, model hessian_cases.model_case("well"), time step
md_oracle.DT_FS, 6 steps.  Barostat of the trajectory tests: taup 100 fs, compressibility 0.75 / GPa, target 1 GPa above the start's own
pressure: kappa (P0 - P) = (0.4 / 100) (0.75 / 3) x 1 = 1e-3 -- the box moves by about 0.1 % per step.

Bounds: f64 trajectories 1e-9 of the largest magnitude (the MD suite's); f32 trajectories by the MD suite's rule -- device error <=
4 x max(the f32 host integrator's own error, eps32 x largest magnitude); kernels alone by the ulp rule of test_gpu_md.py's
test_front_kernel_alone (f32: 2 ulp of the f64 evaluation rounded to f32; f64: 1e-14 relative), the box record (double arithmetic in
the oracle's operation order on the SAME stored inputs) 1e-14 relative.

Measured on the MI355X: the box moves 0.093 % per step (mu of the start 0.999000).  f32 trajectories, ratio = (device error) / max(f32
host integrator's own error, eps32 x largest magnitude): pos 1.26, vel 1.26, epot 0.62, ekin 0.92, cell 0.44 -> largest 1.26, inside
the rule's 4.  f64 trajectories: largest absolute error pos 5.6e-17, vel 1.9e-17, epot 4.4e-16, ekin 0, cell 0, pressure 2.2e-16 GPa, volume
0, virial 5.3e-15 (bound 1e-9 of magnitudes 0.03 .. 235).  The step's virial against the f64 oracle: 2.2e-15 (f64), 3.6e-6 on 2.8 (f32).
"""
import copy
import ctypes

import numpy as np
import pytest
import torch

from tests import guard_bands as gb
from tests import hessian_cases as hc
from tests import md_oracle as mo
from tests import npt_oracle as no

pytestmark = pytest.mark.gpu
DEV = "cuda"
DT_FS = mo.DT_FS
T_K, TAUT, TAUP = 300.0, 20.0, 100.0
BETA = 0.75                     # 1 / GPa
DP = 1.0                        # GPa: the target above the start's own pressure
ACCEL, KB, GPA = 9.648533212331002e-3, 8.617333262145179e-5, no.GPA_EV_A3
N_STEPS = 6
F32_RATIO_MARGIN = 4.0
EPS32 = float(np.finfo(np.float32).eps)
TRICLINIC = np.array([[7.3, 0.0, 0.0], [0.9, 6.1, 0.0], [-0.5, 0.8, 8.2]])


def _t(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def _np(t):
    return t.detach().double().cpu().numpy()


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _i3(v):
    return (ctypes.c_int32 * 3)(*[int(x) for x in v])


_MODELS = {}


def _model(dtype):
    if dtype not in _MODELS:
        _MODELS[dtype] = copy.deepcopy(hc.model_case("well")[0]).to(device=DEV, dtype=dtype).eval().requires_grad_(False)
    return _MODELS[dtype]


def _system(scale=1.0):
    """(pos, z, masses, cell, v0) of the water box, uniformly scaled: v0 = Maxwell-Boltzmann at T_K from the host generator.  (The MD
    suite's drift of the whole box would be 700 eV of kinetic energy in the pressure.)  The box is shifted along z so that the atom with
    the largest |v_z| starts 0.005 A in front of the face it is heading for and crosses it within the run."""
    def make():
        h = hc.host_case("water box")
        pos, z = h["pos"].numpy().copy(), h["atomic_numbers"].numpy().copy()
        cell = h["cell"].numpy().reshape(3, 3).copy()
        assert np.array_equal(cell, np.diag(np.diag(cell)))
        m = mo.masses_of(z)
        v0 = np.sqrt(KB * T_K * ACCEL / m)[:, None] * mo.normals(7, 1, 0, np.arange(len(z), dtype=np.int64))
        k = int(np.argmax(np.abs(v0[:, 2])))
        pos[:, 2] += (0.005 if v0[k, 2] < 0 else cell[2, 2] - 0.005) - pos[k, 2]
        return pos, z, m, cell, v0

    pos, z, m, cell, v0 = hc.cached(("npt system",), make)
    return scale * pos, z, m, scale * cell, v0


def _host_run(dtype, beta=BETA):
    """The host integrator's run; its target is DP above the f64 start's own pressure (the device runs are handed the same number)."""
    def start():
        pos, z, m, cell, v0 = _system()
        return no.integrate(hc.model_case("well")[1], pos, z, m, cell, dt=DT_FS, n_steps=0, accel=ACCEL, kB=KB, gpa=GPA, temperature=T_K, taut=TAUT,
                            pressure_GPa=0.0, taup=TAUP, compressibility_per_GPa=0.0, v0=v0)["pressure"][0]

    p_start = hc.cached(("npt start pressure",), start)

    def make():
        pos, z, m, cell, v0 = _system()
        return no.integrate(hc.model_case("well")[1], pos, z, m, cell, dt=DT_FS, n_steps=N_STEPS, dtype=dtype, accel=ACCEL, kB=KB, gpa=GPA, temperature=T_K,
                            taut=TAUT, pressure_GPa=p_start + DP, taup=TAUP, compressibility_per_GPa=beta, v0=v0)

    return p_start + DP, hc.cached(("npt host", np.dtype(dtype).name, beta), make)


def _dynamics(dtype, scale=1.0, ensemble="npt_berendsen", pressure_GPa=None, beta=BETA, **extra):
    from xequinet_amd import md

    pos, z, m, cell, v0 = _system(scale)
    kw = dict(timestep_fs=DT_FS, ensemble=ensemble, temperature_K=T_K, taut_fs=TAUT, energy_unit="eV", length_unit="Angstrom")
    if ensemble == "npt_berendsen":
        kw.update(pressure_GPa=_host_run(np.float64)[0] if pressure_GPa is None else pressure_GPa, taup_fs=TAUP, compressibility_per_GPa=beta)
    d = md.Dynamics(_model(dtype), _t(pos, dtype), _t(z), _t(m, torch.float64), cell=_t(cell, dtype), **dict(kw, **extra))
    d.set_velocities(_t(v0, dtype))
    return d


def _state(d):
    s = {"pos": d.unwrapped_positions, "vel": d.velocities, "epot": d.potential_energy, "ekin": d.kinetic_energy, "frc": d.forces,
         "image": d.image.clone(), "wrapped": d.positions}
    if d.ensemble == "npt_berendsen":
        s.update(cell=d.cell, pressure=d.pressure, volume=d.volume, virial=d.virial, box=d.box.clone())
    return s


# ------------------------------------------------------------------------------------------------------------------ 1. tables
def _host_counts(cell, pbc, code):
    from xequinet_amd import lib

    reps = (ctypes.c_int32 * 3)()
    lib.call("xeq_pbc_image_counts", code, ctypes.c_void_p(cell.ctypes.data), 1, _i3(pbc), hc.CUTOFF, reps)
    return [int(v) for v in reps]


def _host_table(cell, reps, code):
    from xequinet_amd import lib

    n = 6 * (2 * reps[0] + 1) * (2 * reps[1] + 1) * (2 * reps[2] + 1) + 12
    out = np.empty(n, dtype=cell.dtype)
    lib.call("xeq_pbc_tables_host", code, ctypes.c_void_p(cell.ctypes.data), 1, _i3(reps), hc.CUTOFF, ctypes.c_void_p(out.ctypes.data), n)
    return out


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("case", ["cubic", "triclinic", "slab", "cubic near the cutoff"])
def test_device_tables_are_the_host_tables_bit_for_bit(case, dtype):
    from xequinet_amd import lib

    code = 0 if dtype == np.float32 else 1
    water = _system()[3]
    cell, pbc = {"cubic": (water, [1, 1, 1]), "triclinic": (TRICLINIC, [1, 1, 1]), "slab": (TRICLINIC[[2, 0, 1]] * 0.7, [1, 0, 1]),
                 "cubic near the cutoff": (water * (hc.CUTOFF * 0.999 / water[0, 0]), [1, 1, 1])}[case]
    cell = np.ascontiguousarray(cell.reshape(1, 3, 3).astype(dtype))
    need = _host_counts(cell, pbc, code)
    assert max(need) >= 1 and all((r > 0) == bool(p) for r, p in zip(need, pbc))
    if case == "cubic near the cutoff":
        assert need == [2, 2, 2]
    for extra in (0, 1):
        reps = [r + extra if p else r for r, p in zip(need, pbc)]
        want = _host_table(cell, reps, code)
        out = gb.guarded((want.size,), torch.float32 if dtype == np.float32 else torch.float64, DEV)
        got_reps = gb.guarded((3,), torch.int32, DEV)
        cell_d = gb.guarded_copy(_t(cell))
        lib.call("xeq_pbc_tables_device", code, _p(cell_d), _i3(reps), _i3(pbc), hc.CUTOFF, _p(out), want.size, _p(got_reps), lib.stream())
        torch.cuda.synchronize()
        gb.check(out, got_reps, cell_d)
        assert out.cpu().numpy().tobytes() == want.tobytes(), (case, extra)
        assert got_reps.cpu().tolist() == need, (case, extra)


# ------------------------------------------------------------------------------------------------------------------ 2. the step
def _load(step, dtype, scale=1.0):
    pos, z, _, cell, _ = _system(scale)
    step._load_cell(_t(cell, dtype), [True, True, True])
    step.pos.copy_(_t(pos, dtype))
    step.z.copy_(_t(z).to(torch.int32))
    step.replay()
    torch.cuda.synchronize()
    return {k: v.clone() for k, v in step.outputs.items()}


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_step_with_a_device_cell_and_a_virial(dtype, monkeypatch):
    from xequinet_amd import keys, ops, runtime
    from xequinet_amd.data.radius_graph import single_radius_graph

    if dtype == torch.float32:      # (`auto` picks the message family by the edge count it knows: pinned, as tests/test_gpu_interface.py does)
        monkeypatch.setenv("XEQ_MESSAGE_IMPL", "wq")
    model = _model(dtype)
    pos, z, _, cell, _ = _system()
    plain = _load(runtime.GraphedStepPBC(model, len(pos), 2048), dtype)
    count = int(plain["n_edges"].item())
    assert count == 1286 and "virial" not in plain and "reps_needed" not in plain
    on_device = runtime.GraphedStepPBC(model, len(pos), 2048, device_cell=True)
    dev = _load(on_device, dtype)
    for k in ("energy", "forces", "n_edges"):
        assert torch.equal(plain[k], dev[k]), k
    assert dev["reps_needed"].cpu().tolist() == on_device.reps == [1, 1, 1]
    wider = runtime.GraphedStepPBC(model, len(pos), 2048, device_cell=True, min_images=[2, 1, 2])      # more images: the same list in the same order
    wide = _load(wider, dtype)
    assert wider.reps == [2, 1, 2] and wide["reps_needed"].cpu().tolist() == [1, 1, 1]
    for k in ("energy", "forces", "n_edges"):
        assert torch.equal(plain[k], wide[k]), k
    assert torch.equal(wider.edge_index[:, :count], on_device.edge_index[:, :count]) and torch.equal(wider.cell_offsets[:count], on_device.cell_offsets[:count])
    # the virial: an edge capacity equal to the count, so that both forms hand the kernels the same sizes
    both = runtime.GraphedStepPBC(model, len(pos), count, compute_virial=True, device_cell=True)
    got = _load(both, dtype)
    x, c = _t(pos, dtype), _t(cell, dtype)
    ei, off, rowptr = single_radius_graph(pos=x, cell=c, pbc=torch.tensor([True, True, True], device=DEV), cutoff=hc.CUTOFF, return_rowptr=True)
    data = {keys.POSITIONS: x.clone(), keys.ATOMIC_NUMBERS: _t(z).to(torch.int32), keys.CELL: c.unsqueeze(0), keys.EDGE_INDEX: ei, keys.CELL_OFFSETS: off,
            keys.BATCH: torch.zeros(len(pos), dtype=torch.int64, device=DEV), keys.BATCH_PTR: torch.tensor([0, len(pos)], dtype=torch.int64, device=DEV),
            keys.EDGE_GRAPH: ops.EdgeGraph(ei, len(pos), center_sorted=True, c_rowptr=rowptr, symmetric=True, cell_offsets=off)}
    with torch.enable_grad():
        eager = model(data, compute_forces=True, compute_virial=True)
    assert got["virial"].shape == (1, 3, 3)
    for k in ("energy", "forces", "virial"):
        assert torch.equal(got[k], eager[k].detach()), k
    assert torch.equal(got["energy"], plain["energy"])
    _, _, w, n_edges = no.evaluate(hc.model_case("well")[1], pos, z, cell, torch.float64)
    err, scale = np.abs(_np(got["virial"]).reshape(3, 3) - w).max(), np.abs(w).max()
    print(f"npt parity: step virial {dtype}: max abs error {err:.3e}, largest {scale:.3e}")
    assert n_edges == count
    if dtype == torch.float64:
        assert err <= 1e-9 * scale


# ------------------------------------------------------------------------------------------------------------------ 3. kernels alone
def _ulp_ok(got, ref, dtype, n_ulp=2):
    if dtype == np.float32:
        return np.all(np.abs(got.astype(np.float64) - ref.astype(np.float64)) <= n_ulp * np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64))
    return np.all(np.abs(got - ref) <= 1e-14 * np.abs(ref))


def _record(cell, cell_next, mu):
    from xequinet_amd import lib

    rec = np.zeros(lib.NPT_BOX)
    rec[lib.NPT_CELL : lib.NPT_CELL + 9], rec[lib.NPT_INV : lib.NPT_INV + 9] = cell.reshape(-1), mo.inverse_cell(cell).reshape(-1)
    rec[lib.NPT_CELL_NEXT : lib.NPT_CELL_NEXT + 9], rec[lib.NPT_INV_NEXT : lib.NPT_INV_NEXT + 9] = cell_next.reshape(-1), mo.inverse_cell(cell_next).reshape(-1)
    rec[lib.NPT_MU] = mu
    return rec


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("n", [1, 63, 65, 1537])
def test_npt_front_kernel_alone(n, dtype):
    from xequinet_amd import lib

    code = 0 if dtype == np.float32 else 1
    rng = np.random.default_rng(400 + n)
    cell = TRICLINIC.astype(dtype).astype(np.float64)
    x = (rng.uniform(0.02, 0.98, (n, 3)) @ cell).astype(dtype)
    v = (2.0 * rng.standard_normal((n, 3))).astype(dtype)                # large enough that atoms leave the box
    f = (3.0 * rng.standard_normal((n, 3))).astype(dtype)
    m = rng.uniform(1.0, 20.0, n)
    m[0] = 0.0                                                           # a fixed atom: scaled with the box, never kicked
    if n > 2:
        m[n // 2] = np.inf
    free = np.isfinite(m) & (m > 0)
    inv_mass = np.where(free, ACCEL / np.where(free, m, 1.0), 0.0).astype(dtype)
    ke, tfac = rng.uniform(0.01, 2.0, 1).astype(dtype), rng.uniform(100.0, 5000.0, 1).astype(dtype)
    for mu in (1.0, 0.9987, 1.0021):
        nxt = (mu * cell).astype(dtype).astype(np.float64)
        rec = _record(cell, nxt, mu)
        for dt in (DT_FS, 0.0):
            if dt > 0:
                xr, vr, ir = no.front(x, v, f, np.zeros((n, 3), np.int32), inv_mass, ke, tfac, dt=dt, dt_over_tau=dt / TAUT, t0=T_K, mu=mu, cell_next=nxt, dtype=dtype)
            else:
                zero = np.zeros((n, 3))
                xr, _, ir = mo.front(x, zero, zero, np.zeros((n, 3), np.int32), inv_mass, np.zeros(n, np.int64), None, tfac, None, ensemble=mo.NVE, dt=0.0,
                                     cell=cell, pbc=no.PBC, dtype=dtype)
                vr = np.where(free[:, None], v, 0.0).astype(dtype)
            g = {k: gb.guarded_copy(_t(a)) for k, a in dict(x=x, v=v, f=f, im=inv_mass, batch=np.zeros(n, np.int64), ke=ke, tfac=tfac, rec=rec,
                                                            cell=np.full(9, -7.0, dtype), image=np.zeros((n, 3), np.int32)).items()}
            system = lib.fill(lib.ResSystem(), dtype=code, n=n, n_graphs=1, pos=g["x"], vel=g["v"], frc=g["f"], image=g["image"], batch=g["batch"])
            par = lib.fill(lib.MdParams(), inv_mass=g["im"], ke=g["ke"], tfac=g["tfac"], dt_over_tau=dt / TAUT, t0=T_K)
            lib.call("xeq_npt_front", ctypes.byref(system), ctypes.byref(par), ctypes.byref(lib.fill(lib.NptParams(), box=g["rec"], step_cell=g["cell"])), dt,
                     lib.stream())
            torch.cuda.synchronize()
            gb.check(*g.values())
            tag = (mu, dt)
            xg, vg, ig, rg = g["x"].cpu().numpy(), g["v"].cpu().numpy(), g["image"].cpu().numpy(), g["rec"].cpu().numpy()
            assert np.array_equal(ig, ir), tag
            assert _ulp_ok(vg, vr, dtype) and _ulp_ok(xg, xr, dtype), tag
            assert np.array_equal(vg[~free], np.zeros_like(vg[~free])), tag
            want = rec.copy()
            if dt > 0:      # committed: the record's current cell and inverse are the pending ones, the step's cell their `dtype` values
                want[lib.NPT_CELL : lib.NPT_CELL + 18] = rec[lib.NPT_CELL_NEXT : lib.NPT_CELL_NEXT + 18]
                assert np.array_equal(g["cell"].cpu().numpy().astype(np.float64), nxt.reshape(-1)), tag
                assert np.abs(ig).max() > 0 or n < 3, tag
                if mu != 1.0:
                    assert not np.array_equal(xg[0], x[0]), tag                                            # the fixed atom moved with the box
            else:
                assert np.array_equal(g["cell"].cpu().numpy(), np.full(9, -7.0, dtype)), tag
            assert np.array_equal(rg, want), tag
            for k, a in dict(f=f, im=inv_mass, ke=ke, tfac=tfac).items():                                  # inputs are inputs
                assert np.array_equal(g[k].cpu().numpy(), a), (tag, k)


def _back_inputs(n, dtype, seed):
    rng = np.random.default_rng(seed)
    v = (0.05 * rng.standard_normal((n, 3))).astype(dtype)
    f = (3.0 * rng.standard_normal((n, 3))).astype(dtype)
    m = rng.uniform(1.0, 20.0, n)
    m[0] = 0.0
    free = m > 0
    inv_mass = np.where(free, ACCEL / np.where(free, m, 1.0), 0.0).astype(dtype)
    half_mass = np.where(free, m / (2 * ACCEL), 0.0).astype(dtype)
    w = rng.standard_normal((3, 3))
    return v * free[:, None].astype(dtype), f, inv_mass, half_mass, (0.5 * (w + w.T) * n).astype(dtype)


def _npt_back_call(dtype, v, f_step, inv_mass, half_mass, virial, rec, *, kappa, p0, needed, reps, book, advance=1, energy=-1.5, n_edges=777):
    from xequinet_amd import lib, md

    n = len(v)
    a0, cn, gp = md.chunk_tables(np.array([0, n]))
    C = len(a0)
    code = 0 if dtype == np.float32 else 1
    tdt = torch.float32 if dtype == np.float32 else torch.float64
    g = {"pos": gb.guarded_copy(_t(np.zeros((n, 3), dtype))), "v": gb.guarded_copy(_t(v)), "frc": gb.guarded((n, 3), tdt, DEV), "fs": gb.guarded_copy(_t(f_step)),
         "en": gb.guarded_copy(_t(np.array([energy], dtype))), "ne": gb.guarded_copy(_t(np.array([n_edges], np.int32))), "ws": gb.guarded_copy(_t(virial)),
         "needed": gb.guarded_copy(_t(np.array(needed, np.int32))), "im": gb.guarded_copy(_t(inv_mass)), "hm": gb.guarded_copy(_t(half_mass)),
         "a0": gb.guarded_copy(_t(a0)), "cn": gb.guarded_copy(_t(cn)), "gp": gb.guarded_copy(_t(gp)), "partial": gb.guarded((C,), torch.float64, DEV),
         "pbad": gb.guarded((C,), torch.int32, DEV), "ke": gb.guarded((1,), tdt, DEV), "epot": gb.guarded((1,), tdt, DEV), "w": gb.guarded((9,), tdt, DEV),
         "seen": gb.guarded_copy(_t(np.zeros(3, np.int32))), "book": gb.guarded_copy(_t(book)), "rec": gb.guarded_copy(_t(rec))}
    system = lib.fill(lib.ResSystem(), dtype=code, n=n, n_graphs=1, n_chunks=C, pos=g["pos"], vel=g["v"], frc=g["frc"], book=g["book"])
    step = lib.fill(lib.ResStep(), frc_step=g["fs"], energy_step=g["en"], n_edges_step=g["ne"], virial_step=g["ws"], reps_needed=g["needed"], reps=tuple(reps))
    chunks = lib.fill(lib.ResChunks(), chunk_atom0=g["a0"], chunk_n=g["cn"], graph_chunk_ptr=g["gp"], partial=g["partial"], partial_bad=g["pbad"])
    par = lib.fill(lib.MdParams(), inv_mass=g["im"], half_mass=g["hm"], ke=g["ke"], epot=g["epot"], half_dt=0.5 * DT_FS)
    box = lib.fill(lib.NptParams(), box=g["rec"], virial=g["w"], reps_seen=g["seen"], kappa=kappa, p0=p0, p_unit=1.0 / GPA)
    lib.call("xeq_npt_back", ctypes.byref(system), ctypes.byref(step), ctypes.byref(chunks), ctypes.byref(par), ctypes.byref(box), None, advance, lib.stream())
    torch.cuda.synchronize()
    gb.check(*g.values())
    return g


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("n", [1, 63, 65, 1537])
def test_npt_back_kernel_alone(n, dtype):
    from xequinet_amd import lib

    v, f, inv_mass, half_mass, w = _back_inputs(n, dtype, 500 + n)
    cell = TRICLINIC.astype(dtype).astype(np.float64)
    rec = _record(cell, cell, 1.0)
    kappa = no.kappa_of(DT_FS, TAUP, BETA, GPA)
    ptr = np.array([0, n])
    for advance in (1, 0):
        vr, ker, _ = mo.back(v, f, inv_mass, half_mass, ptr, 0.5 * DT_FS, dtype, advance=bool(advance))
        p_here = no.pressure(ker[0], w, cell)
        for p0 in (p_here + DP * GPA, p_here - DP * GPA):
            g = _npt_back_call(dtype, v, f, inv_mass, half_mass, w, rec, kappa=kappa, p0=p0, needed=[1, 2, 1], reps=[1, 2, 1],
                               book=np.array([41, 500, 0, 0], np.int64), advance=advance)
            tag = (advance, p0 > p_here)
            assert _ulp_ok(g["v"].cpu().numpy(), vr, dtype) and _ulp_ok(g["ke"].cpu().numpy(), ker, dtype), tag
            assert np.array_equal(g["frc"].cpu().numpy(), f) and np.array_equal(g["epot"].cpu().numpy(), np.array([-1.5], dtype)), tag
            assert np.array_equal(g["w"].cpu().numpy().reshape(3, 3), w), tag
            assert g["book"].cpu().tolist() == [41 + advance, 777, 0, 0] and g["seen"].cpu().tolist() == [1, 2, 1], tag
            # the box half on the kinetic energy the DEVICE stored (its sum order is its own): the oracle's operation order on the same inputs
            want = no.box_back(float(g["ke"].cpu().numpy()[0]), w, cell, kappa, p0, dtype)
            rg = g["rec"].cpu().numpy()
            assert abs(want["mu"] - 1.0) > 5e-4 and (want["mu"] < 1.0) == (p0 > p_here), tag
            for k, val in ((lib.NPT_MU, want["mu"]), (lib.NPT_P, want["P"]), (lib.NPT_V, want["V"])):
                assert abs(rg[k] - val) <= 1e-14 * abs(val), (tag, k, rg[k], val)
            nxt = rg[lib.NPT_CELL_NEXT : lib.NPT_CELL_NEXT + 9].reshape(3, 3)
            assert np.array_equal(nxt.astype(dtype).astype(np.float64), nxt) and _ulp_ok(nxt.astype(dtype), want["cell_next"].astype(dtype), dtype, 1), tag
            inv = rg[lib.NPT_INV_NEXT : lib.NPT_INV_NEXT + 9].reshape(3, 3)
            assert np.abs(inv - mo.inverse_cell(nxt)).max() <= 1e-14 * np.abs(inv).max(), tag
            assert np.array_equal(rg[: lib.NPT_CELL_NEXT], rec[: lib.NPT_CELL_NEXT]), tag                # the current cell is the front's to move
    # more images than the captured counts: the flag and the running maximum; a scale factor that is not positive: the non-finite flag, mu = 1
    g = _npt_back_call(dtype, v, f, inv_mass, half_mass, w, rec, kappa=kappa, p0=p_here, needed=[1, 3, 1], reps=[1, 2, 1], book=np.array([0, 0, 0, 0], np.int64))
    assert g["book"].cpu().tolist() == [1, 777, 0, 1] and g["seen"].cpu().tolist() == [1, 3, 1]
    g = _npt_back_call(dtype, v, f, inv_mass, half_mass, w, rec, kappa=1.0e9, p0=p_here + 1.0, needed=[1, 1, 1], reps=[1, 2, 1], book=np.array([0, 0, 0, 0], np.int64))
    rg = g["rec"].cpu().numpy()
    assert g["book"].cpu().tolist() == [1, 777, 1, 0] and rg[lib.NPT_MU] == 1.0
    assert np.array_equal(rg[lib.NPT_CELL_NEXT : lib.NPT_CELL_NEXT + 9], cell.reshape(-1))
    bad = w.copy()
    bad[1, 1] = np.nan
    g = _npt_back_call(dtype, v, f, inv_mass, half_mass, bad, rec, kappa=kappa, p0=p_here, needed=[1, 1, 1], reps=[1, 2, 1], book=np.array([0, 0, 0, 0], np.int64))
    assert g["book"].cpu().tolist() == [1, 777, 1, 0] and g["rec"].cpu().numpy()[lib.NPT_MU] == 1.0


# ------------------------------------------------------------------------------------------------------------------ 4. trajectories
QUANTITIES = ("pos", "vel", "epot", "ekin", "cell")


def _run_device(dtype):
    d = _dynamics(dtype)
    d.run(N_STEPS, check_every=N_STEPS)
    return d, _state(d)


def test_f64_trajectory_against_the_host_integrator():
    d, got = _run_device(torch.float64)
    _, ref = _host_run(np.float64)
    assert d.step_count == N_STEPS
    moved = abs(ref["cell"][-1][0, 0] / ref["cell"][0][0, 0] - 1.0) / N_STEPS
    print(f"npt parity: the box moved by {100 * moved:.4f} % per step (mu of the start {ref['mu'][0]:.6f})")
    assert 3e-4 < moved < 3e-3
    for k in QUANTITIES + ("pressure", "volume", "virial"):
        want = np.asarray(ref[k][-1], dtype=np.float64)
        err, scale = np.abs(_np(got[k]).reshape(want.shape) - want).max(), np.abs(want).max()
        print(f"npt parity: f64 {k}: max abs error {err:.3e}, largest {scale:.3e}")
        assert err <= 1e-9 * scale, (k, err, scale)
    assert np.array_equal(got["image"].cpu().numpy(), ref["image"][-1]) and np.abs(ref["image"][-1]).max() > 0


def test_f32_trajectory_error_against_the_f32_host_integrator():
    d, got = _run_device(torch.float32)
    ref, own = _host_run(np.float64)[1], _host_run(np.float32)[1]
    for k in QUANTITIES:
        want = np.asarray(ref[k][-1], dtype=np.float64)
        e_dev, e_host, scale = np.abs(_np(got[k]).reshape(want.shape) - want).max(), np.abs(np.asarray(own[k][-1]) - want).max(), np.abs(want).max()
        bound = max(F32_RATIO_MARGIN * e_host, F32_RATIO_MARGIN * EPS32 * scale)
        ratio = e_dev / max(e_host, EPS32 * scale)
        print(f"npt parity: f32 {k}: device {e_dev:.3e} host-f32 {e_host:.3e} largest {scale:.3e} ratio {ratio:.3f}")
        assert e_dev <= bound, (k, e_dev, e_host, scale)
    assert np.abs(got["image"].cpu().numpy()).max() > 0


# ------------------------------------------------------------------------------------------------------------------ 5. invariants
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_without_compressibility_it_is_the_berendsen_thermostat_bit_for_bit(dtype):
    a, b = _dynamics(dtype, beta=0.0), _dynamics(dtype, ensemble="berendsen")
    start = a.cell
    a.run(N_STEPS, check_every=4)
    b.run(N_STEPS, check_every=4)
    sa, sb = _state(a), _state(b)
    for k in sb:
        assert torch.equal(sa[k], sb[k]), k
    assert torch.equal(a.cell, start) and torch.equal(a.cell, b.cell)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_pressure_is_that_of_the_objects_own_state(dtype):
    d = _dynamics(dtype)
    for steps in (0, 3):
        d.run(steps)
        ke, w, c = float(_np(d.kinetic_energy)[0]), _np(d.virial).reshape(3, 3), _np(d.cell)
        vol = abs(np.linalg.det(c))
        want = (2.0 * ke + np.trace(w)) / (3.0 * vol) / GPA
        terms = (2.0 * abs(ke) + np.abs(np.diag(w)).sum()) / (3.0 * vol) / GPA
        got = float(d.pressure)
        print(f"npt parity: pressure {got:.9e} GPa, recomputed {want:.9e} (terms {terms:.3e}), volume {float(d.volume):.6f}")
        assert abs(got - want) <= 1e-12 * terms                     # the same stored values in double, another operation order
        assert abs(float(d.volume) - vol) <= 1e-12 * vol
    assert d.step_count == 3


def test_twins_repeat_and_recorder_rows_are_the_states_of_a_twin():
    a, b, c = _dynamics(torch.float32), _dynamics(torch.float32), _dynamics(torch.float32)
    a.run(N_STEPS, check_every=4, record_every=2)
    c.run(N_STEPS, check_every=N_STEPS, record_every=2)
    t = a.trajectory
    assert t["step"].cpu().tolist() == [2, 4, 6] and t["cell"].shape == (3, 3, 3) and t["pressure"].shape == (3,)
    for k in t:
        assert torch.equal(t[k], c.trajectory[k]), k
    sa, sc = _state(a), _state(c)
    for k in sa:
        assert torch.equal(sa[k], sc[k]), k
    for row in range(3):
        b.run(2)
        assert torch.equal(t["pos"][row], b.unwrapped_positions) and torch.equal(t["epot"][row], b.potential_energy)
        assert torch.equal(t["ekin"][row], b.kinetic_energy) and torch.equal(t["cell"][row], b.cell) and torch.equal(t["pressure"][row], b.pressure)
    assert not torch.equal(t["cell"][0], t["cell"][2])
    a.run(1)
    assert a.trajectory == {} and a.step_count == N_STEPS + 1


def test_run_does_not_touch_the_host_between_checks():
    d = _dynamics(torch.float32, beta=BETA / 10)                  # (0.01 % per step: 36 steps stay inside the captured capacity and images)
    d.run(4, check_every=4)
    captures = d.step.captures
    torch.cuda.synchronize()
    former = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        d.run(32, check_every=32)
    finally:
        torch.cuda.set_sync_debug_mode(former)
    assert d.step_count == 36 and d.step.captures == captures
    assert bool(torch.isfinite(d.kinetic_energy).all()) and bool(torch.isfinite(d.pressure))


# ------------------------------------------------------------------------------------------------------------------ 6. protocols
def test_a_box_compressed_past_an_image_count_is_rerun_bit_for_bit():
    """Every axis starts 0.2 % above the cutoff (one image per axis suffices) and is compressed across it inside one window."""
    length = _system()[3][0, 0]
    scale = 1.002 * hc.CUTOFF / length
    probe = _dynamics(torch.float32, scale=scale, pressure_GPa=0.0)
    target = float(probe.pressure) + DP                             # 0.1 % per step: across the 0.2 % within the window
    small = _dynamics(torch.float32, scale=scale, pressure_GPa=target, edge_capacity=3800)       # (room for the denser box; below 4 096, as above)
    roomy = _dynamics(torch.float32, scale=scale, pressure_GPa=target, edge_capacity=3800, min_images=[2, 2, 2])
    assert small.step.reps == [1, 1, 1] and roomy.step.reps == [2, 2, 2]
    small.run(N_STEPS, check_every=N_STEPS)
    roomy.run(N_STEPS, check_every=N_STEPS)
    print(f"npt parity: image protocol: cell {float(small.cell[0, 0]):.5f} (cutoff {hc.CUTOFF}), captures {small.step.captures} / {roomy.step.captures}")
    assert float(small.cell[0, 0]) < hc.CUTOFF and small.step.reps == [2, 2, 2]
    assert small.step.captures == 2 and roomy.step.captures == 1 and small.step_count == N_STEPS and small.edge_capacity == roomy.edge_capacity == 3800
    a, b = _state(small), _state(roomy)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_a_list_that_outgrows_its_capacity_under_compression_is_rerun_bit_for_bit():
    probe = _dynamics(torch.float32, pressure_GPa=0.0)
    probe.run(0)
    count = int(probe.step.outputs["n_edges"].item())
    target = float(probe.pressure) + 10 * DP                        # 1 % per step: 3 % in density, some forty edges more per step
    small = _dynamics(torch.float32, pressure_GPa=target, edge_capacity=count + 8)
    roomy = _dynamics(torch.float32, pressure_GPa=target, edge_capacity=3000)      # (below 4 096, where `auto` changes the message family)
    small.run(N_STEPS, check_every=3)
    roomy.run(N_STEPS, check_every=3)
    print(f"npt parity: capacity protocol: {count} edges at the start, capacity {small.edge_capacity} at the end, captures {small.step.captures}")
    assert small.step.captures >= 2 and roomy.step.captures == 1 and small.edge_capacity > count + 8
    a, b = _state(small), _state(roomy)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert not torch.equal(small.cell, probe.cell)


def test_a_raised_non_finite_flag_leaves_the_checked_state_cell_included():
    d = _dynamics(torch.float32)
    d.run(2)
    before = _state(d)
    real = d._read_book
    d._read_book = lambda: real()[:2] + (True,)
    with pytest.raises(FloatingPointError, match="steps 2 .. 5"):
        d.run(3)
    d._read_book = real
    assert d.step_count == 2 and d.book.cpu().tolist() == [2, 0, 0, 0]
    after = _state(d)
    for k in before:
        assert torch.equal(before[k], after[k]), k
    assert torch.equal(d.step.cell.reshape(3, 3), d.box[:9].view(3, 3).to(d.dtype))
    d.run(3)
    assert d.step_count == 5 and not torch.equal(d.cell, before["cell"])
