"""Device-resident molecular dynamics (xequinet_amd/md.py, csrc/xeq_md.hip) on the MI355X against the host generator and integrator of
tests/md_oracle.py.  Model: hessian_cases.model_case("well"); time step md_oracle.DT_FS (0.4 fs: omega dt <= 0.163 on every case).

Measured on the MI355X (profiles/md_parity.txt holds every figure; the bounds below are the measured values times the stated margins):
  normals, f32 against the f64 host transform: largest absolute error 2.88e-6 (n = 4 097) -> NORMALS_F32_BOUND = 4 x that
  f32 trajectories: ratio = (device error) / max(f32 host integrator's own error, eps32 x largest magnitude) -- the floor of
  tests/test_gpu_train_edge.py is PART of the ratio: where the host integrator happens to land within a rounding of the f64 result its
  own error says nothing.  Largest over the 36 (system, ensemble, quantity) cases 2.10 (water box, Berendsen, potential energy; median
  1.0) -> the project's usual 4 x holds.  Without the floor the same figures give up to 18 (ragged, Berendsen, potential energy:
  4.9e-7 against a host error of 2.7e-8 on a magnitude of 3.4, i.e. 0.07 eps32)
  f64 trajectories: largest error / largest magnitude 7.3e-16 (bound 1e-9)
"""
import copy
import ctypes

import numpy as np
import pytest
import torch

from tests import guard_bands as gb
from tests import hessian_cases as hc
from tests import md_oracle as mo
from tests import parity_record

pytestmark = pytest.mark.gpu
DEV = "cuda"
DT_FS = mo.DT_FS
T_K, FRICTION, TAUT = 300.0, 0.01, 20.0
ACCEL, KB = 9.648533212331002e-3, 8.617333262145179e-5       # eV, Angstrom (tests/test_md_host.py checks the package's against these)
N_STEPS = 6
NORMALS_F32_MEASURED = 2.88e-6                                # largest |device f32 normal - f64 host transform| (profiles/md_parity.txt)
NORMALS_F32_BOUND = 4 * NORMALS_F32_MEASURED
F32_RATIO_MARGIN = 4.0
SYSTEMS = ["ragged", "qm9 seed 9", "water box"]
ENSEMBLES = ["nve", "langevin", "berendsen"]
EPS32 = float(np.finfo(np.float32).eps)


def _t(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


_MODELS = {}


def _model(dtype):
    if dtype not in _MODELS:
        _MODELS[dtype] = copy.deepcopy(hc.model_case("well")[0]).to(device=DEV, dtype=dtype).eval().requires_grad_(False)
    return _MODELS[dtype]


def _system(name):
    """(pos, z, ptr, masses, cell or None, v0): v0 = Maxwell-Boltzmann at T_K from the host generator; the water box also drifts along
    -z at 0.3 A / fs as a whole (no relative motion: the dynamics is the resting box's), which takes atom 20, 0.445 A above the z = 0 face,
    and others through it within the run."""
    def make():
        h = hc.host_case(name)
        pos, z, ptr = h["pos"].numpy().copy(), h["atomic_numbers"].numpy().copy(), h["ptr"].numpy().copy()
        m = mo.masses_of(z)
        cell = h["cell"].numpy().reshape(3, 3).copy() if "cell" in h else None
        batch = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
        ids = (np.arange(len(z)) - ptr[batch]) | (batch.astype(np.int64) << 32)
        v0 = np.sqrt(KB * T_K * ACCEL / m)[:, None] * mo.normals(7, 1, 0, ids)
        if cell is not None:
            v0[:, 2] -= 0.3
        return pos, z, ptr, m, cell, v0

    return hc.cached(("md system", name), make)


def _kwargs(ensemble, seed=11):
    kw = dict(timestep_fs=DT_FS, ensemble=ensemble, seed=seed)
    if ensemble != "nve":
        kw["temperature_K"] = T_K
    if ensemble == "langevin":
        kw["friction_per_fs"] = FRICTION
    if ensemble == "berendsen":
        kw["taut_fs"] = TAUT
    return kw


def _dynamics(name, ensemble, dtype, pos=None, v0=None, sel=None, rng_id=None, **extra):
    from xequinet_amd import md

    p, z, ptr, m, cell, v = _system(name)
    p = p if pos is None else pos
    v = v if v0 is None else v0
    if sel is not None:             # one graph of the batch, alone
        a, b = int(ptr[sel]), int(ptr[sel + 1])
        p, z, m, v, ptr = p[a:b], z[a:b], m[a:b], v[a:b], np.array([0, b - a])
    kw = dict(_kwargs(ensemble), **extra)
    if cell is not None:
        kw["cell"] = _t(cell, dtype)
    else:
        kw["ptr"] = _t(ptr)
    d = md.Dynamics(_model(dtype), _t(p, dtype), _t(z), _t(m, torch.float64), rng_id=None if rng_id is None else _t(rng_id), energy_unit="eV",
                    length_unit="Angstrom", **kw)
    d.set_velocities(_t(v, dtype))
    return d


def _host_run(name, ensemble, dtype):
    def make():
        p, z, ptr, m, cell, v0 = _system(name)
        return mo.integrate(hc.model_case("well")[1], p, z, ptr, m, dt=DT_FS, n_steps=N_STEPS, ensemble=ensemble, dtype=dtype, accel=ACCEL, kB=KB,
                            temperature=T_K, friction=FRICTION if ensemble == "langevin" else 0.0, taut=TAUT if ensemble == "berendsen" else None,
                            seed=11, v0=v0, cell=cell)

    return hc.cached(("md host", name, ensemble, np.dtype(dtype).name), make)


def _state(d):
    return {"pos": d.unwrapped_positions, "vel": d.velocities, "epot": d.potential_energy, "ekin": d.kinetic_energy, "frc": d.forces,
            "image": d.image.clone(), "wrapped": d.positions}


def _np(t):
    return t.detach().double().cpu().numpy()


# ------------------------------------------------------------------------------------------------------------------ 1. generator
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097])
def test_generator_words_are_the_host_philox_bit_for_bit(n):
    from xequinet_amd import md

    ids_h = np.arange(n, dtype=np.int64) * 3 + ((np.arange(n, dtype=np.int64) % 5) << 32)
    ids = _t(ids_h)
    worst = 0.0
    for seed in (0, 0x9E3779B97F4A7C15):
        for step in (0, 2**32 + 5):
            for purpose in (0, 1):
                w, z = md.normals(seed, purpose, step, ids, torch.float32)
                want = mo.words(seed, purpose, step, ids_h)
                assert np.array_equal(w.cpu().numpy().view(np.uint32), want), (seed, step, purpose)
                ref = mo.box_muller(want)
                worst = max(worst, float(np.abs(z.double().cpu().numpy() - ref).max()))
                z64 = md.normals(seed, purpose, step, ids, torch.float64, want_words=False)[1]
                assert np.abs(z64.cpu().numpy() - ref).max() <= 1e-13          # f64: log / sincos against numpy's, |z| < 7
    print(f"md parity: normals f32 vs f64 host transform, n={n}: max abs error {worst:.3e} (bound {NORMALS_F32_BOUND:.3e})")
    parity_record.add({"test": "md_normals_f32", "n": n, "max_abs_err": worst, "bound": NORMALS_F32_BOUND})
    assert worst <= NORMALS_F32_BOUND


def test_generator_moments():
    """The seed tests/test_md_host.py checked on the host generator: |mean| <= 5 / sqrt(n), |var - 1| <= 5 sqrt(2 / n)."""
    from xequinet_amd import md

    ids = _t(np.arange(4097, dtype=np.int64))
    z = torch.cat([md.normals(2024, 0, s, ids, torch.float32, want_words=False)[1] for s in range(8)]).double().reshape(-1)
    n = z.numel()
    assert n == 4097 * 3 * 8 and bool(torch.isfinite(z).all())
    mean, var = float(z.mean()), float(z.var(unbiased=False))
    print(f"md parity: normals moments n={n}: mean {mean:.3e} var-1 {var - 1:.3e}")
    assert abs(mean) <= 5.0 / np.sqrt(n) and abs(var - 1.0) <= 5.0 * np.sqrt(2.0 / n)


# ------------------------------------------------------------------------------------------------------------------ 2. kernels alone
def _layouts(n):
    """One graph; ragged graphs with an empty one inside and one at the end (n = 1537: 512, 0, 641, 384, 0 atoms)."""
    ragged = np.array([0, n // 3, n // 3, n - n // 4, n, n]) if n > 1 else np.array([0, 0, 1, 1])
    return {"single": np.array([0, n]), "ragged": np.maximum.accumulate(ragged)}


def _ulp_ok(got, ref, dtype, n_ulp=2):
    """f32: within ``n_ulp`` ulp of the f64 evaluation rounded to f32.  f64: 1e-14 relative to the result (the oracle restates the kernel
    operation by operation and the file is built without contraction, so the two differ by library functions at most)."""
    if dtype == np.float32:
        return np.all(np.abs(got.astype(np.float64) - ref.astype(np.float64)) <= n_ulp * np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64))
    return np.all(np.abs(got - ref) <= 1e-14 * np.abs(ref))


def _call(name, *args):
    from xequinet_amd import lib

    lib.call(name, *args)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("n", [1, 63, 65, 1537])
def test_front_kernel_alone(n, dtype):
    from xequinet_amd import lib, md

    tdt = torch.float32 if dtype == np.float32 else torch.float64
    code = 0 if dtype == np.float32 else 1
    rng = np.random.default_rng(100 + n)
    cell = np.array([[7.3, 0.0, 0.0], [0.9, 6.1, 0.0], [-0.5, 0.8, 8.2]]).astype(dtype).astype(np.float64)
    for lname, ptr in _layouts(n).items():
        G = len(ptr) - 1
        batch = np.repeat(np.arange(G), np.diff(ptr))
        frac = rng.uniform(0.02, 0.98, (n, 3))
        x = (frac @ cell).astype(dtype)
        v = (2.0 * rng.standard_normal((n, 3))).astype(dtype)            # large enough that atoms leave the box
        f = (3.0 * rng.standard_normal((n, 3))).astype(dtype)
        m = rng.uniform(1.0, 20.0, n)
        m[0] = 0.0                                                       # a fixed atom
        if n > 2:
            m[n // 2] = np.inf
        free = np.isfinite(m) & (m > 0)
        inv_mass = np.where(free, ACCEL / np.where(free, m, 1.0), 0.0).astype(dtype)
        ke = rng.uniform(0.01, 2.0, G).astype(dtype)
        tfac = rng.uniform(100.0, 5000.0, G).astype(dtype)
        ids = rng.integers(0, 2**40, n).astype(np.int64)
        book_h = np.array([2**32 + 17, 0, 0, 0], dtype=np.int64)
        c1 = float(np.exp(-FRICTION * DT_FS))
        noise2 = (1 - c1 * c1) * KB * T_K
        for ens in (mo.NVE, mo.LANGEVIN, mo.BERENDSEN):
            for periodic in (None, [True, True, True], [True, False, True]):
                zz = md.normals(5, 0, int(book_h[0]), _t(ids), tdt, want_words=False)[1].cpu().numpy()
                xr, vr, ir = mo.front(x, v, f, np.zeros((n, 3), np.int32), inv_mass, batch, ke, tfac, zz, ensemble=ens, dt=DT_FS, c1=c1, noise2=noise2,
                                      dt_over_tau=DT_FS / TAUT, t0=T_K, cell=cell if periodic else None, pbc=periodic, dtype=dtype)
                g = {k: gb.guarded_copy(_t(a)) for k, a in dict(x=x, v=v, f=f, im=inv_mass, batch=batch.astype(np.int64), ke=ke, tfac=tfac, ids=ids,
                                                                book=book_h, image=np.zeros((n, 3), np.int32)).items()}
                cell_c = (ctypes.c_double * 9)(*cell.reshape(-1)) if periodic else None
                pbc_c = (ctypes.c_int32 * 3)(*[int(b) for b in periodic]) if periodic else None
                system = lib.fill(lib.ResSystem(), dtype=code, n=n, n_graphs=G, pos=g["x"], vel=g["v"], frc=g["f"], image=g["image"], batch=g["batch"],
                                  book=g["book"], cell=cell_c, pbc=pbc_c)
                par = lib.fill(lib.MdParams(), ensemble=ens, inv_mass=g["im"], ke=g["ke"], tfac=g["tfac"], rng_id=g["ids"], seed=5, c1=c1, noise2=noise2,
                               dt_over_tau=DT_FS / TAUT, t0=T_K)
                _call("xeq_md_front", ctypes.byref(system), ctypes.byref(par), DT_FS, lib.stream())
                torch.cuda.synchronize()
                gb.check(*g.values())
                tag = (lname, ens, periodic)
                xg, vg, ig = g["x"].cpu().numpy(), g["v"].cpu().numpy(), g["image"].cpu().numpy()
                assert np.array_equal(ig, ir), tag
                assert _ulp_ok(vg, vr, dtype), tag
                assert _ulp_ok(xg, xr, dtype), tag
                assert np.array_equal(vg[~free], np.zeros_like(vg[~free])) and np.array_equal(xg[~free], x[~free]), tag       # a fixed atom does not move
                for k in ("f", "im", "batch", "ke", "tfac", "ids", "book"):                                                   # inputs are inputs
                    assert torch.equal(g[k], _t({"f": f, "im": inv_mass, "batch": batch.astype(np.int64), "ke": ke, "tfac": tfac, "ids": ids, "book": book_h}[k]))
                if periodic:
                    assert np.abs(ig).max() > 0 or n < 3, tag                                                               # somebody did leave the box
                    fr = xg.astype(np.float64) @ mo.inverse_cell(cell)
                    per = np.array(periodic)
                    assert np.all((fr[:, per] >= -1e-6) & (fr[:, per] < 1 + 1e-6)), tag


def _back_call(dtype, ptr, v, f_step, inv_mass, half_mass, energy, n_edges, book, advance=1, half_dt=0.5 * DT_FS):
    from xequinet_amd import lib, md

    n, G = len(v), len(ptr) - 1
    a0, cn, gp = md.chunk_tables(ptr)
    C = len(a0)
    code = 0 if dtype == np.float32 else 1
    tdt = torch.float32 if dtype == np.float32 else torch.float64
    g = {"pos": gb.guarded_copy(_t(np.zeros((n, 3), dtype))), "v": gb.guarded_copy(_t(v)), "frc": gb.guarded((n, 3), tdt, DEV), "fs": gb.guarded_copy(_t(f_step)),
         "en": gb.guarded_copy(_t(energy)), "ne": gb.guarded_copy(_t(np.array([n_edges], np.int32))), "im": gb.guarded_copy(_t(inv_mass)),
         "hm": gb.guarded_copy(_t(half_mass)), "a0": gb.guarded_copy(_t(a0)), "cn": gb.guarded_copy(_t(cn)), "gp": gb.guarded_copy(_t(gp)),
         "partial": gb.guarded((max(C, 1),), torch.float64, DEV), "pbad": gb.guarded((max(C, 1),), torch.int32, DEV), "ke": gb.guarded((G,), tdt, DEV),
         "epot": gb.guarded((G,), tdt, DEV), "book": gb.guarded_copy(_t(book))}
    system = lib.fill(lib.ResSystem(), dtype=code, n=n, n_graphs=G, n_chunks=C, pos=g["pos"], vel=g["v"], frc=g["frc"], book=g["book"])
    step = lib.fill(lib.ResStep(), frc_step=g["fs"], energy_step=g["en"], n_edges_step=g["ne"])
    chunks = lib.fill(lib.ResChunks(), chunk_atom0=g["a0"], chunk_n=g["cn"], graph_chunk_ptr=g["gp"], partial=g["partial"], partial_bad=g["pbad"])
    par = lib.fill(lib.MdParams(), inv_mass=g["im"], half_mass=g["hm"], ke=g["ke"], epot=g["epot"], half_dt=half_dt)
    _call("xeq_md_back", ctypes.byref(system), ctypes.byref(step), ctypes.byref(chunks), ctypes.byref(par), None, advance, lib.stream())
    torch.cuda.synchronize()
    gb.check(*g.values())
    return g


def _back_inputs(n, dtype, seed):
    rng = np.random.default_rng(seed)
    v = (0.05 * rng.standard_normal((n, 3))).astype(dtype)
    f = (3.0 * rng.standard_normal((n, 3))).astype(dtype)
    m = rng.uniform(1.0, 20.0, n)
    m[0] = 0.0
    free = m > 0
    inv_mass = np.where(free, ACCEL / np.where(free, m, 1.0), 0.0).astype(dtype)
    half_mass = np.where(free, m / (2 * ACCEL), 0.0).astype(dtype)
    return v * free[:, None].astype(dtype), f, inv_mass, half_mass


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("n", [1, 63, 65, 1537])
def test_back_kernel_alone(n, dtype):
    v, f, inv_mass, half_mass = _back_inputs(n, dtype, 200 + n)
    for lname, ptr in _layouts(n).items():
        G = len(ptr) - 1
        energy = np.linspace(-3.0, 2.0, G).astype(dtype)
        for advance in (1, 0):
            g = _back_call(dtype, ptr, v, f, inv_mass, half_mass, energy, 777, np.array([41, 500, 0, 0], np.int64), advance=advance)
            vr, ker, _ = mo.back(v, f, inv_mass, half_mass, ptr, 0.5 * DT_FS, dtype, advance=bool(advance))
            assert _ulp_ok(g["v"].cpu().numpy(), vr, dtype), (lname, advance)
            assert _ulp_ok(g["ke"].cpu().numpy(), ker, dtype), (lname, advance)          # (a double sum rounded once: within an ulp of numpy's)
            assert np.array_equal(g["frc"].cpu().numpy(), f) and np.array_equal(g["epot"].cpu().numpy(), energy)
            assert np.array_equal(g["v"].cpu().numpy()[0], np.zeros(3, dtype))           # the fixed atom
            assert g["book"].cpu().tolist() == [41 + advance, 777, 0, 0]
    # a non-finite force raises the flag (the kick still runs: the driver voids the window); a smaller edge count leaves the maximum
    bad = f.copy()
    bad[n // 2, 1] = np.nan
    g = _back_call(dtype, np.array([0, n]), v, bad, inv_mass, half_mass, np.zeros(1, dtype), 3, np.array([0, 500, 0, 0], np.int64))
    assert g["book"].cpu().tolist() == [1, 500, 1, 0]


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("na", [65, 1537])
def test_a_graphs_kinetic_energy_has_the_same_bits_anywhere(na, dtype):
    nb = 300
    va, fa, ima, hma = _back_inputs(na, dtype, 300 + na)
    vb, fb, imb, hmb = _back_inputs(nb, dtype, 301)
    book = np.array([0, 0, 0, 0], np.int64)

    def ke(order):
        parts = {"a": (va, fa, ima, hma), "b": (vb, fb, imb, hmb)}
        cat = [np.concatenate([parts[k][i] for k in order]) for i in range(4)]
        ptr = np.concatenate([[0], np.cumsum([len(parts[k][0]) for k in order])])
        g = _back_call(dtype, ptr, cat[0], cat[1], cat[2], cat[3], np.zeros(len(order), dtype), 1, book)
        return g["ke"].cpu().numpy()[order.index("a")]

    alone, front, back = ke("a"), ke("ab"), ke("ba")
    assert alone > 0 and alone.tobytes() == front.tobytes() == back.tobytes()


# ------------------------------------------------------------------------------------------------------------------ 3. trajectories
def _run_device(name, ensemble, dtype):
    d = _dynamics(name, ensemble, dtype)
    d.run(N_STEPS, check_every=N_STEPS)
    return d, _state(d)


@pytest.mark.parametrize("ensemble", ENSEMBLES)
@pytest.mark.parametrize("name", SYSTEMS)
def test_f64_trajectory_against_the_host_integrator(name, ensemble):
    d, got = _run_device(name, ensemble, torch.float64)
    ref = _host_run(name, ensemble, np.float64)
    assert d.step_count == N_STEPS
    for k in ("pos", "vel", "epot", "ekin"):
        want = ref[k][-1]
        err, scale = np.abs(_np(got[k]) - want).max(), np.abs(want).max()
        print(f"md parity: f64 {name} {ensemble} {k}: max abs error {err:.3e}, largest {scale:.3e}")
        parity_record.add({"test": "md_f64_trajectory", "system": name, "ensemble": ensemble, "quantity": k, "max_abs_err": float(err), "scale": float(scale)})
        assert err <= 1e-9 * scale, (k, err, scale)
    if name == "water box":
        assert np.array_equal(got["image"].cpu().numpy(), ref["image"][-1]) and np.abs(ref["image"][-1]).max() > 0       # an atom crossed a face


@pytest.mark.parametrize("ensemble", ENSEMBLES)
@pytest.mark.parametrize("name", SYSTEMS)
def test_f32_trajectory_error_against_the_f32_host_integrators(name, ensemble):
    d, got = _run_device(name, ensemble, torch.float32)
    ref, own = _host_run(name, ensemble, np.float64), _host_run(name, ensemble, np.float32)
    worst = 0.0
    for k in ("pos", "vel", "epot", "ekin"):
        want = ref[k][-1]
        e_dev, e_host, scale = np.abs(_np(got[k]) - want).max(), np.abs(own[k][-1] - want).max(), np.abs(want).max()
        bound = max(F32_RATIO_MARGIN * e_host, F32_RATIO_MARGIN * EPS32 * scale)
        ratio = e_dev / max(e_host, EPS32 * scale)
        worst = max(worst, ratio)
        print(f"md parity: f32 {name} {ensemble} {k}: device {e_dev:.3e} host-f32 {e_host:.3e} largest {scale:.3e} ratio {ratio:.3f}")
        parity_record.add({"test": "md_f32_trajectory", "system": name, "ensemble": ensemble, "quantity": k, "device_err": float(e_dev),
                           "host_f32_err": float(e_host), "scale": float(scale), "ratio": float(ratio)})
        assert e_dev <= bound, (k, e_dev, e_host, scale)
    if name == "water box":
        assert np.abs(got["image"].cpu().numpy()).max() > 0


# ------------------------------------------------------------------------------------------------------------------ 4. residency
@pytest.mark.parametrize("name", ["qm9 seed 9", "water box"])
def test_run_does_not_touch_the_host_between_checks(name):
    d = _dynamics(name, "langevin", torch.float32)
    d.run(4, check_every=4)                                   # warm: captured, capacity settled
    captures = d.step.captures
    torch.cuda.synchronize()
    former = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        d.run(32, check_every=32)                             # (the one read-back lifts the guard for exactly its own call: md.Dynamics._read_book)
    finally:
        torch.cuda.set_sync_debug_mode(former)
    assert d.step_count == 36
    for _ in range(3):
        d.run(5, check_every=2)
    assert d.step.captures == captures and d.step_count == 51
    assert bool(torch.isfinite(d.kinetic_energy).all())


# ------------------------------------------------------------------------------------------------------------------ 5. capacity / restore
@pytest.mark.parametrize("ensemble", ["nve", "langevin"])
def test_a_list_that_outgrows_its_capacity_is_rerun_bit_for_bit(ensemble):
    roomy = _dynamics("water box", ensemble, torch.float32)
    small = _dynamics("water box", ensemble, torch.float32, edge_capacity=64)       # the first step's list has 1 286 edges
    assert small.edge_capacity == 64
    small.run(12, check_every=4)
    roomy.run(12, check_every=4)
    assert small.step_count == 12 and small.edge_capacity >= 1286 and roomy.edge_capacity >= 1286
    a, b = _state(small), _state(roomy)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_open_boundaries_with_a_too_small_explicit_capacity_raise_with_the_count():
    from xequinet_amd import runtime

    p, z, ptr, m, _, _ = _system("qm9 seed 9")
    d = _dynamics("qm9 seed 9", "nve", torch.float32, edge_capacity=16)
    with pytest.raises(ValueError) as e:
        d.run(2)
    roomy = _dynamics("qm9 seed 9", "nve", torch.float32)
    roomy.run(0)
    count = int(roomy.step.outputs["n_edges"].item())
    assert count > 16 and str(count) in str(e.value) and "16" in str(e.value)
    assert roomy.edge_capacity == runtime.pair_capacity(ptr)


# ------------------------------------------------------------------------------------------------------------------ 6. wrap invariance
def test_a_start_shifted_by_a_lattice_vector_gives_the_same_displacement():
    p, z, ptr, m, cell, v0 = _system("water box")
    a = _dynamics("water box", "nve", torch.float32)
    b = _dynamics("water box", "nve", torch.float32, pos=p + cell[0] - 2 * cell[2])
    start_a, start_b = _np(a.unwrapped_positions), _np(b.unwrapped_positions)
    assert np.abs(start_b - start_a - (cell[0] - 2 * cell[2])).max() < 1e-5 and np.abs(_np(b.positions) - _np(a.positions)).max() < 1e-5
    a.run(N_STEPS)
    b.run(N_STEPS)
    da, db = _np(a.unwrapped_positions) - start_a, _np(b.unwrapped_positions) - start_b
    own = np.abs(_host_run("water box", "nve", np.float32)["pos"][-1] - _host_run("water box", "nve", np.float64)["pos"][-1]).max()
    bound = max(F32_RATIO_MARGIN * own, F32_RATIO_MARGIN * EPS32 * np.abs(start_b).max())
    err = np.abs(da - db).max()
    print(f"md parity: wrap invariance: displacement difference {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    e_own = np.abs(_host_run("water box", "nve", np.float32)["epot"][-1] - _host_run("water box", "nve", np.float64)["epot"][-1]).max()
    e_a, e_b = float(a.potential_energy), float(b.potential_energy)
    print(f"md parity: wrap invariance: energy difference {abs(e_a - e_b):.3e}, f32 host integrator's own error {e_own:.3e}")
    assert abs(e_a - e_b) <= max(F32_RATIO_MARGIN * e_own, F32_RATIO_MARGIN * EPS32 * abs(e_a))


# ------------------------------------------------------------------------------------------------------------------ 7. recorder
@pytest.mark.parametrize("name", ["ragged", "water box"])
def test_recorder_rows_are_the_states_of_a_twin(name):
    a, b = _dynamics(name, "langevin", torch.float32), _dynamics(name, "langevin", torch.float32)
    a.run(6, check_every=4, record_every=2)
    t = a.trajectory
    assert t["step"].cpu().tolist() == [2, 4, 6] and t["pos"].shape == (3, a.n_atoms, 3) and t["epot"].shape == (3, a.n_graphs)
    for row in range(3):
        b.run(2)
        assert torch.equal(t["pos"][row], b.unwrapped_positions) and torch.equal(t["epot"][row], b.potential_energy)
        assert torch.equal(t["ekin"][row], b.kinetic_energy)
    a.run(3)                       # a run without a recorder keeps none
    assert a.trajectory == {} and a.step_count == 9


# ------------------------------------------------------------------------------------------------------------------ 8. replays repeat
@pytest.mark.parametrize("ensemble", ["nve", "langevin"])
def test_twins_and_batch_members_repeat_bit_for_bit(ensemble):
    a, b = _dynamics("qm9 seed 9", ensemble, torch.float32), _dynamics("qm9 seed 9", ensemble, torch.float32)
    a.run(N_STEPS, record_every=1)
    b.run(N_STEPS, check_every=2, record_every=1)
    for k in a.trajectory:
        assert torch.equal(a.trajectory[k], b.trajectory[k]), k
    p, z, ptr, m, _, _ = _system("qm9 seed 9")
    for g in range(len(ptr) - 1):
        lo, hi = int(ptr[g]), int(ptr[g + 1])
        ids = np.arange(hi - lo, dtype=np.int64) | (g << 32)           # the ids the molecule has inside the batch
        alone = _dynamics("qm9 seed 9", ensemble, torch.float32, sel=g, rng_id=ids)
        alone.run(N_STEPS, record_every=1)
        assert torch.equal(alone.trajectory["pos"], a.trajectory["pos"][:, lo:hi]), g
        assert torch.equal(alone.trajectory["epot"][:, 0], a.trajectory["epot"][:, g]) and torch.equal(alone.trajectory["ekin"][:, 0], a.trajectory["ekin"][:, g])
        assert torch.equal(alone.velocities, a.velocities[lo:hi])


def test_a_raised_non_finite_flag_leaves_the_checked_state():
    """The flag itself is the back kernel's (test_back_kernel_alone); here the driver's answer to it: checkpoint back, then the error."""
    d = _dynamics("qm9 seed 9", "nve", torch.float32)
    d.run(2)
    before = _state(d)
    real = d._read_book
    d._read_book = lambda: real()[:2] + (True,)
    with pytest.raises(FloatingPointError, match="steps 2 .. 5"):
        d.run(3)
    d._read_book = real
    assert d.step_count == 2 and d.book.cpu().tolist()[:3] == [2, 0, 0]
    after = _state(d)
    for k in before:
        assert torch.equal(before[k], after[k]), k
    d.run(3)
    assert d.step_count == 5


def test_maxwell_boltzmann_and_zero_momentum():
    d = _dynamics("ragged", "nve", torch.float32)
    p, z, ptr, m, _, _ = _system("ragged")
    d.maxwell_boltzmann(T_K)
    batch = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
    ids = (np.arange(len(z)) - ptr[batch]) | (batch.astype(np.int64) << 32)
    sigma = np.sqrt(KB * T_K * ACCEL / m)[:, None]
    want = sigma * mo.normals(11, 1, 0, ids)
    assert np.abs(_np(d.velocities) - want).max() <= (NORMALS_F32_BOUND + 2 * EPS32 * 7) * sigma.max()
    d.zero_momentum()
    v = _np(d.velocities)
    for a, b in zip(ptr[:-1], ptr[1:]):
        assert np.abs((m[a:b, None] * v[a:b]).sum(0)).max() <= 1e-5 * m[a:b].sum() * max(np.abs(v[a:b]).max(), 1e-30)
    t = _np(d.temperature)
    assert t.shape == (len(ptr) - 1,) and np.all(t >= 0) and np.isfinite(t).all()
