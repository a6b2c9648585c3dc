"""The canonical thermostats of md.Dynamics (ensembles "nose_hoover" and "bussi": xeq_nvt_front / xeq_nvt_back, csrc/xeq_md.hip, DESIGN.md
section 17) on the MI355X against tests/nvt_oracle.py.  Model, systems, time step and tolerances are those of tests/test_gpu_md.py
(rebuilt here from hessian_cases): f64 trajectories to 1e-9 of the largest magnitude, f32 trajectories within F32_RATIO_MARGIN of the f32
host integrator's own error (floor: eps32 of the largest magnitude), kernels alone to 2 ulp of the state's type.

The thermostat's row (scale, bath, xi, vxi) is f64 whatever the state's type and differs from the oracle's by the C library's exp / log /
sqrt / cos against the device's and by the order of the kinetic-energy sum.  Relative to the largest magnitude of the quantity in the
launch (for bath, an energy accumulated from kinetic-energy-sized terms: of bath and of the kinetic energies), measured on the MI355X
(profiles/nvt_parity.txt): NVT_F64_MEASURED; the assertion is 4 x that, and anything above 1e-12 fails outright."""
import copy
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import guard_bands as gb
from tests import hessian_cases as hc
from tests import md_oracle as mo
from tests import nvt_oracle as no
from tests import parity_record

pytestmark = pytest.mark.gpu
DEV = "cuda"
DT_FS = mo.DT_FS
T_K, TAUT = 300.0, 20.0
ACCEL, KB = 9.648533212331002e-3, 8.617333262145179e-5       # eV, Angstrom (tests/test_md_host.py checks the package's against these)
N_STEPS = 6
F32_RATIO_MARGIN = 4.0
EPS32, EPS64 = float(np.finfo(np.float32).eps), float(np.finfo(np.float64).eps)
SYSTEMS = no.TRAJ_SYSTEMS
ENSEMBLES = ["nose_hoover", "bussi"]
NVT_F64_MEASURED = 7.111e-16                                  # largest of the kernel-alone cases: vxi, 63 atoms, f64 state, chain of 8
NVT_F64_CEILING = 1e-12
KT = KB * T_K


def _t(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def _np(t):
    return t.detach().double().cpu().numpy()


_MODELS = {}


def _model(dtype):
    if dtype not in _MODELS:
        _MODELS[dtype] = copy.deepcopy(hc.model_case("well")[0]).to(device=DEV, dtype=dtype).eval().requires_grad_(False)
    return _MODELS[dtype]


def _system(name):
    """(pos, z, ptr, masses, cell or None, v0) as tests/test_gpu_md.py builds them: Maxwell-Boltzmann velocities at T_K from the host
    generator; the water box drifts along -z at 0.3 A / fs as a whole, which takes atoms through the z = 0 face within the run."""
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

    return hc.cached(("nvt system", name), make)


def _dynamics(name, ensemble, dtype, sel=None, graph_rng_id=None, **extra):
    from xequinet_amd import md

    p, z, ptr, m, cell, v = _system(name)
    if sel is not None:             # one graph of the batch, alone
        a, b = int(ptr[sel]), int(ptr[sel + 1])
        p, z, m, v, ptr = p[a:b], z[a:b], m[a:b], v[a:b], np.array([0, b - a])
    kw = dict(timestep_fs=DT_FS, ensemble=ensemble, temperature_K=T_K, taut_fs=TAUT, **extra)
    if ensemble == "bussi":
        kw.update(seed=no.TRAJ_SEED, graph_rng_id=None if graph_rng_id is None else _t(graph_rng_id))
    if cell is not None:
        kw["cell"] = _t(cell, dtype)
    else:
        kw["ptr"] = _t(ptr)
    d = md.Dynamics(_model(dtype), _t(p, dtype), _t(z), _t(m, torch.float64), energy_unit="eV", length_unit="Angstrom", **kw)
    d.set_velocities(_t(v, dtype))
    return d


def _host_run(name, ensemble, dtype):
    def make():
        p, z, ptr, m, cell, v0 = _system(name)
        return no.integrate(hc.model_case("well")[1], p, z, ptr, m, dt=DT_FS, n_steps=N_STEPS, ensemble=ensemble, dtype=dtype, accel=ACCEL, kB=KB,
                            temperature=T_K, taut=TAUT, seed=no.TRAJ_SEED, v0=v0, cell=cell)

    return hc.cached(("nvt host", name, ensemble, np.dtype(dtype).name), make)


def _state(d):
    return {"pos": d.unwrapped_positions, "vel": d.velocities, "epot": d.potential_energy, "ekin": d.kinetic_energy, "bath": d.thermostat_energy,
            "frc": d.forces, "image": d.image.clone(), "wrapped": d.positions, "raw vel": d.vel.clone(), "row": d.thermo.clone()}


def _ulp_ok(got, ref, dtype, n_ulp=2):
    """tests/test_gpu_md.py's rule.  f32: within ``n_ulp`` ulp of the f64 evaluation rounded to f32.  f64: 1e-14 relative to the result."""
    if dtype == np.float32:
        return np.all(np.abs(got.astype(np.float64) - ref.astype(np.float64)) <= n_ulp * np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64))
    return np.all(np.abs(got - ref) <= 1e-14 * np.abs(ref))


_WORST = {"value": 0.0}


def _row_parity(tag, got, ref, k_sums):
    """The thermostat rows of one launch against the oracle's: the largest error of each quantity relative to its largest magnitude."""
    for name, cols in (("scale", slice(no.SCALE, no.SCALE + 1)), ("bath", slice(no.BATH, no.BATH + 1)), ("xi", slice(no.XI, no.VXI)),
                       ("vxi", slice(no.VXI, no.ROW))):
        g, r = got[:, cols], ref[:, cols]
        assert np.isfinite(g).all(), (tag, name)
        size = np.abs(r).max() if r.size else 0.0
        if name == "bath":
            size = max(size, float(np.max(k_sums))) if len(k_sums) else size
        err = np.abs(g - r).max() if r.size else 0.0
        rel = 0.0 if err == 0.0 else err / size
        _WORST["value"] = max(_WORST["value"], rel)
        parity_record.add({"test": "nvt_row_f64", "case": str(tag), "quantity": name, "rel_err": float(rel)})
        print(f"nvt parity: row {tag} {name}: relative error {rel:.3e} (worst so far {_WORST['value']:.3e})")
        assert rel <= NVT_F64_CEILING, (tag, name, rel)
        assert rel <= 4.0 * NVT_F64_MEASURED, (tag, name, rel)


# ------------------------------------------------------------------------------------------------------------------ 1. back kernel alone
def _layout(name):
    """(ptr, free [n]) of a kernel-alone layout: a single graph of ``name`` atoms, "ragged" (nvt_oracle.RAGGED_SIZES: an empty graph, a last
    graph whose atoms are all fixed) or "many" one-atom graphs."""
    sizes = no.RAGGED_SIZES if name == "ragged" else [1] * no.MANY_GRAPHS if name == "many" else [int(name)]
    ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    free = np.ones(int(ptr[-1]), dtype=bool)
    if name == "ragged":
        free[ptr[-2]:] = False
    return ptr, free


def _inputs(ptr, free, dtype, seed):
    n, G = int(ptr[-1]), len(ptr) - 1
    rng = np.random.default_rng(seed)
    v = (0.05 * rng.standard_normal((n, 3))).astype(dtype) * free[:, None].astype(dtype)
    f = (3.0 * rng.standard_normal((n, 3))).astype(dtype)
    m = rng.uniform(1.0, 20.0, n)
    inv_mass = np.where(free, ACCEL / m, 0.0).astype(dtype)
    half_mass = np.where(free, m / (2 * ACCEL), 0.0).astype(dtype)
    n_free = np.array([free[a:b].sum() for a, b in zip(ptr[:-1], ptr[1:])], dtype=np.int64)
    state = np.zeros((G, no.ROW))
    state[:, no.SCALE] = rng.uniform(0.9, 1.1, G)
    state[:, no.BATH] = rng.uniform(-0.5, 0.5, G)
    state[:, no.XI : no.VXI] = rng.uniform(-0.5, 0.5, (G, no.MAX_CHAIN))
    state[:, no.VXI : no.ROW] = rng.uniform(-0.02, 0.02, (G, no.MAX_CHAIN))
    return v, f, inv_mass, half_mass, n_free, state


def _nvt_record(lib, kind, g, chain, tau=TAUT, dt=DT_FS):
    return lib.fill(lib.NvtParams(), kind=kind, state=g["state"], n_free=g["n_free"], graph_rng_id=g["gid"], chain_length=chain, kT=KT, tau=tau, dt=dt)


def _back_call(dtype, kind, chain, ptr, v, f_step, inv_mass, half_mass, n_free, state, energy, book, advance=1, tau=TAUT, seed=no.KERNEL_SEED):
    from xequinet_amd import lib, md

    n, G = len(v), len(ptr) - 1
    a0, cn, gp = md.chunk_tables(ptr)
    C = len(a0)
    code = 0 if dtype == np.float32 else 1
    tdt = torch.float32 if dtype == np.float32 else torch.float64
    g = {"pos": gb.guarded_copy(_t(np.zeros((n, 3), dtype))), "v": gb.guarded_copy(_t(v)), "frc": gb.guarded((n, 3), tdt, DEV), "fs": gb.guarded_copy(_t(f_step)),
         "en": gb.guarded_copy(_t(energy)), "ne": gb.guarded_copy(_t(np.array([7], np.int32))), "im": gb.guarded_copy(_t(inv_mass)),
         "hm": gb.guarded_copy(_t(half_mass)), "a0": gb.guarded_copy(_t(a0)), "cn": gb.guarded_copy(_t(cn)), "gp": gb.guarded_copy(_t(gp)),
         "partial": gb.guarded((max(C, 1),), torch.float64, DEV), "pbad": gb.guarded((max(C, 1),), torch.int32, DEV), "ke": gb.guarded((G,), tdt, DEV),
         "epot": gb.guarded((G,), tdt, DEV), "book": gb.guarded_copy(_t(book)), "state": gb.guarded_copy(_t(state)),
         "n_free": gb.guarded_copy(_t(n_free)), "gid": gb.guarded_copy(_t(np.arange(G, dtype=np.int64) << 32))}
    system = lib.fill(lib.ResSystem(), dtype=code, n=n, n_graphs=G, n_chunks=C, pos=g["pos"], vel=g["v"], frc=g["frc"], book=g["book"])
    step = lib.fill(lib.ResStep(), frc_step=g["fs"], energy_step=g["en"], n_edges_step=g["ne"])
    chunks = lib.fill(lib.ResChunks(), chunk_atom0=g["a0"], chunk_n=g["cn"], graph_chunk_ptr=g["gp"], partial=g["partial"], partial_bad=g["pbad"])
    par = lib.fill(lib.MdParams(), inv_mass=g["im"], half_mass=g["hm"], ke=g["ke"], epot=g["epot"], half_dt=0.5 * DT_FS, seed=seed)
    nvt = _nvt_record(lib, kind, g, chain, tau=tau)
    lib.call("xeq_nvt_back", ctypes.byref(system), ctypes.byref(step), ctypes.byref(chunks), ctypes.byref(par), ctypes.byref(nvt), None, advance, lib.stream())
    torch.cuda.synchronize()
    gb.check(*g.values())
    return g


def _sums(e, ptr):
    return np.array([e[a:b].sum() for a, b in zip(ptr[:-1], ptr[1:])])


THERMOSTATS = [("nose_hoover", 3), ("nose_hoover", 8), ("nose_hoover", 1), ("bussi", 0)]
BOOK = np.array([no.KERNEL_STEP, 500, 0, 0], np.int64)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("layout", [*[str(n) for n in no.SINGLE_SIZES], "ragged", "many"])
def test_back_kernel_alone(layout, dtype):
    ptr, free = _layout(layout)
    G = len(ptr) - 1
    v, f, inv_mass, half_mass, n_free, state0 = _inputs(ptr, free, dtype, 400 + len(free))
    energy = np.linspace(-3.0, 2.0, G).astype(dtype)
    for name, chain in THERMOSTATS:
        kind = no.KINDS[name]
        for advance in (1, 0):
            g = _back_call(dtype, kind, chain, ptr, v, f, inv_mass, half_mass, n_free, state0, energy, BOOK, advance=advance)
            vr, _, e = mo.back(v, f, inv_mass, half_mass, ptr, 0.5 * DT_FS, dtype, advance=bool(advance))
            k_sums = _sums(e, ptr)
            want, ker, bad = no.join(kind, state0, k_sums, n_free, advance=bool(advance), kT=KT, tau=TAUT, dt=DT_FS, chain_length=chain,
                                     seed=no.KERNEL_SEED, step=no.KERNEL_STEP, dtype=dtype)
            tag = (layout, np.dtype(dtype).name, name, chain, advance)
            got = g["state"].cpu().numpy()
            assert not bad and g["book"].cpu().tolist() == [no.KERNEL_STEP + advance, 500, 0, 0], tag
            assert _ulp_ok(g["v"].cpu().numpy(), vr, dtype), tag                       # vel holds the velocities BEFORE the factor
            assert _ulp_ok(g["ke"].cpu().numpy(), ker, dtype), tag
            assert np.array_equal(g["frc"].cpu().numpy(), f) and np.array_equal(g["epot"].cpu().numpy(), energy), tag
            _row_parity(tag, got, want, k_sums)
            if not advance:                                                             # no thermostat acts: factor 1, the rest of the row untouched
                assert np.all(got[:, no.SCALE] == 1.0) and np.array_equal(got[:, 1:], state0[:, 1:]), tag
                assert _ulp_ok(g["ke"].cpu().numpy(), k_sums.astype(dtype), dtype), tag
            else:
                acted = (n_free > 0) & (k_sums > 0)
                assert np.all(got[~acted, no.SCALE] == 1.0) and np.array_equal(got[~acted, 1:], state0[~acted, 1:]), tag       # an empty graph, fixed atoms
                assert np.all(got[acted, no.SCALE] != 1.0) and np.all(got[acted, no.SCALE] > 0.5) and np.all(got[acted, no.SCALE] < 2.0), tag
                if kind == no.NOSE_HOOVER and chain < no.MAX_CHAIN:                                                             # links beyond the chain are not its
                    assert np.array_equal(got[:, no.XI + chain : no.VXI], state0[:, no.XI + chain : no.VXI]), tag
                    assert np.array_equal(got[:, no.VXI + chain :], state0[:, no.VXI + chain :]), tag
                if kind == no.BUSSI:
                    assert np.array_equal(got[:, no.XI :], state0[:, no.XI :]), tag


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_back_kernel_without_kinetic_energy_leaves_the_row(dtype):
    """K = 0 (resting atoms, no force) and a graph whose atoms are all fixed: factor 1, nothing non-finite, the row untouched."""
    for layout, fixed in (("65", False), ("257", False), ("65", True), ("ragged", False)):
        ptr, free = _layout(layout)
        if fixed:
            free[:] = False
        v, f, inv_mass, half_mass, n_free, state0 = _inputs(ptr, free, dtype, 77)
        v[:], f[:] = 0.0, 0.0
        for name, chain in (("nose_hoover", 3), ("bussi", 0)):
            g = _back_call(dtype, no.KINDS[name], chain, ptr, v, f, inv_mass, half_mass, n_free, state0, np.zeros(len(ptr) - 1, dtype), BOOK)
            got = g["state"].cpu().numpy()
            assert np.isfinite(got).all() and np.all(got[:, no.SCALE] == 1.0) and np.array_equal(got[:, 1:], state0[:, 1:]), (layout, fixed, name)
            assert np.array_equal(g["ke"].cpu().numpy(), np.zeros(len(ptr) - 1, dtype)) and g["book"].cpu().tolist() == [no.KERNEL_STEP + 1, 500, 0, 0]


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("name,chain", [("nose_hoover", 3), ("bussi", 0)])
def test_a_graphs_thermostat_has_the_same_bits_anywhere(name, chain, dtype):
    """A graph of 1 537 atoms (the wide join) and one of 65 (the serial one), alone and behind / in front of another graph, with their ids."""
    parts = {}
    for key, n, seed in (("a", 1537, 31), ("b", 300, 32), ("c", 65, 33)):
        ptr, free = _layout(str(n))
        parts[key] = _inputs(ptr, free, dtype, seed)

    def run(order):
        cat = [np.concatenate([parts[k][i] for k in order]) for i in range(4)]
        ptr = np.concatenate([[0], np.cumsum([len(parts[k][0]) for k in order])])
        n_free = np.concatenate([parts[k][4] for k in order])
        state = np.concatenate([parts[k][5] for k in order])
        # (_back_call numbers the ids by position: a Bussi row is compared where the graph keeps its number)
        g = _back_call(dtype, no.KINDS[name], chain, ptr, cat[0], cat[1], cat[2], cat[3], n_free, state, np.zeros(len(order), dtype), BOOK)
        return g["state"].cpu().numpy(), g["ke"].cpu().numpy()

    for key in ("a", "c"):
        alone_s, alone_k = run(key)
        front_s, front_k = run(key + "b")                       # graph 0 in both: the same id
        assert alone_s[0].tobytes() == front_s[0].tobytes() and alone_k[0].tobytes() == front_k[0].tobytes(), key
        if name == "nose_hoover":                                # (no generator: the position in the batch does not matter either)
            back_s, back_k = run("b" + key)
            assert alone_s[0].tobytes() == back_s[1].tobytes() and alone_k[0].tobytes() == back_k[1].tobytes(), key


# ------------------------------------------------------------------------------------------------------------------ 2. front kernel alone
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("n", [1, 65, 1537])
def test_front_kernel_alone(n, dtype):
    from xequinet_amd import lib

    code = 0 if dtype == np.float32 else 1
    rng = np.random.default_rng(500 + n)
    cell = np.array([[7.3, 0.0, 0.0], [0.9, 6.1, 0.0], [-0.5, 0.8, 8.2]]).astype(dtype).astype(np.float64)
    ptr = np.array([0, n // 3, n // 3, n - n // 4, n, n]) if n > 1 else np.array([0, 0, 1, 1])
    G = len(ptr) - 1
    batch = np.repeat(np.arange(G), np.diff(ptr))
    x = (rng.uniform(0.02, 0.98, (n, 3)) @ cell).astype(dtype)
    v = (2.0 * rng.standard_normal((n, 3))).astype(dtype)
    f = (3.0 * rng.standard_normal((n, 3))).astype(dtype)
    m = rng.uniform(1.0, 20.0, n)
    if n > 2:
        m[0], m[n // 2] = 0.0, np.inf                                     # fixed atoms
    free = np.isfinite(m) & (m > 0)
    inv_mass = np.where(free, ACCEL / np.where(free, m, 1.0), 0.0).astype(dtype)
    state0 = np.zeros((G, no.ROW))
    state0[:, no.SCALE] = rng.uniform(0.8, 1.2, G)
    state0[:, 1:] = rng.uniform(-1.0, 1.0, (G, no.ROW - 1))
    for periodic in (None, [True, True, True], [True, False, True]):
        for dt in (DT_FS, 0.0):
            scaled = state0[batch, no.SCALE][:, None] * v.astype(np.float64) if dt > 0 else v.astype(np.float64)
            xr, vr, ir = mo.front(x, scaled, f, np.zeros((n, 3), np.int32), inv_mass, batch, None, None, None, ensemble=mo.NVE, dt=dt,
                                  cell=cell if periodic else None, pbc=periodic, dtype=dtype)
            g = {k: gb.guarded_copy(_t(a)) for k, a in dict(x=x, v=v, f=f, im=inv_mass, batch=batch.astype(np.int64), state=state0,
                                                            image=np.zeros((n, 3), np.int32), n_free=np.ones(G, np.int64), gid=np.zeros(G, np.int64)).items()}
            cell_c = (ctypes.c_double * 9)(*cell.reshape(-1)) if periodic else None
            pbc_c = (ctypes.c_int32 * 3)(*[int(b) for b in periodic]) if periodic else None
            system = lib.fill(lib.ResSystem(), dtype=code, n=n, n_graphs=G, pos=g["x"], vel=g["v"], frc=g["f"], image=g["image"], batch=g["batch"],
                              cell=cell_c, pbc=pbc_c)
            par = lib.fill(lib.MdParams(), inv_mass=g["im"])
            nvt = _nvt_record(lib, no.NOSE_HOOVER, g, 3)
            lib.call("xeq_nvt_front", ctypes.byref(system), ctypes.byref(par), ctypes.byref(nvt), dt, lib.stream())
            torch.cuda.synchronize()
            gb.check(*g.values())
            tag = (n, periodic, dt)
            xg, vg, ig = g["x"].cpu().numpy(), g["v"].cpu().numpy(), g["image"].cpu().numpy()
            assert np.array_equal(g["state"].cpu().numpy(), state0), tag                  # the front never writes the row: the factor survives
            assert np.array_equal(ig, ir), tag
            assert _ulp_ok(xg, xr, dtype), tag
            assert np.array_equal(vg[~free], np.zeros_like(vg[~free])) and np.array_equal(xg[~free], xr[~free]), tag       # a fixed atom stays as it is
            if dt == 0.0:                                                                 # the wrap alone: no kick, no factor
                assert np.array_equal(vg[free], v[free]), tag
            else:
                assert _ulp_ok(vg, vr, dtype), tag


# ------------------------------------------------------------------------------------------------------------------ 3. the draws
@pytest.mark.parametrize("nf", no.MOMENT_NF)
def test_one_launch_draws_the_oracles_chi_squares(nf):
    """4 096 graphs of Nf / 3 atoms in one launch, tau = 2 dt (c = exp(-1/2): the statement is well conditioned in S).  The S each factor
    implies against the oracle's draw, one by one: S = (s^2 - c - 2 R sqrt(c q)) / q - R^2 carries the roundings of the device's dozen
    operations, the libraries' last bits in exp / log / sqrt / cos and the order of a sum of at most 21 terms, each at most an eps of the
    terms' magnitudes: 64 eps of (s^2 + c + |2 R| sqrt(c q)) / q + R^2 + S bounds it.  Their mean: the bound tests/test_nvt_host.py
    shows the oracle's own draws to keep."""
    G, per, tau = no.MOMENT_GRAPHS, nf // 3, 2.0 * DT_FS
    ptr = np.arange(G + 1, dtype=np.int64) * per
    free = np.ones(G * per, dtype=bool)
    v, f, inv_mass, half_mass, n_free, state0 = _inputs(ptr, free, np.float64, 600 + nf)
    book = np.array([no.MOMENT_STEP, 0, 0, 0], np.int64)
    g = _back_call(np.float64, no.BUSSI, 0, ptr, v, f, inv_mass, half_mass, n_free, state0, np.zeros(G), book, tau=tau, seed=no.MOMENT_SEED)
    scale = g["state"].cpu().numpy()[:, no.SCALE]
    _, _, e = mo.back(v, f, inv_mass, half_mass, ptr, 0.5 * DT_FS, np.float64)
    k_sums = _sums(e, ptr)
    c = math.exp(-(DT_FS / tau))
    implied, worst = np.zeros(G), 0.0
    for j in range(G):
        r, s_want = no.chi_square(nf, no.MOMENT_SEED, j << 32, no.MOMENT_STEP)
        implied[j] = no.implied_chi_square(float(scale[j]), float(k_sums[j]), nf, KT, tau, DT_FS, r)
        q = ((1.0 - c) * (0.5 * (nf * KT))) / (nf * float(k_sums[j]))
        bound = 64 * EPS64 * ((scale[j] ** 2 + c + abs(2 * r) * math.sqrt(c * q)) / q + r * r + s_want)
        worst = max(worst, abs(implied[j] - s_want) / bound)
        assert abs(implied[j] - s_want) <= bound, (j, implied[j], s_want, bound)
    limit = 5.0 * math.sqrt(2.0 * (nf - 1) / G)
    print(f"nvt parity: chi-square Nf={nf}: largest error / bound {worst:.3f}; mean {implied.mean():.4f} (want {nf - 1}, bound {limit:.4f})")
    assert abs(implied.mean() - (nf - 1)) <= limit


# ------------------------------------------------------------------------------------------------------------------ 4. trajectories
def _run_device(name, ensemble, dtype):
    d = _dynamics(name, ensemble, dtype)
    d.run(N_STEPS, check_every=N_STEPS)
    return d, _state(d)


def _size(ref, k):
    """The largest magnitude a quantity's error is held against; the thermostat's energy is accumulated from kinetic-energy-sized terms."""
    size = np.abs(ref[k][-1]).max()
    return max(size, np.abs(ref["ekin"][-1]).max()) if k == "bath" else size


@pytest.mark.parametrize("ensemble", ENSEMBLES)
@pytest.mark.parametrize("name", SYSTEMS)
def test_f64_trajectory_against_the_host_integrator(name, ensemble):
    d, got = _run_device(name, ensemble, torch.float64)
    ref = _host_run(name, ensemble, np.float64)
    assert d.step_count == N_STEPS
    for k in ("pos", "vel", "epot", "ekin", "bath"):
        want = ref[k][-1]
        err, size = np.abs(_np(got[k]) - want).max(), _size(ref, k)
        print(f"nvt parity: f64 {name} {ensemble} {k}: max abs error {err:.3e}, largest {size:.3e}")
        parity_record.add({"test": "nvt_f64_trajectory", "system": name, "ensemble": ensemble, "quantity": k, "max_abs_err": float(err), "scale": float(size)})
        assert err <= 1e-9 * size, (k, err, size)
    assert np.abs(ref["bath"][-1]).max() > 0 and np.any(_np(d.thermo[:, no.SCALE]) != 1.0)             # a factor IS pending
    assert np.allclose(_np(d.conserved_energy), _np(got["epot"]) + _np(got["ekin"]) + _np(got["bath"]), rtol=1e-14, atol=0)
    assert np.allclose(_np(d.temperature), _np(got["ekin"]) * 2.0 / (3.0 * np.diff(_system(name)[2]) * KB), rtol=1e-12)
    if name == "water box":
        assert np.array_equal(got["image"].cpu().numpy(), ref["image"][-1]) and np.abs(ref["image"][-1]).max() > 0       # an atom crossed a face


@pytest.mark.parametrize("ensemble", ENSEMBLES)
@pytest.mark.parametrize("name", SYSTEMS)
def test_f32_trajectory_error_against_the_f32_host_integrators(name, ensemble):
    d, got = _run_device(name, ensemble, torch.float32)
    ref, own = _host_run(name, ensemble, np.float64), _host_run(name, ensemble, np.float32)
    for k in ("pos", "vel", "epot", "ekin", "bath"):
        want = ref[k][-1]
        e_dev, e_host, size = np.abs(_np(got[k]) - want).max(), np.abs(own[k][-1] - want).max(), _size(ref, k)
        bound = max(F32_RATIO_MARGIN * e_host, F32_RATIO_MARGIN * EPS32 * size)
        ratio = e_dev / max(e_host, EPS32 * size)
        print(f"nvt parity: f32 {name} {ensemble} {k}: device {e_dev:.3e} host-f32 {e_host:.3e} largest {size:.3e} ratio {ratio:.3f}")
        parity_record.add({"test": "nvt_f32_trajectory", "system": name, "ensemble": ensemble, "quantity": k, "device_err": float(e_dev),
                           "host_f32_err": float(e_host), "scale": float(size), "ratio": float(ratio)})
        assert e_dev <= bound, (k, e_dev, e_host, size)
    if name == "water box":
        assert np.array_equal(got["image"].cpu().numpy(), own["image"][-1]) and np.abs(got["image"].cpu().numpy()).max() > 0


# ------------------------------------------------------------------------------------------------------------------ 5. same bits
@pytest.mark.parametrize("ensemble", ENSEMBLES)
def test_twins_batch_members_and_split_runs_repeat_bit_for_bit(ensemble):
    a, b, c = (_dynamics("ragged", ensemble, torch.float32) for _ in range(3))
    a.run(N_STEPS, record_every=1)
    b.run(N_STEPS, check_every=2, record_every=1)
    for k in a.trajectory:
        assert torch.equal(a.trajectory[k], b.trajectory[k]), k
    c.run(2)
    c.run(4)                                                                  # run(2); run(4) is run(6)
    sa, sb, sc = _state(a), _state(b), _state(c)
    for k in sa:
        assert torch.equal(sa[k], sb[k]) and torch.equal(sa[k], sc[k]), k
    ptr = _system("ragged")[2]
    for g in range(len(ptr) - 1):
        lo, hi = int(ptr[g]), int(ptr[g + 1])
        alone = _dynamics("ragged", ensemble, torch.float32, sel=g, graph_rng_id=np.array([g << 32], dtype=np.int64) if ensemble == "bussi" else None)
        alone.run(N_STEPS, record_every=1)
        assert torch.equal(alone.trajectory["pos"], a.trajectory["pos"][:, lo:hi]), g
        assert torch.equal(alone.trajectory["epot"][:, 0], a.trajectory["epot"][:, g]) and torch.equal(alone.trajectory["ekin"][:, 0], a.trajectory["ekin"][:, g])
        assert torch.equal(alone.velocities, a.velocities[lo:hi]) and torch.equal(alone.thermo[0], a.thermo[g]), g


@pytest.mark.parametrize("ensemble", ENSEMBLES)
def test_a_list_that_outgrows_its_capacity_is_rerun_bit_for_bit(ensemble):
    roomy = _dynamics("water box", ensemble, torch.float32)
    small = _dynamics("water box", ensemble, torch.float32, edge_capacity=64)       # the first step's list has 1 286 edges
    assert small.edge_capacity == 64
    small.run(12, check_every=4)
    roomy.run(12, check_every=4)
    assert small.step_count == 12 and small.edge_capacity >= 1286
    a, b = _state(small), _state(roomy)
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("ensemble", ENSEMBLES)
@pytest.mark.parametrize("name", ["ragged", "water box"])
def test_recorder_rows_are_the_states_of_a_twin(name, ensemble):
    a, b = _dynamics(name, ensemble, torch.float32), _dynamics(name, ensemble, torch.float32)
    a.run(6, check_every=4, record_every=2)
    t = a.trajectory
    assert t["step"].cpu().tolist() == [2, 4, 6]
    for row in range(3):
        b.run(2)
        assert torch.equal(t["pos"][row], b.unwrapped_positions) and torch.equal(t["epot"][row], b.potential_energy)
        assert torch.equal(t["ekin"][row], b.kinetic_energy)


def test_set_up_calls_reset_the_pending_factor_and_other_ensembles_keep_no_thermostat_energy():
    d = _dynamics("ragged", "bussi", torch.float32)
    d.run(3)
    assert bool((d.thermo[:, no.SCALE] != 1.0).all())
    seen = d.velocities
    assert not torch.equal(seen, d.vel) and torch.equal(seen, (d.vel.double() * d.thermo[:, no.SCALE][d.step.batch[: d.n_atoms]][:, None]).float())
    ke = d.kinetic_energy
    d.zero_momentum()                                                          # acts on the velocities behind the factor
    assert bool((d.thermo[:, no.SCALE] == 1.0).all())
    p, z, ptr, m, _, _ = _system("ragged")
    vv = _np(d.velocities)
    for a, b in zip(ptr[:-1], ptr[1:]):
        assert np.abs((m[a:b, None] * vv[a:b]).sum(0)).max() <= 1e-5 * m[a:b].sum() * np.abs(vv[a:b]).max()
    assert bool((d.kinetic_energy <= ke * (1 + 1e-6)).all())
    d.set_velocities(seen)
    assert torch.equal(d.velocities, seen) and torch.allclose(d.kinetic_energy, ke, rtol=1e-5)
    d.maxwell_boltzmann(T_K)
    assert bool((d.thermo[:, no.SCALE] == 1.0).all()) and torch.equal(d.velocities, d.vel)
    other = _dynamics("ragged", "berendsen", torch.float32)
    for prop in ("thermostat_energy", "conserved_energy"):
        with pytest.raises(AttributeError, match="keeps no thermostat energy"):
            getattr(other, prop)
    with pytest.raises(ValueError, match="zero low word"):
        _dynamics("ragged", "bussi", torch.float32, graph_rng_id=np.arange(len(ptr) - 1, dtype=np.int64))


# ------------------------------------------------------------------------------------------------------------------ 6. residency
@pytest.mark.parametrize("ensemble", ENSEMBLES)
@pytest.mark.parametrize("name", ["qm9 seed 9", "water box"])
def test_run_does_not_touch_the_host_between_checks(name, ensemble):
    from xequinet_amd import lib

    d = _dynamics(name, ensemble, torch.float32)
    d.run(4, check_every=4)                                   # warm: captured, capacity settled
    captures = d.step.captures
    torch.cuda.synchronize()
    former = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        n0 = lib.launch_count()
        d.run(32, check_every=32)                             # (the one read-back lifts the guard for exactly its own call)
        names = [n for n in lib.launch_names(n0) if n.startswith("xeq_nvt") or n.startswith("xeq_md_")]
    finally:
        torch.cuda.set_sync_debug_mode(former)
    assert d.step_count == 36 and d.step.captures == captures
    assert names.count("xeq_nvt_front") == 32 and "xeq_nvt_back" in names and not [n for n in names if n.startswith("xeq_md_")]
    assert bool(torch.isfinite(d.kinetic_energy).all()) and bool(torch.isfinite(d.thermostat_energy).all())
