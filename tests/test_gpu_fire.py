"""Device-resident batched FIRE (xequinet_amd/optimize.py, csrc/xeq_md.hip) on the MI355X against the host restatement and minimiser of
tests/fire_oracle.py.  Model: hessian_cases.model_case("well"); systems "ragged", "qm9 seed 9", "water box"; the defaults of ASE's FIRE and
fmax = 0.05.

Tolerances of the kernels alone are those of tests/test_gpu_md.py for xeq_md_back alone (``_ulp_ok``: f32 state within 2 ulp of the f64
evaluation rounded to f32, f64 and the double per-graph state within 1e-14 relative).  That fits the sums here because every compared sum
is well conditioned by construction: ff and vv have positive terms only, and P is either exactly 0 (v = 0), or of graphs with
v = +-0.1 f (+ 1 % noise), so sum |terms| / |sum| < 1.05 and a tree sum of 1 537 terms is within ~12 eps = 1.3e-15 of numpy's.
The decisions of the whole runs are safe from a rounding for the same reason: over the 30 compared iterations |P| / sqrt(ff vv) of every
active graph is above 0.0136 on the f64 oracle (asserted below against 1e-6).

Measured on the MI355X (the f32 and f64 tests add their figures to tests/parity_record.py):
  f64 runs, 30 iterations: largest error / largest magnitude 1.7e-15 (ragged, energy; bound 1e-9); dt, n_pos, status, converged_at equal
  f32 runs to convergence at fmax = 0.05: converged at evaluations 127 / 0 / 0 / 12 (ragged), 93 / 79 (qm9 seed 9), 106 (water box) -- the
  f64 host minimiser's own; the f64 oracle's fmax at the device's final positions 0.04755 / 0.04798 / 0.04603 against bounds of
  0.05 + 4 x (2.7e-6, 9.3e-7, 1.5e-6)
"""
import copy
import ctypes

import numpy as np
import pytest
import torch

from tests import fire_oracle as fo
from tests import guard_bands as gb
from tests import hessian_cases as hc
from tests import md_oracle as mo
from tests import parity_record

pytestmark = pytest.mark.gpu
DEV = "cuda"
FMAX = 0.05
N_ITER = 30
SYSTEMS = ["ragged", "qm9 seed 9", "water box"]
PAR = dict(fo.DEFAULTS)


def _t(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def _np(t):
    return t.detach().double().cpu().numpy()


_MODELS = {}


def _model(dtype):
    if dtype not in _MODELS:
        _MODELS[dtype] = copy.deepcopy(hc.model_case("well")[0]).to(device=DEV, dtype=dtype).eval().requires_grad_(False)
    return _MODELS[dtype]


def _fire(name, dtype, pos=None, sel=None, **extra):
    from xequinet_amd import optimize

    p, z, ptr, cell = fo.case(name)
    p = p if pos is None else pos
    if sel is not None:             # one graph of the batch, alone
        a, b = int(ptr[sel]), int(ptr[sel + 1])
        p, z, ptr = p[a:b], z[a:b], np.array([0, b - a])
    kw = dict(fmax=FMAX, energy_unit="eV", length_unit="Angstrom")
    kw.update(extra)
    if cell is not None:
        kw["cell"] = _t(cell, dtype)
    else:
        kw["ptr"] = _t(ptr)
    return optimize.FIRE(_model(dtype), _t(p, dtype), _t(z), **kw)


def _state(o):
    return {"pos": o.unwrapped_positions, "wrapped": o.positions, "image": o.image.clone(), "vel": o.vel.clone(), "frc": o.forces, "epot": o.potential_energy,
            "fmax": o.max_force, "dt": o.time_steps, "alpha": o.alpha.clone(), "n_pos": o.n_pos.clone(), "status": o.status.clone(),
            "converged_at": o.converged_at, "coef": o.coef.clone()}


def _ulp_ok(got, ref, dtype, n_ulp=2):
    """tests/test_gpu_md.py::_ulp_ok."""
    if dtype == np.float32:
        return np.all(np.abs(got.astype(np.float64) - ref.astype(np.float64)) <= n_ulp * np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64))
    return np.all(np.abs(got - ref) <= 1e-14 * np.abs(ref))


# ------------------------------------------------------------------------------------------------------------------ 1. kernels alone
def _zoo(n, dtype, seed):
    """One batch that meets every state of the machine: (ptr, state, v, f, fixed, energy, names).  ``n``: the size of the graph "big"."""
    rng = np.random.default_rng(seed)
    graphs = []

    def add(name, m, status, v_of_f, fscale=0.3, dt=0.1, alpha=0.1, n_pos=0, fix=(), **more):
        f = fscale * rng.standard_normal((m, 3))
        v = v_of_f(f) if m else np.zeros((0, 3))
        fixed = np.zeros(m, bool)
        for i in fix:
            fixed[i], v[i], f[i] = True, 0.0, 40.0          # a fixed atom holds no velocity; its (large) force must reach no sum
        graphs.append(dict(name=name, m=m, status=status, v=v, f=f, fixed=fixed, dt=dt, alpha=alpha, n_pos=n_pos, **more))

    along = lambda c: (lambda f: c * f * (1.0 + 0.01 * rng.standard_normal(f.shape)))
    zero = lambda f: np.zeros_like(f)
    add("fresh", 5, fo.FRESH, zero)
    add("up, n_pos <= n_min", 6, fo.ACTIVE, along(0.1), n_pos=2, dt=0.2, alpha=0.08)
    add("up, n_pos > n_min", 5, fo.ACTIVE, along(0.1), n_pos=7, dt=0.3, alpha=0.07)
    add("up, dt hits dtmax", 4, fo.ACTIVE, along(0.1), n_pos=9, dt=0.95, alpha=0.05)
    add("down", 7, fo.ACTIVE, along(-0.1), n_pos=4, dt=0.4, alpha=0.06)
    add("P = 0, v = 0", 3, fo.ACTIVE, zero, n_pos=3, dt=0.2, alpha=0.09)
    add("big", n, fo.ACTIVE, along(0.1), n_pos=8, dt=0.25, alpha=0.07)
    add("clamp", 5, fo.ACTIVE, lambda f: 0.1 * f, fscale=15.0, n_pos=1, dt=0.5)
    add("converged before", 6, fo.CONVERGED, along(0.1), n_pos=5, dt=0.37, alpha=0.033, converged_at=3, epot=-1.25, fmax=0.031, coef=(0.9, 0.4, 0.37))
    add("newly converged", 5, fo.ACTIVE, along(0.1), fscale=1e-3, n_pos=6, dt=0.6)
    add("fixed atoms", 8, fo.ACTIVE, along(0.1), n_pos=6, dt=0.3, fix=(0, 5))
    add("empty", 0, fo.ACTIVE, zero)
    add("lone atom, ff = 0", 1, fo.ACTIVE, zero, fscale=0.0, n_pos=2)
    add("two chunks", 300, fo.ACTIVE, along(-0.1), n_pos=6, dt=0.3)
    G = len(graphs)
    ptr = np.concatenate([[0], np.cumsum([g["m"] for g in graphs])])
    st = fo.new_state(G, 0.1, 0.1)
    for i, g in enumerate(graphs):
        st["dt"][i], st["alpha"][i], st["n_pos"][i], st["status"][i] = g["dt"], g["alpha"], g["n_pos"], g["status"]
        st["converged_at"][i] = g.get("converged_at", -1)
        st["epot"][i], st["fmax"][i], st["coef"][i] = dtype(g.get("epot", 0.0)), dtype(g.get("fmax", 0.0)), g.get("coef", (0.0, 0.0, 0.0))
    cat = lambda k: np.concatenate([g[k] for g in graphs])
    energy = np.linspace(-3.0, 2.0, G).astype(dtype)
    return ptr, st, cat("v").astype(dtype), cat("f").astype(dtype), cat("fixed"), energy, [g["name"] for g in graphs]


def _device_state(st, tdt):
    return {"epot": _t(st["epot"], tdt), "fmax": _t(st["fmax"], tdt), "dt": _t(st["dt"]), "alpha": _t(st["alpha"]), "n_pos": _t(st["n_pos"]),
            "status": _t(st["status"]), "converged_at": _t(st["converged_at"]), "coef": _t(st["coef"])}


def _back_call(dtype, ptr, st, v, f_step, fixed, energy, n_edges, book, frc0=None):
    from xequinet_amd import lib, resident

    n, G = len(v), len(ptr) - 1
    a0, cn, gp = resident.chunk_tables(ptr)
    C = len(a0)
    code = 0 if dtype == np.float32 else 1
    tdt = torch.float32 if dtype == np.float32 else torch.float64
    batch = np.repeat(np.arange(G), np.diff(ptr)).astype(np.int64)
    frc0 = np.full((n, 3), 7.0, dtype) if frc0 is None else frc0
    g = {"pos": _t(np.zeros((n, 3), dtype)), "v": _t(v), "frc": _t(frc0), "fs": _t(f_step), "en": _t(energy), "ne": _t(np.array([n_edges], np.int32)),
         "fixed": _t(fixed.astype(np.uint8)), "batch": _t(batch), "a0": _t(a0), "cn": _t(cn), "gp": _t(gp),
         "partial": torch.zeros((max(C, 1), 4), dtype=torch.float64, device=DEV), "pbad": torch.zeros(max(C, 1), dtype=torch.int32, device=DEV),
         "book": _t(book), **_device_state(st, tdt)}
    g = {k: gb.guarded_copy(t) for k, t in g.items()}
    system = lib.fill(lib.ResSystem(), dtype=code, n=n, n_graphs=G, n_chunks=C, pos=g["pos"], vel=g["v"], frc=g["frc"], batch=g["batch"], book=g["book"])
    step = lib.fill(lib.ResStep(), frc_step=g["fs"], energy_step=g["en"], n_edges_step=g["ne"])
    chunks = lib.fill(lib.ResChunks(), chunk_atom0=g["a0"], chunk_n=g["cn"], graph_chunk_ptr=g["gp"], partial=g["partial"], partial_bad=g["pbad"])
    par = lib.fill(lib.FireParams(), fixed=g["fixed"], epot=g["epot"], fmax=g["fmax"], dt=g["dt"], alpha=g["alpha"], n_pos=g["n_pos"], status=g["status"],
                   converged_at=g["converged_at"], coef=g["coef"], fmax_tol=FMAX, maxstep=PAR["maxstep"], dtmax=PAR["dtmax"], n_min=PAR["n_min"],
                   f_inc=PAR["f_inc"], f_dec=PAR["f_dec"], alpha_start=PAR["alpha_start"], f_alpha=PAR["f_alpha"])
    lib.call("xeq_fire_back", ctypes.byref(system), ctypes.byref(step), ctypes.byref(chunks), ctypes.byref(par), None, lib.stream())
    torch.cuda.synchronize()
    gb.check(*g.values())
    return {k: t.cpu().numpy() for k, t in g.items()}


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("n", [1, 63, 65, 1537])
def test_back_kernel_alone(n, dtype):
    ptr, st, v, f, fixed, energy, names = _zoo(n, dtype, 400 + n)
    G = len(ptr) - 1
    frc0 = np.full((len(v), 3), 7.0, dtype)
    got = _back_call(dtype, ptr, st, v, f, fixed, energy, 777, np.array([41, 500, 0, 0], np.int64), frc0)
    ref, frc_ref, sums = fo.back(st, v, f, frc0, energy, fixed, ptr, 41, fmax_tol=FMAX, dtype=dtype, **PAR)
    ix = {name: i for i, name in enumerate(names)}
    # the call met the states it was built for
    assert st["status"][ix["fresh"]] == fo.FRESH and ref["status"][ix["fresh"]] == fo.ACTIVE and ref["coef"][ix["fresh"], 0] == 0.0
    assert ref["n_pos"][ix["up, n_pos <= n_min"]] == 3 and ref["dt"][ix["up, n_pos <= n_min"]] == 0.2
    assert ref["n_pos"][ix["up, n_pos > n_min"]] == 8 and ref["dt"][ix["up, n_pos > n_min"]] == 0.3 * 1.1
    assert ref["dt"][ix["up, dt hits dtmax"]] == 1.0
    assert ref["n_pos"][ix["down"]] == 0 and ref["dt"][ix["down"]] == 0.2 and sums["P"][ix["down"]] < 0
    assert sums["P"][ix["P = 0, v = 0"]] == 0.0 and ref["n_pos"][ix["P = 0, v = 0"]] == 0 and ref["dt"][ix["P = 0, v = 0"]] == 0.1
    assert ref["coef"][ix["clamp"], 2] < ref["dt"][ix["clamp"]] and ref["coef"][ix["up, n_pos <= n_min"], 2] == ref["dt"][ix["up, n_pos <= n_min"]]
    for name in ("newly converged", "empty", "lone atom, ff = 0"):
        assert st["status"][ix[name]] == fo.ACTIVE and ref["status"][ix[name]] == fo.CONVERGED and ref["converged_at"][ix[name]] == 41, name
    assert ref["status"][ix["fixed atoms"]] == fo.ACTIVE and sums["m2"][ix["fixed atoms"]] < 100.0
    # integer state, dt and alpha: exactly (every decision here is unambiguous)
    for k in ("n_pos", "status", "converged_at", "dt", "alpha"):
        assert np.array_equal(got[k], ref[k]), (k, got[k], ref[k])
    assert _ulp_ok(got["coef"], ref["coef"], np.float64), np.abs(got["coef"] - ref["coef"]).max()
    assert _ulp_ok(got["fmax"], ref["fmax"].astype(dtype), dtype) and np.array_equal(got["epot"], ref["epot"].astype(dtype))
    assert np.array_equal(got["frc"], frc_ref)
    # the converged graph: every bit of its state, its force rows included
    c = ix["converged before"]
    for k in ("epot", "fmax", "dt", "alpha", "n_pos", "status", "converged_at", "coef"):
        assert np.array_equal(got[k][c], np.asarray(st[k][c]).astype(got[k].dtype)), k
    assert np.array_equal(got["frc"][ptr[c]:ptr[c + 1]], frc0[ptr[c]:ptr[c + 1]])
    assert np.array_equal(got["frc"][fixed], np.zeros((int(fixed.sum()), 3), dtype))
    assert got["book"].tolist() == [42, 777, 0, int((ref["status"] != fo.CONVERGED).sum())]
    for k, a in (("v", v), ("fs", f), ("en", energy)):                                    # inputs are inputs
        assert np.array_equal(got[k], a), k
    # a non-finite force of an active graph raises the flag; a smaller edge count leaves the maximum
    bad = f.copy()
    bad[ptr[ix["down"]] + 1, 1] = np.nan
    got = _back_call(dtype, ptr, st, v, bad, fixed, energy, 3, np.array([0, 500, 0, 0], np.int64))
    assert got["book"].tolist()[:3] == [1, 500, 1]


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("n", [1, 63, 65, 1537])
def test_front_kernel_alone(n, dtype):
    from xequinet_amd import lib

    tdt = torch.float32 if dtype == np.float32 else torch.float64
    code = 0 if dtype == np.float32 else 1
    ptr, st, v, f, fixed, energy, names = _zoo(n, dtype, 500 + n)
    G, N = len(ptr) - 1, len(v)
    rng = np.random.default_rng(600 + n)
    st["coef"] = np.stack([rng.uniform(0.0, 1.0, G), rng.uniform(0.1, 1.5, G), rng.uniform(0.5, 4.0, G)], axis=1)     # d large: atoms leave the box
    cell = np.array([[7.3, 0.0, 0.0], [0.9, 6.1, 0.0], [-0.5, 0.8, 8.2]]).astype(dtype).astype(np.float64)
    x = (rng.uniform(0.02, 0.98, (N, 3)) @ cell).astype(dtype)
    v = (v.astype(np.float64) * 5.0).astype(dtype)
    frc = np.where(fixed[:, None], 0.0, f).astype(dtype)
    batch = np.repeat(np.arange(G), np.diff(ptr)).astype(np.int64)
    still = fixed | np.isin(st["status"], (fo.CONVERGED, fo.FRESH))[batch]
    assert still.any() and (~still).any()
    for periodic in (None, [True, True, True], [True, False, True]):
        xr, vr, ir = fo.front(st, x, v, frc, np.zeros((N, 3), np.int32), fixed, ptr, cell if periodic else None, periodic, dtype)
        g = {k: gb.guarded_copy(_t(a)) for k, a in dict(x=x, v=v, f=frc, fixed=fixed.astype(np.uint8), batch=batch, status=st["status"], coef=st["coef"],
                                                        image=np.zeros((N, 3), np.int32)).items()}
        cell_c = (ctypes.c_double * 9)(*cell.reshape(-1)) if periodic else None
        pbc_c = (ctypes.c_int32 * 3)(*[int(b) for b in periodic]) if periodic else None
        system = lib.fill(lib.ResSystem(), dtype=code, n=N, n_graphs=G, pos=g["x"], vel=g["v"], frc=g["f"], image=g["image"], batch=g["batch"], cell=cell_c,
                          pbc=pbc_c)
        lib.call("xeq_fire_front", ctypes.byref(system), ctypes.byref(lib.fill(lib.FireParams(), fixed=g["fixed"], status=g["status"], coef=g["coef"])),
                 lib.stream())
        torch.cuda.synchronize()
        gb.check(*g.values())
        xg, vg, ig = g["x"].cpu().numpy(), g["v"].cpu().numpy(), g["image"].cpu().numpy()
        assert np.array_equal(ig, ir), periodic
        assert _ulp_ok(vg, vr, dtype) and _ulp_ok(xg, xr, dtype), periodic
        assert np.array_equal(xg[still], x[still]) and np.array_equal(vg[still], v[still]) and not ig[still].any(), periodic      # bit-unchanged rows
        assert not np.array_equal(xg[~still], x[~still])
        for k, a in (("f", frc), ("status", st["status"]), ("coef", st["coef"]), ("batch", batch)):
            assert np.array_equal(g[k].cpu().numpy(), a), k
        if periodic:
            assert np.abs(ig).max() > 0, periodic                                          # somebody was carried through a face
            fr = xg[~still].astype(np.float64) @ mo.inverse_cell(cell)
            per = np.array(periodic)
            assert np.all((fr[:, per] >= -1e-6) & (fr[:, per] < 1 + 1e-6)), periodic


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("na", [65, 1537])
def test_a_graphs_sums_and_state_have_the_same_bits_anywhere(na, dtype):
    rng = np.random.default_rng(700 + na)

    def part(m, n_pos, dt):
        f = (0.3 * rng.standard_normal((m, 3))).astype(dtype)
        return dict(v=(0.1 * f * (1.0 + 0.01 * rng.standard_normal((m, 3)))).astype(dtype), f=f, n_pos=n_pos, dt=dt)

    parts = {"a": part(na, 8, 0.25), "b": part(300, 2, 0.4)}

    def run(order):
        ptr = np.concatenate([[0], np.cumsum([len(parts[k]["v"]) for k in order])])
        st = fo.new_state(len(order), 0.1, 0.1)
        st["status"][:] = fo.ACTIVE
        for i, k in enumerate(order):
            st["n_pos"][i], st["dt"][i] = parts[k]["n_pos"], parts[k]["dt"]
        v, f = (np.concatenate([parts[k][q] for k in order]) for q in "vf")
        got = _back_call(dtype, ptr, st, v, f, np.zeros(len(v), bool), np.zeros(len(order), dtype), 1, np.zeros(4, np.int64))
        i = order.index("a")
        return b"".join(got[k][i].tobytes() for k in ("epot", "fmax", "dt", "alpha", "n_pos", "status", "converged_at", "coef")), got["coef"][i]

    alone, front, back = run("a"), run("ab"), run("ba")
    assert alone[1][1] > 0 and alone[0] == front[0] == back[0]


# ------------------------------------------------------------------------------------------------------------------ 2. whole runs
@pytest.mark.parametrize("name", SYSTEMS)
def test_f64_trajectory_against_the_host_minimiser(name):
    ref = fo.host_run(name, np.float64, N_ITER, FMAX)
    events = 0
    for it in range(N_ITER + 1):                      # the condition the comparison of decisions rests on, and that the run has the events
        for g in range(len(ref["P"][it])):
            if ref["was"][it][g] == fo.ACTIVE and ref["status"][it][g] == fo.ACTIVE:
                assert abs(ref["P"][it][g]) / np.sqrt(ref["ff"][it][g] * ref["vv"][it][g]) > 1e-6, (it, g)
                events += ref["P"][it][g] <= 0.0
    assert events >= 1
    if name == "ragged":
        assert ref["converged_at"].tolist() == [-1, 0, 0, 12] and any(ref["P"][it][g] <= 0 and ref["was"][it][g] == fo.ACTIVE for it in range(13) for g in (0, 3))
    o = _fire(name, torch.float64)
    assert o.run(N_ITER, check_every=N_ITER) is False and o.step_count == N_ITER
    got = _state(o)
    for k, want in (("pos", ref["pos"][-1]), ("epot", ref["epot"][-1])):
        err, scale = np.abs(_np(got[k]) - want).max(), np.abs(want).max()
        print(f"fire parity: f64 {name} {k}: max abs error {err:.3e}, largest {scale:.3e}")
        parity_record.add({"test": "fire_f64_trajectory", "system": name, "quantity": k, "max_abs_err": float(err), "scale": float(scale)})
        assert err <= 1e-9 * scale, (k, err, scale)
    st = ref["state"]
    assert np.array_equal(got["dt"].cpu().numpy(), st["dt"]) and np.array_equal(got["n_pos"].cpu().numpy(), st["n_pos"])
    assert np.array_equal(got["status"].cpu().numpy(), st["status"]) and np.array_equal(got["converged_at"].cpu().numpy(), st["converged_at"])
    if name == "water box":
        assert np.array_equal(got["image"].cpu().numpy(), ref["image"])


def _converged_run(name):
    """The f32 run to convergence, recorded at every iteration: shared by the tests below (and left unchanged by them)."""
    def make():
        o = _fire(name, torch.float32)
        e0 = o.potential_energy
        x0 = o.unwrapped_positions
        done = o.run(400, check_every=20, record_every=1)
        return o, e0, x0, done

    return hc.cached(("fire f32 run", name), make)


@pytest.mark.parametrize("name", SYSTEMS)
def test_f32_runs_converge(name):
    """The f64 oracle's fmax at the device's final positions against 0.05 + 4 x the f32 oracle's own force error there (the project's 4 x
    rule against the reference's own f32 error).  A graph that converged at evaluation 0 never moved: its final energy IS the starting one,
    every other graph's is below."""
    o, e0, x0, done = _converged_run(name)
    assert done is True and bool(o.converged.all())
    p, z, ptr, cell = fo.case(name)
    x = _np(o.positions)
    sd = hc.model_case("well")[1]
    _, f64 = mo.evaluate(sd, x, z, ptr, cell, [True] * 3 if cell is not None else None, torch.float64)
    _, f32 = mo.evaluate(sd, x, z, ptr, cell, [True] * 3 if cell is not None else None, torch.float32)
    own = float(np.abs(f32 - f64).max())
    fm = np.array([np.sqrt((f64[a:b] ** 2).sum(1).max()) if b > a else 0.0 for a, b in zip(ptr[:-1], ptr[1:])])
    at = o.converged_at.cpu().numpy()
    print(f"fire parity: f32 {name}: converged at {at.tolist()}, f64-oracle fmax {fm.max():.5f}, f32 oracle's own force error {own:.3e}, "
          f"bound {FMAX + 4 * own:.5f}; device fmax {_np(o.max_force).max():.5f}")
    parity_record.add({"test": "fire_f32_converged", "system": name, "converged_at": at.tolist(), "oracle_fmax": float(fm.max()), "f32_oracle_force_err": own,
                       "bound": FMAX + 4 * own, "device_fmax": float(_np(o.max_force).max())})
    assert np.all(fm < FMAX + 4 * own), (fm, own)
    e1, e0 = _np(o.potential_energy), _np(e0)
    moved = at > 0
    assert np.all(e1[moved] < e0[moved]) and np.array_equal(e1[~moved], e0[~moved]), (e0, e1)
    assert int(at.max()) <= o.step_count <= 400


def test_converged_graphs_are_frozen_while_the_others_run_on():
    o, e0, x0, _ = _converged_run("ragged")
    ptr = fo.case("ragged")[2]
    at = o.converged_at.cpu().tolist()
    assert at[1] == 0 and at[2] == 0 and 0 < at[3] < at[0]
    rows = o.trajectory["pos"]                                   # row r: behind evaluation r + 1
    steps = o.trajectory["step"].cpu().tolist()
    assert steps[: o.step_count] == list(range(1, o.step_count + 1))
    last = at[0] - 1
    for r in range(last + 1):
        assert torch.equal(rows[r, ptr[1]:ptr[3]], x0[ptr[1]:ptr[3]]), r
        if r >= at[3] - 1:
            assert torch.equal(rows[r, ptr[3]:], rows[at[3] - 1, ptr[3]:]), r
    assert not torch.equal(rows[at[3] - 1, ptr[3]:], x0[ptr[3]:]) and not torch.equal(rows[last, : ptr[1]], rows[at[3] - 1, : ptr[1]])
    assert torch.equal(rows[last], o.unwrapped_positions)


def test_batch_members_repeat_bit_for_bit():
    o, _, _, _ = _converged_run("qm9 seed 9")
    twin = _fire("qm9 seed 9", torch.float32)
    assert twin.run(400, check_every=7) is True                  # another window length: the same states
    ptr = fo.case("qm9 seed 9")[2]
    assert torch.equal(twin.positions, o.positions) and torch.equal(twin.converged_at, o.converged_at)
    for g in range(len(ptr) - 1):
        lo, hi = int(ptr[g]), int(ptr[g + 1])
        alone = _fire("qm9 seed 9", torch.float32, sel=g)
        assert alone.run(400, check_every=20, record_every=1) is True
        n = alone.step_count
        assert torch.equal(alone.converged_at[0], o.converged_at[g]) and n >= int(o.converged_at[g])
        assert torch.equal(alone.trajectory["pos"][:n], o.trajectory["pos"][:n, lo:hi]), g
        assert torch.equal(alone.trajectory["epot"][:n, 0], o.trajectory["epot"][:n, g]) and torch.equal(alone.trajectory["fmax"][:n, 0], o.trajectory["fmax"][:n, g])
        assert torch.equal(alone.positions, o.positions[lo:hi]) and torch.equal(alone.time_steps[0], o.time_steps[g])


# ------------------------------------------------------------------------------------------------------------------ 3. residency
@pytest.mark.parametrize("name,per_iteration", [("qm9 seed 9", 3), ("water box", 2)])
def test_run_does_not_touch_the_host_between_checks(name, per_iteration):
    from xequinet_amd import lib

    o = _fire(name, torch.float32)
    o.run(4, check_every=4)                                   # warm: captured, capacity settled
    captures = o.step.captures
    torch.cuda.synchronize()
    former = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    n0 = lib.launch_count()
    try:
        o.run(32, check_every=32)                             # (the one read-back lifts the guard for exactly its own call: ResidentDriver._read_book)
    finally:
        torch.cuda.set_sync_debug_mode(former)
    names = [n for n in lib.launch_names(n0) if n.startswith("xeq_fire")]
    assert names.count("xeq_fire_front") == 32 and names.count("xeq_fire_back") == 32 * (per_iteration - 1)
    assert o.step_count == 36 and o.step.captures == captures
    assert bool(torch.isfinite(o.potential_energy).all())


# ------------------------------------------------------------------------------------------------------------------ 4. capacity / restore
def test_a_list_that_outgrows_its_capacity_is_rerun_bit_for_bit():
    roomy = _fire("water box", torch.float32)
    small = _fire("water box", torch.float32, edge_capacity=64)       # the first evaluation's list has 1 286 edges
    assert small.edge_capacity == 64
    small.run(12, check_every=4)
    roomy.run(12, check_every=4)
    assert small.step_count == 12 and small.edge_capacity >= 1286 and roomy.edge_capacity >= 1286
    a, b = _state(small), _state(roomy)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_open_boundaries_with_a_too_small_explicit_capacity_raise_with_the_count():
    o = _fire("qm9 seed 9", torch.float32, edge_capacity=16)
    with pytest.raises(ValueError) as e:
        o.run(2)
    roomy = _fire("qm9 seed 9", torch.float32)
    roomy.run(0)
    count = int(roomy.step.outputs["n_edges"].item())
    assert count > 16 and str(count) in str(e.value) and "16" in str(e.value) and "FIRE" in str(e.value)


def test_a_raised_non_finite_flag_leaves_the_checked_state():
    """The flag itself is the back kernel's (test_back_kernel_alone); here the driver's answer to it: checkpoint back, then the error."""
    o = _fire("qm9 seed 9", torch.float32)
    o.run(2)
    before = _state(o)
    real = o._read_book
    o._read_book = lambda: real()[:2] + (True,)
    with pytest.raises(FloatingPointError, match="evaluations 3 .. 6"):
        o.run(3)
    o._read_book = real
    assert o.step_count == 2 and o.book.cpu().tolist()[:3] == [3, 0, 0]
    after = _state(o)
    for k in before:
        assert torch.equal(before[k], after[k]), k
    o.run(3)
    assert o.step_count == 5


# ------------------------------------------------------------------------------------------------------------------ 5. recorder, reset
@pytest.mark.parametrize("name", ["ragged", "water box"])
def test_recorder_rows_are_the_states_of_a_twin(name):
    a, b = _fire(name, torch.float32), _fire(name, torch.float32)
    a.run(6, check_every=4, record_every=2)
    t = a.trajectory
    assert t["step"].cpu().tolist() == [2, 4, 6] and t["pos"].shape == (3, a.n_atoms, 3) and t["epot"].shape == (3, a.n_graphs)
    for row in range(3):
        b.run(2)
        assert torch.equal(t["pos"][row], b.unwrapped_positions) and torch.equal(t["epot"][row], b.potential_energy)
        assert torch.equal(t["fmax"][row], b.max_force)
    a.run(3)                       # a run without a recorder keeps none
    assert a.trajectory == {} and a.step_count == 9


@pytest.mark.parametrize("name", ["qm9 seed 9", "water box"])
def test_reset_then_run_repeats_a_first_run_from_the_same_positions(name):
    a = _fire(name, torch.float32)
    a.run(7, check_every=3)
    start = _np(a.positions)
    a.reset()
    assert a.step_count == 0 and a.converged_at.cpu().tolist() == [-1] * a.n_graphs and not bool(a.vel.any())
    b = _fire(name, torch.float32, pos=start)
    a.run(9, check_every=4)
    b.run(9, check_every=4)
    sa, sb = _state(a), _state(b)
    for k in sa:
        if k not in ("pos", "image"):          # (the first object carries the image counts of its first run)
            assert torch.equal(sa[k], sb[k]), k
    assert a.step_count == 9
