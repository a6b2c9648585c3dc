"""Device-resident batched L-BFGS (xequinet_amd/optimize.py: LBFGS, csrc/xeq_lbfgs.hip) on the MI355X against the host restatement and
minimiser of tests/lbfgs_oracle.py.  Model: hessian_cases.model_case("well"); systems "ragged", "qm9 seed 9", "water box"; ASE's
alpha = 70 and maxstep = 0.2, fmax = 0.05.

Bounds of the kernels alone.
  Gram entries: |B_dev - B_ref| <= 32 eps64 sum |terms| with B_ref by math.fsum.  A tree or sequential sum of n <= 4611 products is within
  (ceil(log2 n) + 2) eps = 15 eps of the exact one relative to sum |terms|; 32 leaves room for any order.  Every input is double, so the
  bound is the same for both dtypes.
  delta: the oracle is fed the device's own B; ``own`` is the oracle's deviation between the stated order of the row products and the
  reversed one on that B (the reference's own rounding, measured on the CPU); the bound is 8 x own + 4 eps64 max |delta| (the 8 x rule of
  tests/test_gpu_hessian.py).  Fresh graphs must be exact.
  New positions: the oracle is fed the device's delta; ``_ulp_ok`` of tests/test_gpu_fire.py (2 ulp in f32, 1e-14 relative in f64).
  The pending s, the images, the ring rows and every integer must be equal.

The whole f64 runs are compared over 12 iterations with memory 4; the decisions they rest on (a pair's sign, the clamp, fmax against the
tolerance) are asserted to be clear of their thresholds by 1e-6 on the oracle's run (also on the CPU: tests/test_lbfgs_host.py).

The f32 runs to convergence use the criterion of test_gpu_fire.py::test_f32_runs_converge on all three systems.  One graph is exempt from
one clause, "the energy of every graph that moved went down": the bonded pair of "ragged" (graph 3).  The rule has no line search and so
no descent guarantee, and the f64 HOST minimiser itself leaves that pair 1.4e-3 above its start (0.1035 -> 0.1049, converged at
evaluation 15 with 5 rejected pairs); the test asserts exactly that on the oracle's own run before it exempts the graph, and holds the
graph to the fmax bound like every other.

Measured on the MI355X (the tests add their figures to tests/parity_record.py):
  kernels alone, every n, form, memory and dtype: refreshed Gram entries at most 0.034 of their bound; delta equal to the oracle's on the device's
  own B (error 0; the oracle's own order sensitivity is at most 1.3e-15)
  f64 runs, 12 iterations, memory 4: largest error / largest magnitude 1.2e-14 (qm9 seed 9, energy; bound 1e-9); integers equal
  f32 runs to convergence at fmax = 0.05: converged at evaluations 118 / 0 / 0 / 15 (ragged), 73 / 104 (qm9 seed 9) and 187 (water box);
  the f64 oracle's fmax at the device's final positions 0.04522 / 0.04717 / 0.04705 against bounds of 0.05 + 4 x (1.0e-6, 1.1e-6, 8.4e-7)
"""
import copy
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import fire_oracle as fo
from tests import guard_bands as gb
from tests import hessian_cases as hc
from tests import lbfgs_oracle as lo
from tests import md_oracle as mo
from tests import parity_record

pytestmark = pytest.mark.gpu
DEV = "cuda"
FMAX = 0.05
ALPHA, MAXSTEP, DAMPING = 70.0, 0.2, 1.0
EPS = np.finfo(np.float64).eps
SYSTEMS = ["ragged", "qm9 seed 9", "water box"]
CELL = np.array([[4.0, 0.0, 0.0], [0.3, 4.2, 0.0], [0.1, -0.2, 3.9]])


def _t(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def _np(t):
    return t.detach().double().cpu().numpy()


_MODELS = {}


def _model(dtype):
    if dtype not in _MODELS:
        _MODELS[dtype] = copy.deepcopy(hc.model_case("well")[0]).to(device=DEV, dtype=dtype).eval().requires_grad_(False)
    return _MODELS[dtype]


def _lbfgs(name, dtype, pos=None, sel=None, **extra):
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
    return optimize.LBFGS(_model(dtype), _t(p, dtype), _t(z), **kw)


def _state(o):
    return {"pos": o.unwrapped_positions, "wrapped": o.positions, "image": o.image.clone(), "frc": o.forces, "epot": o.potential_energy,
            "fmax": o.max_force, "hist_s": o.hist_s.clone(), "hist_y": o.hist_y.clone(), "pending": o.pending_s.clone(), "gram": o.gram.clone(),
            "delta": o.delta.clone(), "count": o.history_length, "head": o.head.clone(), "status": o.status.clone(),
            "dropped": o.dropped_pairs, "converged_at": o.converged_at}


def _ulp_ok(got, ref, dtype, n_ulp=2):
    """tests/test_gpu_fire.py::_ulp_ok."""
    if dtype == np.float32:
        return np.all(np.abs(got.astype(np.float64) - ref.astype(np.float64)) <= n_ulp * np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64))
    return np.all(np.abs(got - ref) <= 1e-14 * np.abs(ref))


# ------------------------------------------------------------------------------------------------------------------ 1. kernels alone
PER_GRAPH = ("gram", "delta", "count", "head", "status", "dropped", "converged_at", "epot", "fmax")
PER_ATOM = ("pos", "frc", "pending", "image")


def _graph(rng, m_atoms, memory, dtype, status=lo.ACTIVE, count=0, head=None, pair="accepted", fscale=0.3, fix=(), **more):
    """One graph's buffers: a ring of ``count`` pairs y = a s (a > 0 per coordinate: SPD), the pending s, f_prev and the step's force
    f = f_prev - y_new with y_new = +a s (accepted) or -a s (rejected)."""
    a = rng.uniform(0.5, 2.0, (m_atoms, 3))
    S = np.zeros((memory, m_atoms, 3))
    Y = np.zeros((memory, m_atoms, 3))
    S[:count] = 0.05 * rng.standard_normal((count, m_atoms, 3))
    Y[:count] = a * S[:count]
    pending = 0.05 * rng.standard_normal((m_atoms, 3))
    fixed = np.zeros(m_atoms, bool)
    f_prev = (fscale * rng.standard_normal((m_atoms, 3))).astype(dtype)
    f = (f_prev.astype(np.float64) - (a * pending if pair == "accepted" else -a * pending)).astype(dtype)
    for i in fix:
        fixed[i], pending[i], f[i], f_prev[i] = True, 0.0, 40.0, 0.0          # its (large) force must reach no sum
        S[:, i], Y[:, i] = 0.0, 0.0
    K = 2 * memory + 1
    b = np.concatenate([S, Y, -f_prev.astype(np.float64)[None]]).reshape(K, -1)
    on = lo.live(count, memory)
    gram = np.where(on[:, None] & on[None, :], b @ b.T, 0.0)
    head = (count % memory) if head is None else head
    return dict(m=m_atoms, S=S, Y=Y, pending=pending, fixed=fixed, f_prev=f_prev, f=f, gram=gram, status=status, count=count, head=head, **more)


def _zoo(n, memory, dtype, seed, two_chunks=True):
    """One batch that meets every state: -> (names, ptr, oracle state, frc0, f_step, fixed, energy).  ``n``: the size of the graph "big".
    Without ``two_chunks`` (and with n <= 256) no graph has more than one chunk: the entries take their one-launch form."""
    rng = np.random.default_rng(seed)
    part, full = min(2, memory), memory
    graphs = {
        "fresh": _graph(rng, 5, memory, dtype, status=lo.FRESH),
        "partly filled": _graph(rng, 6, memory, dtype, count=part),
        "full ring, wrapped head": _graph(rng, 7, memory, dtype, count=full, head=1 % memory),
        "rejected pair": _graph(rng, 5, memory, dtype, count=part, pair="rejected"),
        "big": _graph(rng, n, memory, dtype, count=full, head=(memory - 1)),
        "clamp": _graph(rng, 5, memory, dtype, count=0, fscale=60.0),
        "converged before": _graph(rng, 6, memory, dtype, status=lo.CONVERGED, count=part, converged_at=3, epot=-1.25, fmax=0.031),
        "newly converged": _graph(rng, 5, memory, dtype, count=part, fscale=1e-3),
        "fixed atoms": _graph(rng, 8, memory, dtype, count=part, fix=(0, 5)),
        "empty": _graph(rng, 0, memory, dtype),
        "lone atom, zero force": _graph(rng, 1, memory, dtype, count=0, fscale=0.0),
        "two chunks": _graph(rng, 300, memory, dtype, count=part),
    }
    if not two_chunks:
        del graphs["two chunks"]
    g = graphs["newly converged"]
    g["f"] = (1e-3 * rng.standard_normal((5, 3))).astype(dtype)
    g = graphs["lone atom, zero force"]
    g["f"], g["pending"] = np.zeros((1, 3), dtype), np.zeros((1, 3))
    names, gs = list(graphs), list(graphs.values())
    G = len(gs)
    ptr = np.concatenate([[0], np.cumsum([q["m"] for q in gs])]).astype(np.int64)
    N = int(ptr[-1])
    st = lo.new_state(N, G, memory)
    for i, q in enumerate(gs):
        a, b = ptr[i], ptr[i + 1]
        st["hist_s"][:, a:b], st["hist_y"][:, a:b], st["pending"][a:b], st["gram"][i] = q["S"], q["Y"], q["pending"], q["gram"]
        st["count"][i], st["head"][i], st["status"][i] = q["count"], q["head"], q["status"]
        st["converged_at"][i], st["epot"][i], st["fmax"][i] = q.get("converged_at", -1), dtype(q.get("epot", 0.0)), dtype(q.get("fmax", 0.0))
        if q["status"] == lo.CONVERGED:
            st["delta"][i] = rng.standard_normal(2 * memory + 1) * lo.live(q["count"], memory)
    cat = lambda k: np.concatenate([q[k] for q in gs])
    return names, ptr, st, cat("f_prev"), cat("f"), cat("fixed"), np.linspace(-3.0, 2.0, G).astype(dtype)


def _device_round(dtype, ptr, st, x, frc0, f_step, fixed, energy, book, memory, n_edges=1, cell=None):
    """xeq_lbfgs_back, then xeq_lbfgs_front, on guarded copies: -> (buffers behind the back, buffers behind the front) as numpy."""
    from xequinet_amd import lib, resident

    n, G = len(x), len(ptr) - 1
    a0, cn, gp = resident.chunk_tables(ptr)
    C = len(a0)
    most = int(np.diff(gp).max()) if G else 0
    code = 0 if dtype == np.float32 else 1
    tdt = torch.float32 if dtype == np.float32 else torch.float64
    batch = np.repeat(np.arange(G), np.diff(ptr)).astype(np.int64)
    g = {"pos": _t(x, tdt), "frc": _t(frc0, tdt), "image": _t(np.zeros((n, 3), np.int32)), "fs": _t(f_step, tdt), "en": _t(energy, tdt),
         "ne": _t(np.array([n_edges], np.int32)), "fixed": _t(fixed.astype(np.uint8)), "batch": _t(batch), "a0": _t(a0), "cn": _t(cn), "gp": _t(gp),
         "partial": torch.zeros((max(C, 1), 3 * (2 * memory + 3) + 1), dtype=torch.float64, device=DEV),
         "pbad": torch.zeros((max(C, 1), 4), dtype=torch.int32, device=DEV), "book": _t(book), "ticket": _t(np.zeros(1, np.int32)),
         "hist_s": _t(st["hist_s"]), "hist_y": _t(st["hist_y"]), "pending": _t(st["pending"]), "gram": _t(st["gram"]), "delta": _t(st["delta"]),
         "count": _t(st["count"]), "head": _t(st["head"]), "status": _t(st["status"]), "dropped": _t(st["dropped"]),
         "converged_at": _t(st["converged_at"]), "epot": _t(st["epot"], tdt), "fmax": _t(st["fmax"], tdt)}
    g = {k: gb.guarded_copy(t) for k, t in g.items()}
    cell_c = None if cell is None else (ctypes.c_double * 9)(*[float(v) for v in np.asarray(cell).reshape(-1)])
    pbc_c = None if cell is None else (ctypes.c_int32 * 3)(1, 1, 1)
    system = lib.fill(lib.ResSystem(), dtype=code, n=n, n_graphs=G, n_chunks=C, pos=g["pos"], frc=g["frc"], image=g["image"], batch=g["batch"],
                      book=g["book"], cell=cell_c, pbc=pbc_c)
    step = lib.fill(lib.ResStep(), frc_step=g["fs"], energy_step=g["en"], n_edges_step=g["ne"])
    chunks = lib.fill(lib.ResChunks(), chunk_atom0=g["a0"], chunk_n=g["cn"], graph_chunk_ptr=g["gp"], partial=g["partial"], partial_bad=g["pbad"])
    params = lib.fill(lib.LbfgsParams(), fixed=g["fixed"], hist_s=g["hist_s"], hist_y=g["hist_y"], pending_s=g["pending"], gram=g["gram"],
                      delta=g["delta"], count=g["count"], head=g["head"], status=g["status"], dropped=g["dropped"], converged_at=g["converged_at"],
                      epot=g["epot"], fmax=g["fmax"], ticket=g["ticket"], memory=memory, max_graph_chunks=most, fmax_tol=FMAX, alpha=ALPHA,
                      maxstep=MAXSTEP, damping=DAMPING)
    first = lib.launch_count()
    lib.call("xeq_lbfgs_back", ctypes.byref(system), ctypes.byref(step), ctypes.byref(chunks), ctypes.byref(params), None, lib.stream())
    torch.cuda.synchronize()
    gb.check(*g.values())
    behind_back = {k: t.cpu().numpy() for k, t in g.items()}
    assert lib.launch_count() - first == (1 if most <= 1 else 2)
    lib.call("xeq_lbfgs_front", ctypes.byref(system), ctypes.byref(chunks), ctypes.byref(params), lib.stream())
    torch.cuda.synchronize()
    gb.check(*g.values())
    assert lib.launch_count() - first == (2 if most <= 1 else 4)
    return behind_back, {k: t.cpu().numpy() for k, t in g.items()}


def _as_state(d):
    return {k: d[k].astype(np.float64) if d[k].dtype.kind == "f" else d[k] for k in ("hist_s", "hist_y", "pending", "gram", "delta", "count", "head",
                                                                                     "status", "dropped", "converged_at", "epot", "fmax")}


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("memory", [1, 3, 16])
@pytest.mark.parametrize("n,fused", [(1, False), (63, False), (65, False), (257, False), (1537, False), (1, True), (63, True), (65, True)],
                         ids=lambda v: ("one launch" if v else "two launches") if isinstance(v, bool) else str(v))
def test_kernels_alone(n, fused, memory, dtype):
    """``fused``: no graph above one chunk, so each entry is ONE launch (the form batches of molecules take), and open boundaries (no wrap);
    otherwise the two-chunk graph is in the batch, each entry is two launches, and the batch sits in a periodic cell."""
    names, ptr, st, frc0, f_step, fixed, energy = _zoo(n, memory, dtype, 100 * n + memory, two_chunks=not fused)
    cell, pbc = (None, None) if fused else (CELL, [True] * 3)
    rng = np.random.default_rng(n + 7)
    N, G, m, K = int(ptr[-1]), len(ptr) - 1, memory, 2 * memory + 1
    x = rng.uniform(-1.0, 5.0, (N, 3)).astype(dtype)
    book = np.array([9, 50, 0, 77], np.int64)
    back, front = _device_round(dtype, ptr, st, x, frc0, f_step, fixed, energy, book, memory, n_edges=64, cell=cell)
    par = dict(fmax_tol=FMAX, alpha=ALPHA, memory=memory, dtype=dtype)
    ref, frc_ref, info = lo.back(st, f_step, frc0, energy, fixed, ptr, 9, **par)
    # integers, the ring, forces: equal
    for k in ("count", "head", "status", "dropped", "converged_at"):
        assert np.array_equal(back[k], ref[k]), k
    assert np.array_equal(back["hist_s"], ref["hist_s"]) and np.array_equal(back["hist_y"], ref["hist_y"]) and np.array_equal(back["frc"], frc_ref)
    assert np.array_equal(back["epot"], ref["epot"].astype(dtype)) and _ulp_ok(back["fmax"], ref["fmax"].astype(dtype), dtype)
    assert back["book"].tolist() == [10, 64, 0, int((ref["status"] != lo.CONVERGED).sum())] and back["ticket"].tolist() == [0]
    i = {k: names.index(k) for k in names}
    assert info["accepted"][i["rejected pair"]] is False and info["accepted"][i["big"]] is True and ref["dropped"][i["rejected pair"]] == 1
    assert ref["status"][i["newly converged"]] == lo.CONVERGED and ref["converged_at"][i["newly converged"]] == 9
    assert ref["status"][i["empty"]] == lo.CONVERGED and ref["status"][i["lone atom, zero force"]] == lo.CONVERGED
    assert ref["fmax"][i["fixed atoms"]] < 40.0
    worst_b, worst_d, worst_own = 0.0, 0.0, 0.0
    for g in range(G):
        a, b = int(ptr[g]), int(ptr[g + 1])
        if st["status"][g] == lo.CONVERGED:          # converged before: every buffer of the graph byte-equal
            for k in PER_GRAPH:
                assert back[k][g].tobytes() == front[k][g].tobytes() == np.asarray(st[k][g]).astype(back[k].dtype).tobytes(), (names[g], k)
            assert np.array_equal(front["pos"][a:b], x[a:b]) and np.array_equal(front["frc"][a:b], frc0[a:b]) and not front["image"][a:b].any()
            assert np.array_equal(front["pending"][a:b], st["pending"][a:b])
            assert np.array_equal(front["hist_s"][:, a:b], st["hist_s"][:, a:b]) and np.array_equal(front["hist_y"][:, a:b], st["hist_y"][:, a:b])
            continue
        if ref["status"][g] == lo.CONVERGED:         # newly converged (or without atoms): no Gram row, no coefficients, no move
            assert np.array_equal(back["gram"][g], st["gram"][g]) and np.array_equal(back["delta"][g], st["delta"][g]), names[g]
            assert np.array_equal(front["pos"][a:b], x[a:b]) and np.array_equal(front["pending"][a:b], st["pending"][a:b])
            continue
        # Gram: the refreshed rows against math.fsum, the others untouched
        cnt, hd = int(ref["count"][g]), int(ref["head"][g])
        on = lo.live(cnt, m)
        rows = [2 * m] + ([(hd - 1) % m, m + (hd - 1) % m] if info["accepted"][g] else [])
        basis = lo.basis(ref, np.concatenate([np.zeros((a, 3)), frc_ref[a:b].astype(np.float64)]), a, b, m).reshape(K, -1)
        for r in range(K):
            for t in range(K):
                if not (on[r] and on[t]):
                    continue
                if r in rows or t in rows:
                    terms = basis[r] * basis[t]
                    want, room = math.fsum(terms), 32 * EPS * math.fsum(np.abs(terms))
                    err = abs(back["gram"][g, r, t] - want)
                    assert err <= room, (names[g], r, t, err, room)
                    worst_b = max(worst_b, err / room if room else 0.0)
                    assert back["gram"][g, r, t] == back["gram"][g, t, r]
                else:
                    assert back["gram"][g, r, t] == st["gram"][g, r, t], (names[g], r, t)
        # delta from the device's own B
        d_ref = lo.recursion(back["gram"][g], cnt, hd, m, ALPHA)
        own = np.abs(d_ref - lo.recursion(back["gram"][g], cnt, hd, m, ALPHA, reverse=True)).max()
        err = np.abs(back["delta"][g] - d_ref).max()
        if st["status"][g] == lo.FRESH or cnt == 0:
            assert np.array_equal(back["delta"][g], d_ref), names[g]
        assert err <= 8 * own + 4 * EPS * np.abs(d_ref).max(), (names[g], err, own)
        worst_d, worst_own = max(worst_d, err), max(worst_own, own)
    # the front, fed the device's state
    dev = _as_state(back)
    xr, pend, img, finfo = lo.front(dev, back["pos"], back["frc"], back["image"], fixed, ptr, cell, pbc, maxstep=MAXSTEP, damping=DAMPING,
                                    memory=memory, dtype=dtype)
    assert finfo["longest"][i["clamp"]] >= MAXSTEP and finfo["longest"][i["fresh"]] < MAXSTEP
    assert np.array_equal(front["image"], img)
    assert _ulp_ok(front["pos"], xr, dtype)
    moved = np.any(front["pos"] != back["pos"], axis=1) | np.any(front["image"] != 0, axis=1)
    assert not moved[fixed].any() and moved[ptr[i["big"]]:ptr[i["big"] + 1]].all()
    # the pending s IS (double)x_new - (double)x, taken before the wrap.  Where no image changed (every atom without a cell) the wrap is the
    # identity, the stored position is x_new and the two must agree bit for bit; an atom that crossed a face is held to: x + s is a dtype
    # value, exactly, and the unwrapped stored position is that value to the rounding of the unwrapping
    free_active = np.repeat(ref["status"] == lo.ACTIVE, np.diff(ptr)) & ~fixed
    stayed = free_active & ~np.any(front["image"] != 0, axis=1)
    assert np.array_equal(front["pending"][stayed], front["pos"][stayed].astype(np.float64) - back["pos"][stayed].astype(np.float64))
    assert stayed.sum() >= 20 and (fused or (free_active & ~stayed).sum() >= 20)          # both kinds are met
    if fused:
        assert np.array_equal(stayed, free_active) and not front["image"].any()
    else:
        unwrapped = mo.unwrapped(front["pos"].astype(np.float64), front["image"], CELL)
        x_new = back["pos"].astype(np.float64)[free_active] + front["pending"][free_active]
        assert np.array_equal(x_new.astype(dtype).astype(np.float64), x_new)
        assert np.abs(unwrapped[free_active] - x_new).max() <= 8 * np.spacing(dtype(8.0))
    assert np.array_equal(front["pending"][~free_active], back["pending"][~free_active])
    for k in ("hist_s", "hist_y", "gram", "delta", "count", "head", "status", "dropped", "converged_at", "frc", "book"):
        assert np.array_equal(front[k], back[k]), k                                                        # the front writes pos, image, pending alone
    print(f"lbfgs parity: n {n} {'one launch' if fused else 'two launches'} memory {memory} {np.dtype(dtype).name}: gram err / bound {worst_b:.3f}, delta err {worst_d:.3e}, own {worst_own:.3e}")
    parity_record.add({"test": "lbfgs_kernels_alone", "n": n, "fused": fused, "memory": memory, "dtype": np.dtype(dtype).name, "gram_err_over_bound": float(worst_b),
                       "delta_err": float(worst_d), "delta_own": float(worst_own)})


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("na", [65, 1537])
def test_a_graph_has_the_same_bits_anywhere(na, dtype):
    memory = 3
    rng = np.random.default_rng(900 + na)
    parts = {"a": _graph(rng, na, memory, dtype, count=3, head=2), "b": _graph(rng, 300, memory, dtype, count=2)}
    xs = {k: rng.uniform(-1.0, 5.0, (q["m"], 3)).astype(dtype) for k, q in parts.items()}

    def run(order):
        gs = [parts[k] for k in order]
        ptr = np.concatenate([[0], np.cumsum([q["m"] for q in gs])]).astype(np.int64)
        st = lo.new_state(int(ptr[-1]), len(gs), memory)
        for i, q in enumerate(gs):
            a, b = ptr[i], ptr[i + 1]
            st["hist_s"][:, a:b], st["hist_y"][:, a:b], st["pending"][a:b], st["gram"][i] = q["S"], q["Y"], q["pending"], q["gram"]
            st["count"][i], st["head"][i], st["status"][i] = q["count"], q["head"], q["status"]
        cat = lambda k: np.concatenate([q[k] for q in gs])
        _, got = _device_round(dtype, ptr, st, np.concatenate([xs[k] for k in order]), cat("f_prev"), cat("f"), cat("fixed"),
                               np.zeros(len(gs), dtype), np.zeros(4, np.int64), memory, cell=CELL)
        i = order.index("a")
        a, b = int(ptr[i]), int(ptr[i + 1])
        return (b"".join(got[k][i].tobytes() for k in PER_GRAPH) + b"".join(got[k][a:b].tobytes() for k in PER_ATOM)
                + got["hist_s"][:, a:b].tobytes() + got["hist_y"][:, a:b].tobytes()), got["count"][i]

    alone, first, last = run("a"), run("ab"), run("ba")
    assert alone[1] == 3 and alone[0] == first[0] == last[0]


# ------------------------------------------------------------------------------------------------------------------ 2. whole runs
N_ITER, MEMORY = 12, 4


@pytest.mark.parametrize("name", SYSTEMS)
def test_f64_trajectory_against_the_host_minimiser(name):
    ref = lo.host_run(name, np.float64, N_ITER, FMAX, memory=MEMORY)
    offered = 0
    for it in range(N_ITER + 1):                      # the conditions the comparison of decisions rests on
        for g, acc in enumerate(ref["accepted"][it]):
            if acc is not None:
                offered += 1
                assert (ref["cos"][it][g] > 1e-6) if acc else (ref["cos"][it][g] < -1e-6), (it, g)
            if ref["longest"][it][g] is not None:
                assert abs(ref["longest"][it][g] / MAXSTEP - 1.0) > 1e-6, (it, g)
            if ref["status"][it][g] != lo.CONVERGED:
                assert abs(ref["fmax"][it][g] / FMAX - 1.0) > 1e-6, (it, g)
    assert offered >= N_ITER and ref["count"][-1].max() == MEMORY
    o = _lbfgs(name, torch.float64, memory=MEMORY)
    assert o.run(N_ITER, check_every=N_ITER) is False and o.step_count == N_ITER
    got = _state(o)
    for k, want in (("pos", ref["pos"][-1]), ("epot", ref["epot"][-1])):
        err, scale = np.abs(_np(got[k]) - want).max(), np.abs(want).max()
        print(f"lbfgs parity: f64 {name} {k}: max abs error {err:.3e}, largest {scale:.3e}")
        parity_record.add({"test": "lbfgs_f64_trajectory", "system": name, "quantity": k, "max_abs_err": float(err), "scale": float(scale)})
        assert err <= 1e-9 * scale, (k, err, scale)
    st = ref["state"]
    for k in ("count", "head", "status", "dropped", "converged_at"):
        assert np.array_equal(got[k].cpu().numpy(), st[k]), k
    if name == "water box":
        assert np.array_equal(got["image"].cpu().numpy(), ref["image"])


def _converged_run(name):
    """The f32 run to convergence, recorded at every iteration: shared by the tests below (and left unchanged by them)."""
    def make():
        o = _lbfgs(name, torch.float32)
        e0 = o.potential_energy
        x0 = o.unwrapped_positions
        done = o.run(400, check_every=20, record_every=1)
        return o, e0, x0, done

    return hc.cached(("lbfgs f32 run", name), make)


RISES = {"ragged": [3]}          # graphs whose energy the f64 HOST minimiser itself leaves above the start (asserted on its run below)


@pytest.mark.parametrize("name", SYSTEMS)
def test_f32_runs_converge(name):
    """test_gpu_fire.py::test_f32_runs_converge's criterion: the f64 oracle's fmax at the device's final positions against 0.05 + 4 x the
    f32 oracle's own force error there; a graph that converged at evaluation 0 never moved: its final energy IS the starting one, every
    other graph's is below -- but for the graphs of RISES, which the rule (no line search: no descent guarantee) takes uphill on the f64
    host minimiser too: that is asserted here on the oracle's run, and such a graph is held to everything else."""
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
    print(f"lbfgs parity: f32 {name}: converged at {at.tolist()}, f64-oracle fmax {fm.max():.5f}, f32 oracle's own force error {own:.3e}, "
          f"bound {FMAX + 4 * own:.5f}; device fmax {_np(o.max_force).max():.5f}; dropped {o.dropped_pairs.cpu().tolist()}")
    parity_record.add({"test": "lbfgs_f32_converged", "system": name, "converged_at": at.tolist(), "oracle_fmax": float(fm.max()),
                       "f32_oracle_force_err": own, "bound": FMAX + 4 * own, "device_fmax": float(_np(o.max_force).max())})
    assert np.all(fm < FMAX + 4 * own), (fm, own)
    e1, e0 = _np(o.potential_energy), _np(e0)
    moved = at > 0
    down = moved.copy()
    if name in RISES:
        host = lo.host_run(name, np.float64, 400, FMAX, stop=True)
        went_up = (host["epot"][-1] > host["epot"][0]) & (host["converged_at"] > 0)
        assert np.all(host["state"]["status"] == lo.CONVERGED) and np.nonzero(went_up)[0].tolist() == RISES[name], (host["epot"][0], host["epot"][-1])
        down[RISES[name]] = False
    assert np.all(e1[down] < e0[down]) and np.array_equal(e1[~moved], e0[~moved]), (e0, e1)
    assert down.any() and int(at.max()) <= o.step_count <= 400


def test_converged_graphs_are_frozen_while_the_others_run_on():
    o, e0, x0, done = _converged_run("ragged")
    assert done is True
    ptr = fo.case("ragged")[2]
    at = o.converged_at.cpu().tolist()
    assert at[1] == 0 and at[2] == 0 and 0 < at[3] < at[0]
    assert torch.equal(o.potential_energy[1:3], e0[1:3])         # converged at evaluation 0: the energy bit for bit
    rows = o.trajectory["pos"]                                   # row r: behind evaluation r + 1
    steps = o.trajectory["step"].cpu().tolist()
    assert steps[: o.step_count] == list(range(1, o.step_count + 1))
    last = at[0] - 1
    for r in range(last + 1):
        assert torch.equal(rows[r, ptr[1]:ptr[3]], x0[ptr[1]:ptr[3]]), r
        if r >= at[3] - 1:
            assert torch.equal(rows[r, ptr[3]:], rows[at[3] - 1, ptr[3]:]), r
            assert torch.equal(o.trajectory["epot"][r, 1:], o.trajectory["epot"][at[3] - 1, 1:]), r          # converged graphs' recorder rows are constant
            assert torch.equal(o.trajectory["fmax"][r, 1:], o.trajectory["fmax"][at[3] - 1, 1:]), r
    assert not torch.equal(rows[at[3] - 1, ptr[3]:], x0[ptr[3]:]) and not torch.equal(rows[last, : ptr[1]], rows[at[3] - 1, : ptr[1]])
    assert torch.equal(rows[last], o.unwrapped_positions)


def test_batch_members_repeat_bit_for_bit():
    o, _, _, _ = _converged_run("qm9 seed 9")
    twin = _lbfgs("qm9 seed 9", torch.float32)
    assert twin.run(400, check_every=7) is True                  # another window length: the same states
    ptr = fo.case("qm9 seed 9")[2]
    assert torch.equal(twin.positions, o.positions) and torch.equal(twin.converged_at, o.converged_at)
    assert torch.equal(twin.hist_s, o.hist_s) and torch.equal(twin.gram, o.gram) and torch.equal(twin.delta, o.delta)
    for g in range(len(ptr) - 1):
        a, b = int(ptr[g]), int(ptr[g + 1])
        alone = _lbfgs("qm9 seed 9", torch.float32, sel=g)
        assert alone.run(400, check_every=20, record_every=1) is True
        n = alone.step_count
        assert torch.equal(alone.converged_at[0], o.converged_at[g]) and n >= int(o.converged_at[g])
        assert torch.equal(alone.trajectory["pos"][:n], o.trajectory["pos"][:n, a:b]), g
        assert torch.equal(alone.trajectory["epot"][:n, 0], o.trajectory["epot"][:n, g]) and torch.equal(alone.trajectory["fmax"][:n, 0], o.trajectory["fmax"][:n, g])
        assert torch.equal(alone.positions, o.positions[a:b]) and torch.equal(alone.gram[0], o.gram[g]) and torch.equal(alone.hist_y[:, :], o.hist_y[:, a:b])
        assert torch.equal(alone.history_length[0], o.history_length[g]) and torch.equal(alone.dropped_pairs[0], o.dropped_pairs[g])


def test_minimize_takes_the_method():
    from xequinet_amd import optimize

    p, z, ptr, _ = fo.case("qm9 seed 9")
    data = {"pos": _t(p, torch.float32), "atomic_numbers": _t(z), "ptr": _t(ptr)}
    out = optimize.minimize(_model(torch.float32), data, FMAX, max_steps=400, method="lbfgs", energy_unit="eV", length_unit="Angstrom")
    o, _, _, _ = _converged_run("qm9 seed 9")
    assert bool(out["converged"].all()) and torch.equal(out["pos"], o.positions) and out["n_steps"] == o.step_count


# ------------------------------------------------------------------------------------------------------------------ 3. residency
@pytest.mark.parametrize("name,per_iteration", [("qm9 seed 9", 2), ("water box", 2)])
def test_run_does_not_touch_the_host_between_checks(name, per_iteration):
    from xequinet_amd import lib

    o = _lbfgs(name, torch.float32)
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
    names = [n for n in lib.launch_names(n0) if n.startswith("xeq_lbfgs")]
    assert names.count("xeq_lbfgs_front") + names.count("xeq_lbfgs_back") == len(names) == 32 * per_iteration <= 32 * 4
    assert o.step_count == 36 and o.step.captures == captures
    assert bool(torch.isfinite(o.potential_energy).all())


# ------------------------------------------------------------------------------------------------------------------ 4. capacity / restore / reset
def test_a_list_that_outgrows_its_capacity_is_rerun_bit_for_bit():
    roomy = _lbfgs("water box", torch.float32, memory=MEMORY)
    small = _lbfgs("water box", torch.float32, memory=MEMORY, edge_capacity=64)       # the first evaluation's list has 1 286 edges
    assert small.edge_capacity == 64
    small.run(12, check_every=4)
    roomy.run(12, check_every=4)
    assert small.step_count == 12 and small.edge_capacity >= 1286 and roomy.edge_capacity >= 1286
    a, b = _state(small), _state(roomy)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_a_raised_non_finite_flag_leaves_the_checked_state():
    """The flag itself is the back kernel's; here the driver's answer to it: checkpoint back, then the error."""
    o = _lbfgs("qm9 seed 9", torch.float32)
    o.run(2)
    before = _state(o)
    real = o._read_book
    o._read_book = lambda: real()[:2] + (True,)
    with pytest.raises(FloatingPointError, match="LBFGS: .* evaluations 3 .. 6"):
        o.run(3)
    o._read_book = real
    assert o.step_count == 2 and o.book.cpu().tolist()[:3] == [3, 0, 0]
    after = _state(o)
    for k in before:
        assert torch.equal(before[k], after[k]), k
    o.run(3)
    assert o.step_count == 5


def test_the_back_raises_the_flag_on_a_non_finite_force_of_a_live_graph_only():
    memory = 3
    names, ptr, st, frc0, f_step, fixed, energy = _zoo(65, memory, np.float64, 11)
    x = np.zeros((int(ptr[-1]), 3))
    f_bad = f_step.copy()
    f_bad[ptr[names.index("converged before")]] = np.nan          # a converged graph's force is not looked at
    back, _ = _device_round(np.float64, ptr, st, x, frc0, f_bad, fixed, energy, np.zeros(4, np.int64), memory)
    assert back["book"][2] == 0
    e_bad = energy.copy()
    e_bad[names.index("two chunks")] = np.inf
    back, _ = _device_round(np.float64, ptr, st, x, frc0, f_step, fixed, e_bad, np.zeros(4, np.int64), memory)
    assert back["book"][2] == 1
    f_bad = f_step.copy()
    f_bad[ptr[names.index("two chunks")] + 299, 1] = np.nan       # in the graph's second chunk
    back, _ = _device_round(np.float64, ptr, st, x, frc0, f_bad, fixed, energy, np.zeros(4, np.int64), memory)
    assert back["book"][2] == 1


@pytest.mark.parametrize("name", ["qm9 seed 9", "water box"])
def test_reset_then_run_repeats_a_first_run_from_the_same_positions(name):
    a = _lbfgs(name, torch.float32, memory=MEMORY)
    a.run(7, check_every=3)
    start = _np(a.positions)
    a.reset()
    assert a.step_count == 0 and a.converged_at.cpu().tolist() == [-1] * a.n_graphs and not bool(a.history_length.any())
    b = _lbfgs(name, torch.float32, memory=MEMORY, pos=start)
    a.run(9, check_every=4)
    b.run(9, check_every=4)
    sa, sb = _state(a), _state(b)
    for k in sa:
        if k not in ("pos", "image"):          # (the first object carries the image counts of its first run)
            assert torch.equal(sa[k], sb[k]), k
    assert a.step_count == 9
