"""Host side of the L-BFGS tests (tests/test_lbfgs_host.py, tests/test_gpu_lbfgs.py): numpy restatements of xeq_lbfgs_back and
xeq_lbfgs_front (csrc/xeq_lbfgs.hip; the contract is the text at the two prototypes in include/xeq.h), operation by operation and in
the stated summation orders -- evaluated in f64, rounded to the state's type where a value of that type is stored -- and a host minimiser
built on them and on md_oracle.evaluate, as fire_oracle.minimize is.

``reverse=True`` runs every row product of the recursion sequentially from the last basis vector to the first instead of in the stated
order (a pair per lane, a butterfly): the difference between the two on one Gram matrix is the reference's own rounding.
"""
import numpy as np

from tests import hessian_cases as hc
from tests import md_oracle as mo

FRESH, ACTIVE, CONVERGED = 0, 1, 2
CHUNK = 256
DEFAULTS = dict(memory=16, alpha=70.0, maxstep=0.2, damping=1.0)
_LANES = np.arange(64)


def new_state(n, n_graphs, memory):
    K = 2 * memory + 1
    return {"hist_s": np.zeros((memory, n, 3)), "hist_y": np.zeros((memory, n, 3)), "pending": np.zeros((n, 3)),
            "gram": np.zeros((n_graphs, K, K)), "delta": np.zeros((n_graphs, K)), "count": np.zeros(n_graphs, np.int32),
            "head": np.zeros(n_graphs, np.int32), "status": np.full(n_graphs, FRESH, np.int32), "dropped": np.zeros(n_graphs, np.int32),
            "converged_at": np.full(n_graphs, -1, np.int64), "epot": np.zeros(n_graphs), "fmax": np.zeros(n_graphs)}


def dot3(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def butterfly(v):
    """What every lane of a wave holds behind v += shuffle_xor(v, off) for off = 32, 16, .. 1."""
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[_LANES ^ off]
    return v[0]


def chunk_sum(terms):
    """A chunk's sum: lanes, butterfly, the four waves in order."""
    t = np.zeros(CHUNK)
    t[:len(terms)] = terms
    s = butterfly(t[:64])
    for w in range(1, 4):
        s = s + butterfly(t[64 * w:64 * w + 64])
    return s


def graph_sum(terms):
    """A graph's sum: chunks of CHUNK atoms counted from its first atom, added chunk after chunk."""
    if len(terms) == 0:
        return 0.0
    s = chunk_sum(terms[:CHUNK])
    for a in range(CHUNK, len(terms), CHUNK):
        s = s + chunk_sum(terms[a:a + CHUNK])
    return s


def live(count, memory):
    """The basis vectors that exist: the filled s slots, the filled y slots, g."""
    j = np.arange(memory)
    return np.concatenate([j < count, j < count, [True]])


def ring_order(count, head, memory):
    """The filled slots from OLDEST to NEWEST."""
    return [(head - count + t) % memory for t in range(count)]


def recursion(B, count, head, memory, alpha, reverse=False):
    """delta [K] of one graph from its Gram matrix: the two-loop recursion in coefficient space."""
    m, K = memory, 2 * memory + 1
    on = live(count, m)
    delta = np.zeros(K)
    delta[2 * m] = 1.0

    def rowdot(r):
        if reverse:
            s = 0.0
            for k in range(K - 1, -1, -1):
                if on[k]:
                    s = s + B[r, k] * delta[k]
            return s
        t = np.zeros(64)
        w = min(K, 64)
        t[:w] = np.where(on[:w], B[r, :w] * delta[:w], 0.0)
        if K > 64 and on[64]:
            t[0] = t[0] + B[r, 64] * delta[64]
        return butterfly(t)

    order = ring_order(count, head, m)
    a = {}
    with np.errstate(all="ignore"):
        for slot in reversed(order):
            a[slot] = rowdot(slot) / B[slot, m + slot]
            delta[m + slot] = delta[m + slot] - a[slot]
        delta = delta * (1.0 / alpha)
        for slot in order:
            beta = rowdot(m + slot) / B[slot, m + slot]
            delta[slot] = delta[slot] + (a[slot] - beta)
    return np.where(on, delta, 0.0)


def basis(state, frc64, lo, hi, memory):
    """[K, n_g, 3]: the basis vectors of one graph's atoms (rows of empty slots are whatever the ring holds)."""
    return np.concatenate([state["hist_s"][:, lo:hi], state["hist_y"][:, lo:hi], -frc64[None, lo:hi]])


def back(state, f_step, frc, energy, fixed, ptr, evaluation, *, fmax_tol, alpha, memory, dtype=np.float64, reverse=False, **_):
    """xeq_lbfgs_back behind evaluation ``evaluation``: -> (new state, new frc, info).  ``state`` is not changed.  info: per graph
    ``sy`` (the candidate pair's s.y), ``cos`` (s.y / (|s| |y|)), ``accepted`` (None where no pair was offered)."""
    st = {k: a.copy() for k, a in state.items()}
    m = memory
    ptr = np.asarray(ptr, dtype=np.int64)
    G = len(ptr) - 1
    n = len(f_step)
    fixed = np.zeros(n, bool) if fixed is None else np.asarray(fixed, dtype=bool)
    f_step = np.asarray(f_step, dtype=dtype)
    old = np.asarray(frc, dtype=dtype)
    new = old.copy()
    f64 = np.where(fixed[:, None], 0.0, f_step.astype(np.float64))
    info = {"sy": [None] * G, "cos": [None] * G, "accepted": [None] * G}
    for g in range(G):
        lo, hi = int(ptr[g]), int(ptr[g + 1])
        if state["status"][g] == CONVERGED:
            continue
        f = f64[lo:hi]
        fm = np.sqrt(np.max(dot3(f, f))) if hi > lo else 0.0
        st["epot"][g] = dtype(energy[g])
        st["fmax"][g] = dtype(fm)
        new[lo:hi] = np.where(fixed[lo:hi, None], dtype(0), f_step[lo:hi])
        if fm < fmax_tol:
            st["status"][g], st["converged_at"][g] = CONVERGED, evaluation
            continue
        cnt, hd = int(state["count"][g]), int(state["head"][g])
        accept = False
        if state["status"][g] == ACTIVE:
            s = np.where(fixed[lo:hi, None], 0.0, state["pending"][lo:hi])
            y = np.where(fixed[lo:hi, None], 0.0, old[lo:hi].astype(np.float64) - f)
            sy = graph_sum(dot3(s, y))
            accept = bool(np.isfinite(sy) and sy > 0.0)
            with np.errstate(all="ignore"):
                info["sy"][g], info["accepted"][g] = sy, accept
                info["cos"][g] = sy / np.sqrt(graph_sum(dot3(s, s)) * graph_sum(dot3(y, y)))
            if accept:
                st["hist_s"][hd, lo:hi], st["hist_y"][hd, lo:hi] = s, y
            else:
                st["dropped"][g] += 1
        cnt2, hd2 = (min(cnt + 1, m), (hd + 1) % m) if accept else (cnt, hd)
        b = basis(st, np.concatenate([np.zeros((lo, 3)), f]), lo, hi, m)
        on = live(cnt2, m)
        for r in ([hd, m + hd] if accept else []) + [2 * m]:
            for t in np.nonzero(on)[0]:
                st["gram"][g, r, t] = st["gram"][g, t, r] = graph_sum(dot3(b[r], b[t]))
        st["delta"][g] = recursion(st["gram"][g], cnt2, hd2, m, alpha, reverse)
        st["count"][g], st["head"][g], st["status"][g] = cnt2, hd2, ACTIVE
    return st, new, info


def direction(delta, count, b, memory):
    """p [n_g, 3] = -sum_k delta_k b_k in slot order over the basis vectors that exist."""
    acc = np.zeros(b.shape[1:])
    for k in np.nonzero(live(count, memory))[0]:
        acc = acc + delta[k] * b[k]
    return -acc


def front(state, x, frc, image, fixed, ptr, cell=None, pbc=None, *, maxstep, damping, memory, dtype=np.float64, delta=None, **_):
    """xeq_lbfgs_front: -> (x as ``dtype``, pending s f64, image, info); rows of fixed atoms and of graphs that are not ACTIVE are the
    inputs'.  ``delta``: coefficients to use instead of the state's.  info: ``longest`` per graph (None where the graph did not move)."""
    ptr = np.asarray(ptr, dtype=np.int64)
    G = len(ptr) - 1
    n = len(x)
    fixed = np.zeros(n, bool) if fixed is None else np.asarray(fixed, dtype=bool)
    x0 = np.asarray(x, dtype=dtype)
    image = np.zeros((n, 3), dtype=np.int32) if image is None else image
    delta = state["delta"] if delta is None else delta
    frc64 = np.asarray(frc, dtype=np.float64)
    xn, pend, img = x0.copy(), state["pending"].copy(), image.copy()
    info = {"longest": [None] * G}
    for g in range(G):
        lo, hi = int(ptr[g]), int(ptr[g + 1])
        if state["status"][g] != ACTIVE or hi == lo:
            continue
        free = ~fixed[lo:hi]
        p = np.where(free[:, None], direction(delta[g], int(state["count"][g]), basis(state, frc64, lo, hi, memory), memory), 0.0)
        longest = np.sqrt(np.max(dot3(p, p)))
        info["longest"][g] = longest
        with np.errstate(all="ignore"):
            scale = maxstep / longest if longest >= maxstep else 1.0
        step = damping * scale
        xo = x0[lo:hi].astype(np.float64)
        moved = (xo + step * p).astype(dtype)
        s = moved.astype(np.float64) - xo
        im = image[lo:hi]
        if cell is not None and pbc is not None and any(pbc):
            c = np.asarray(cell, dtype=np.float64).reshape(3, 3)
            w, im = mo.wrap(moved.astype(np.float64), image[lo:hi], c, mo.inverse_cell(c), pbc, dtype)
            moved = w.astype(dtype)
        f = free[:, None]
        xn[lo:hi], pend[lo:hi], img[lo:hi] = np.where(f, moved, x0[lo:hi]), np.where(f, s, state["pending"][lo:hi]), np.where(f, im, image[lo:hi])
    return xn, pend, img, info


def minimize(sd, pos, z, ptr, *, fmax, n_iter, fixed=None, cell=None, pbc=None, dtype=np.float64, stop=False, **kw):
    """The host minimiser: evaluation 0 at the start, then ``n_iter`` x (front, evaluation, back).  -> dict of per-evaluation lists
    (``pos`` unwrapped, ``epot``, ``fmax``, ``count``, ``head``, ``status``, ``dropped``, ``was``, ``cos``, ``accepted``, ``longest``)
    and the final ``state``, ``x``, ``frc``, ``image``, ``converged_at``.  ``stop``: end at the first evaluation behind which no graph
    is active."""
    import torch

    par = dict(DEFAULTS, **kw)
    tdtype = torch.float64 if dtype == np.float64 else torch.float32
    ptr = np.asarray(ptr, dtype=np.int64)
    n, G = len(pos), len(ptr) - 1
    fixed = np.zeros(n, bool) if fixed is None else np.asarray(fixed, dtype=bool)
    if cell is not None:
        cell = np.asarray(cell, dtype=np.float64).reshape(3, 3).astype(dtype).astype(np.float64)
        pbc = [True, True, True] if pbc is None else list(pbc)
    state = new_state(n, G, par["memory"])
    x = np.asarray(pos, dtype=np.float64).astype(dtype)
    frc = np.zeros((n, 3), dtype)
    image = np.zeros((n, 3), dtype=np.int32)
    if cell is not None:
        w = mo.wrap(x.astype(np.float64), image, cell, mo.inverse_cell(cell), pbc, dtype)
        x, image = w[0].astype(dtype), w[1]
    unw = (lambda: mo.unwrapped(x.astype(np.float64), image, cell).astype(dtype).astype(np.float64)) if cell is not None else (lambda: x.astype(np.float64))
    names = ("pos", "epot", "fmax", "count", "head", "status", "dropped", "was", "cos", "accepted", "longest")
    out = {k: [] for k in names}
    for it in range(n_iter + 1):
        longest = [None] * G
        if it:
            x, state["pending"], image, fi = front(state, x, frc, image, fixed, ptr, cell, pbc, dtype=dtype, **par)
            longest = fi["longest"]
        e, f = mo.evaluate(sd, x, z, ptr, cell, pbc, tdtype)
        was = state["status"].copy()
        state, frc, bi = back(state, f.astype(dtype), frc, e, fixed, ptr, it, fmax_tol=fmax, dtype=dtype, **par)
        for k, a in zip(names, (unw(), state["epot"].copy(), state["fmax"].copy(), state["count"].copy(), state["head"].copy(),
                                state["status"].copy(), state["dropped"].copy(), was, bi["cos"], bi["accepted"], longest)):
            out[k].append(a)
        if stop and np.all(state["status"] == CONVERGED):
            break
    out.update(state=state, x=x.astype(np.float64), frc=frc.astype(np.float64), image=image, converged_at=state["converged_at"].copy())
    return out


def host_run(name, dtype, n_iter, fmax, stop=False, **kw):
    from tests import fire_oracle as fo

    def make():
        p, z, ptr, cell = fo.case(name)
        return minimize(hc.model_case("well")[1], p, z, ptr, fmax=fmax, n_iter=n_iter, cell=cell, dtype=dtype, stop=stop, **kw)

    return hc.cached(("lbfgs host", name, np.dtype(dtype).name, n_iter, fmax, stop, tuple(sorted(kw.items()))), make)
