"""Host side of the FIRE tests (tests/test_fire_host.py, tests/test_gpu_fire.py): numpy restatements of xeq_fire_back and xeq_fire_front
(csrc/xeq_md.hip), operation by operation -- evaluated in f64, rounded to the state's type where stored -- and a host minimiser built on
them and on md_oracle.evaluate (forces from the f64 / f32 oracle on a neighbour list rebuilt at every evaluation).

The per-graph sums are numpy's here (the device's order is its own: lanes, butterfly, waves, chunks), so a sum agrees with the device's to
rounding and a decision agrees wherever P is not within rounding of 0.
"""
import numpy as np

from tests import hessian_cases as hc
from tests import md_oracle as mo

FRESH, ACTIVE, CONVERGED = 0, 1, 2
DEFAULTS = dict(dt=0.1, maxstep=0.2, dtmax=1.0, n_min=5, f_inc=1.1, f_dec=0.5, alpha_start=0.1, f_alpha=0.99)


def new_state(n_graphs, dt, alpha_start):
    """The per-graph state of a fresh minimiser."""
    return {"dt": np.full(n_graphs, float(dt)), "alpha": np.full(n_graphs, float(alpha_start)), "n_pos": np.zeros(n_graphs, np.int32),
            "status": np.full(n_graphs, FRESH, np.int32), "converged_at": np.full(n_graphs, -1, np.int64), "coef": np.zeros((n_graphs, 3)),
            "epot": np.zeros(n_graphs), "fmax": np.zeros(n_graphs)}


def sums(v, f, fixed, ptr):
    """(P, ff, vv, max |f|^2) [G] over the free atoms, and the per-atom terms they are made of."""
    v, f = np.asarray(v, dtype=np.float64), np.asarray(f, dtype=np.float64)
    free = ~np.asarray(fixed, dtype=bool)[:, None]
    v, f = np.where(free, v, 0.0), np.where(free, f, 0.0)
    p = (f[:, 0] * v[:, 0] + f[:, 1] * v[:, 1]) + f[:, 2] * v[:, 2]
    ff = (f[:, 0] * f[:, 0] + f[:, 1] * f[:, 1]) + f[:, 2] * f[:, 2]
    vv = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
    seg = lambda a, op, empty: np.array([op(a[lo:hi]) if hi > lo else empty for lo, hi in zip(ptr[:-1], ptr[1:])])
    return seg(p, np.sum, 0.0), seg(ff, np.sum, 0.0), seg(vv, np.sum, 0.0), seg(ff, np.max, 0.0)


def back(state, v, f_step, frc, energy, fixed, ptr, evaluation, *, fmax_tol, maxstep, dtmax, n_min, f_inc, f_dec, alpha_start, f_alpha,
         dtype=np.float64, **_):
    """xeq_fire_back behind evaluation number ``evaluation``: -> (new state, new frc, dict of the graphs' sums).  ``state`` is not changed."""
    st = {k: a.copy() for k, a in state.items()}
    ptr = np.asarray(ptr, dtype=np.int64)
    G = len(ptr) - 1
    fixed = np.zeros(len(v), bool) if fixed is None else np.asarray(fixed, dtype=bool)
    batch = np.repeat(np.arange(G), np.diff(ptr))
    frozen = (state["status"] == CONVERGED)[batch] if G else np.zeros(0, bool)
    f_step = np.asarray(f_step, dtype=dtype)
    frc = np.where(frozen[:, None], np.asarray(frc, dtype=dtype), np.where(fixed[:, None], dtype(0), f_step)).astype(dtype)
    p, ff, vv, m2 = sums(v, f_step, fixed, ptr)
    for g in range(G):
        if state["status"][g] == CONVERGED:
            continue
        fm = np.sqrt(m2[g])
        st["epot"][g] = dtype(energy[g])
        st["fmax"][g] = dtype(fm)
        if fm < fmax_tol:
            st["status"][g], st["converged_at"][g] = CONVERGED, evaluation
            continue
        dt, al, n_pos = state["dt"][g], state["alpha"][g], int(state["n_pos"][g])
        if state["status"][g] == FRESH:
            cv, cf = 0.0, dt
        elif p[g] > 0.0:
            al_old = al
            cv = 1.0 - al
            if n_pos > n_min:
                dt = min(dt * f_inc, dtmax)
                al = al * f_alpha
            n_pos += 1
            with np.errstate(divide="ignore", invalid="ignore"):
                cf = al_old * np.sqrt(vv[g]) / np.sqrt(ff[g]) + dt
        else:
            cv, al, dt, n_pos = 0.0, alpha_start, dt * f_dec, 0
            cf = dt
        vn2 = ((cv * cv) * vv[g] + ((2.0 * cv) * cf) * p[g]) + (cf * cf) * ff[g]
        norm = dt * np.sqrt(max(vn2, 0.0)) if vn2 == vn2 else np.nan
        d = dt * (maxstep / norm) if norm > maxstep else dt
        st["dt"][g], st["alpha"][g], st["n_pos"][g], st["status"][g] = dt, al, n_pos, ACTIVE
        st["coef"][g] = (cv, cf, d)
    return st, frc, {"P": p, "ff": ff, "vv": vv, "m2": m2}


def front(state, x, v, frc, image, fixed, ptr, cell=None, pbc=None, dtype=np.float64):
    """xeq_fire_front: -> (x, v, image) as ``dtype``; rows of fixed atoms and of graphs that are not ACTIVE are the inputs'."""
    ptr = np.asarray(ptr, dtype=np.int64)
    G = len(ptr) - 1
    batch = np.repeat(np.arange(G), np.diff(ptr))
    fixed = np.zeros(len(x), bool) if fixed is None else np.asarray(fixed, dtype=bool)
    move = ((state["status"] == ACTIVE)[batch] if G else np.zeros(0, bool)) & ~fixed
    x0, v0 = np.asarray(x, dtype=dtype), np.asarray(v, dtype=dtype)
    image = np.zeros(x0.shape, dtype=np.int32) if image is None else image
    c = state["coef"][batch] if G else np.zeros((0, 3))
    vn = c[:, 0:1] * v0.astype(np.float64) + c[:, 1:2] * np.asarray(frc, dtype=np.float64)
    xn = x0.astype(np.float64) + c[:, 2:3] * vn
    img = image
    if cell is not None and pbc is not None and any(pbc):
        cell = np.asarray(cell, dtype=np.float64).reshape(3, 3)
        xn, img = mo.wrap(xn, image, cell, mo.inverse_cell(cell), pbc, dtype)
    m = move[:, None]
    return np.where(m, xn.astype(dtype), x0), np.where(m, vn.astype(dtype), v0), np.where(m, img, image)


def minimize(sd, pos, z, ptr, *, fmax, n_iter, fixed=None, cell=None, pbc=None, dtype=np.float64, stop=False, **kw):
    """The host minimiser: evaluation 0 at the start, then ``n_iter`` x (front, evaluation, back).  -> dict of per-evaluation lists
    (``pos`` unwrapped, ``epot``, ``fmax``, ``dt``, ``n_pos``, ``status``, ``P``, ``ff``, ``vv``) and the final ``state``, ``x``, ``frc``,
    ``converged_at``.  ``stop``: end at the first evaluation after which no graph is active."""
    import torch

    par = dict(DEFAULTS, **kw)
    tdtype = torch.float64 if dtype == np.float64 else torch.float32
    ptr = np.asarray(ptr, dtype=np.int64)
    n, G = len(pos), len(ptr) - 1
    fixed = np.zeros(n, bool) if fixed is None else np.asarray(fixed, dtype=bool)
    if cell is not None:
        cell = np.asarray(cell, dtype=np.float64).reshape(3, 3).astype(dtype).astype(np.float64)
        pbc = [True, True, True] if pbc is None else list(pbc)
    state = new_state(G, par["dt"], par["alpha_start"])
    x = np.asarray(pos, dtype=np.float64).astype(dtype)
    v = np.zeros((n, 3), dtype)
    frc = np.zeros((n, 3), dtype)
    image = np.zeros((n, 3), dtype=np.int32)
    if cell is not None:
        x = mo.wrap(x.astype(np.float64), image, cell, mo.inverse_cell(cell), pbc, dtype)
        x, image = x[0].astype(dtype), x[1]
    unw = (lambda: mo.unwrapped(x.astype(np.float64), image, cell).astype(dtype).astype(np.float64)) if cell is not None else (lambda: x.astype(np.float64))
    out = {k: [] for k in ("pos", "epot", "fmax", "dt", "n_pos", "status", "P", "ff", "vv", "was")}
    for it in range(n_iter + 1):
        if it:
            x, v, image = front(state, x, v, frc, image, fixed, ptr, cell, pbc, dtype)
        e, f = mo.evaluate(sd, x, z, ptr, cell, pbc, tdtype)
        was = state["status"].copy()
        state, frc, s = back(state, v, f.astype(dtype), frc, e, fixed, ptr, it, fmax_tol=fmax, dtype=dtype, **par)
        for k, a in (("pos", unw()), ("epot", state["epot"].copy()), ("fmax", state["fmax"].copy()), ("dt", state["dt"].copy()),
                     ("n_pos", state["n_pos"].copy()), ("status", state["status"].copy()), ("P", s["P"]), ("ff", s["ff"]), ("vv", s["vv"]), ("was", was)):
            out[k].append(a)
        if stop and np.all(state["status"] == CONVERGED):
            break
    out.update(state=state, x=x.astype(np.float64), v=v.astype(np.float64), frc=frc.astype(np.float64), image=image,
               converged_at=state["converged_at"].copy())
    return out


def case(name):
    """(pos, z, ptr, cell or None) of a system of tests/hessian_cases.py."""
    def make():
        h = hc.host_case(name)
        cell = h["cell"].numpy().reshape(3, 3).copy() if "cell" in h else None
        return h["pos"].numpy().copy(), h["atomic_numbers"].numpy().copy(), h["ptr"].numpy().copy(), cell

    return hc.cached(("fire system", name), make)


def host_run(name, dtype, n_iter, fmax, stop=False):
    def make():
        p, z, ptr, cell = case(name)
        return minimize(hc.model_case("well")[1], p, z, ptr, fmax=fmax, n_iter=n_iter, cell=cell, dtype=dtype, stop=stop)

    return hc.cached(("fire host", name, np.dtype(dtype).name, n_iter, fmax, stop), make)
