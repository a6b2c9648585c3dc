"""Host side of the canonical-thermostat tests (tests/test_nvt_host.py, tests/test_gpu_nvt.py): the Nose-Hoover chain and the stochastic
velocity rescaling of csrc/xeq_md.hip (NvtThermostat; the contract is the text at xeq_nvt_back in include/xeq.h) restated in f64,
operation by operation, on Python floats (IEEE doubles; exp / log / sqrt / cos / sin are the C library's), and an integrator built on
md_oracle.front / back / evaluate / wrap.  The generator is md_oracle's Philox with purpose 2; a plain-integer copy of it serves the long
host runs (test_nvt_host.py holds the two against each other).
"""
import math

import numpy as np

from tests import md_oracle as mo

ROW, MAX_CHAIN, TRIES, PURPOSE = 18, 8, 16, 2           # XEQ_NVT_* of include/xeq.h (tests/test_nvt_host.py holds them against the header)
SCALE, BATH, XI, VXI = 0, 1, 2, 10
NOSE_HOOVER, BUSSI = 0, 1
KINDS = {"nose_hoover": NOSE_HOOVER, "bussi": BUSSI}
MASK = 0xFFFFFFFF
TWO_PI = 2.0 * math.pi
TWO_M32 = 2.0**-32


# What the GPU tests draw with (tests/test_gpu_nvt.py); gpu_draw_cases() lists every Bussi step they run, for the host's margin test.
KERNEL_SEED, KERNEL_STEP = 5, 2**32 + 17
SINGLE_SIZES = [1, 2, 63, 65, 256, 257, 1537]
RAGGED_SIZES = [1, 2, 255, 256, 257, 1281, 0, 3]          # the last graph's atoms are all fixed
MANY_GRAPHS = 1100
MOMENT_SEED, MOMENT_STEP, MOMENT_GRAPHS, MOMENT_NF = 2024, 3, 4096, (3, 6, 63)
TRAJ_SEED, TRAJ_STEPS = 11, 12                             # (the restore test runs 12 steps, the others 6)
TRAJ_SYSTEMS = ["ragged", "qm9 seed 9", "water box"]


def gpu_draw_cases():
    """(seed, graph id, step, Nf) of every Bussi step of tests/test_gpu_nvt.py; ids are the default g << 32."""
    from tests import hessian_cases as hc

    for n in SINGLE_SIZES:
        yield KERNEL_SEED, 0, KERNEL_STEP, 3 * n
    for g, n in enumerate(RAGGED_SIZES[:-1]):
        if n:
            yield KERNEL_SEED, g << 32, KERNEL_STEP, 3 * n
    for g in range(MANY_GRAPHS):
        yield KERNEL_SEED, g << 32, KERNEL_STEP, 3
    for nf in MOMENT_NF:
        for g in range(MOMENT_GRAPHS):
            yield MOMENT_SEED, g << 32, MOMENT_STEP, nf
    for name in TRAJ_SYSTEMS:
        ptr = hc.host_case(name)["ptr"].numpy()
        for g, n in enumerate(np.diff(ptr)):
            for step in range(TRAJ_STEPS):
                yield TRAJ_SEED, g << 32, step, 3 * int(n)


def philox_ints(c, k0, k1):
    """Philox4x32-10 on Python integers: c = four counter words -> four words."""
    c0, c1, c2, c3 = c
    for _ in range(10):
        p0, p1 = mo.M0 * c0, mo.M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + mo.W0) & MASK, (k1 + mo.W1) & MASK
    return c0, c1, c2, c3


def block(seed, graph_id, j, step):
    """Block j of (graph, step) under purpose 2 -> (z0, z1, u): the transform of include/xeq.h in double, u = (word_2 + 1) 2^-32."""
    seed, gid = int(seed) & (2**64 - 1), (int(graph_id) | int(j)) & (2**64 - 1)
    w = philox_ints((gid & MASK, gid >> 32, step & MASK, ((step >> 32) & MASK) | (PURPOSE << 30)), seed & MASK, seed >> 32)
    u0, u1, u2 = ((float(x) + 1.0) * TWO_M32 for x in w[:3])
    r0 = math.sqrt(-2.0 * math.log(u0))
    return r0 * math.cos(TWO_PI * u1), r0 * math.sin(TWO_PI * u1), u2


def gamma_draw(a, seed, graph_id, step, trace=None):
    """Marsaglia-Tsang with attempts j = 1 .. TRIES from blocks j; ``trace`` (a list) takes (j, log u, rhs, v) of every attempt."""
    d = a - 1.0 / 3.0
    cp = 1.0 / math.sqrt(9.0 * d)
    gam = 0.0
    for j in range(1, TRIES + 1):
        x, _, u = block(seed, graph_id, j, step)
        t = 1.0 + cp * x
        v = (t * t) * t
        gam = d * abs(v)
        rhs = ((0.5 * (x * x) + d) - d * v) + d * math.log(v) if v > 0.0 else -math.inf
        if trace is not None:
            trace.append((j, math.log(u), rhs, v))
        if v > 0.0 and math.log(u) < rhs:
            return gam
    return gam


def chi_square(nf, seed, graph_id, step, trace=None):
    """(R, S): the normal and the chi-square variate with nf - 1 degrees of freedom of one Bussi step."""
    r, z1, _ = block(seed, graph_id, 0, step)
    even = (nf - 1) % 2 == 0
    a = float((nf - 1 if even else nf - 2) // 2)
    gam = gamma_draw(a, seed, graph_id, step, trace)
    return r, (2.0 * gam if even else 2.0 * gam + z1 * z1)


def _chain_velocities(vxi, k_now, nfkT, q1, q, kT, hd, qd, M, down):
    for k in (range(M - 1, -1, -1) if down else range(M)):
        gk = (2.0 * k_now - nfkT) / q1 if k == 0 else ((q1 if k == 1 else q) * (vxi[k - 1] * vxi[k - 1]) - kT) / q
        if k == M - 1:
            vxi[k] = vxi[k] + hd * gk
        else:
            e = math.exp(-(qd * vxi[k + 1]))
            vxi[k] = vxi[k] * e
            vxi[k] = vxi[k] + hd * gk
            vxi[k] = vxi[k] * e


def nose_hoover_step(row, k_now, nf, kT, tau, dt, M):
    """-> (s, the new row or None when s is not finite and positive)."""
    xi, vxi = [float(v) for v in row[XI : XI + MAX_CHAIN]], [float(v) for v in row[VXI : VXI + MAX_CHAIN]]
    nfkT, tau2 = nf * kT, tau * tau
    q1, q = nfkT * tau2, kT * tau2
    delta = dt / 2.0
    hd, qd = 0.5 * delta, 0.25 * delta
    s = 1.0
    try:
        for _ in range(2):
            _chain_velocities(vxi, k_now, nfkT, q1, q, kT, hd, qd, M, True)
            sigma = math.exp(-(delta * vxi[0]))
            k_now = (sigma * sigma) * k_now
            s = s * sigma
            for k in range(M):
                xi[k] = xi[k] + delta * vxi[k]
            _chain_velocities(vxi, k_now, nfkT, q1, q, kT, hd, qd, M, False)
    except OverflowError:
        return math.inf, None
    if not (math.isfinite(s) and s > 0.0):
        return s, None
    b = 0.0
    for k in range(M):
        b = b + 0.5 * ((q1 if k == 0 else q) * (vxi[k] * vxi[k]))
    b = b + nfkT * xi[0]
    t = 0.0
    for k in range(1, M):
        t = t + xi[k]
    b = b + kT * t
    new = np.array(row, dtype=np.float64)
    new[BATH] = b
    new[XI : XI + M], new[VXI : VXI + M] = xi[:M], vxi[:M]
    return s, new


def bussi_step(row, k_now, nf, kT, tau, dt, seed, graph_id, step, trace=None):
    r, sdraw = chi_square(nf, seed, graph_id, step, trace)
    c = math.exp(-(dt / tau))
    q = ((1.0 - c) * (0.5 * (float(nf) * kT))) / (float(nf) * k_now)
    s2 = (c + q * (r * r + sdraw)) + (2.0 * r) * math.sqrt(c * q)
    s = math.sqrt(s2) if s2 >= 0.0 else math.nan
    if not (math.isfinite(s) and s > 0.0):
        return s, None
    new = np.array(row, dtype=np.float64)
    new[BATH] = new[BATH] - (s2 - 1.0) * k_now
    return s, new


def implied_chi_square(s, k_now, nf, kT, tau, dt, r):
    """S from a factor: the Bussi statement solved for it (the GPU moment test reads the device's draws this way)."""
    c = math.exp(-(dt / tau))
    q = ((1.0 - c) * (0.5 * (float(nf) * kT))) / (float(nf) * k_now)
    return (s * s - c - (2.0 * r) * math.sqrt(c * q)) / q - r * r


def join(kind, state, k_sums, n_free, *, advance, kT, tau, dt, chain_length=3, seed=0, graph_rng_id=None, step=0, dtype=np.float64, traces=None):
    """The thermostat part of xeq_nvt_back's join for every graph: -> (new state [G, ROW], ke [G] as ``dtype``, non-finite flag)."""
    state = np.array(state, dtype=np.float64).reshape(-1, ROW)
    G = len(state)
    ke = np.zeros(G)
    bad = False
    ids = (np.arange(G, dtype=np.int64) << 32) if graph_rng_id is None else np.asarray(graph_rng_id, dtype=np.int64)
    for g in range(G):
        K, nf = float(k_sums[g]), 3 * int(n_free[g])
        s = 1.0
        if advance and nf > 0 and K > 0.0:
            if kind == BUSSI:
                trace = None if traces is None else traces.setdefault(g, [])
                s, new = bussi_step(state[g], K, nf, kT, tau, dt, seed, int(ids[g]), int(step), trace)
            else:
                s, new = nose_hoover_step(state[g], K, float(nf), kT, tau, dt, chain_length)
            if new is None:
                bad |= not math.isfinite(s)
                s = 1.0
            else:
                state[g] = new
        state[g, SCALE] = s
        ke[g] = (s * s) * K
    return state, ke.astype(dtype), bad


def integrate(sd, pos, z, ptr, masses, *, dt, n_steps, ensemble, dtype=np.float64, accel, kB, temperature, taut, chain_length=3, seed=0,
              graph_rng_id=None, v0=None, cell=None, pbc=None, first_step=0, evaluate=None, keep=("pos", "vel", "epot", "ekin", "bath", "image")):
    """md_oracle.integrate with a canonical thermostat.  -> dict of per-step lists (entry 0: the start) of the quantities named in
    ``keep``: ``pos`` (unwrapped), ``vel`` (behind the pending factor, as the ``velocities`` property), ``epot``, ``ekin`` [G] (behind
    the factor), ``bath`` [G], ``image``, ``scale`` [G], ``state`` [G, ROW].  ``evaluate(x) -> (energies [G], forces [N, 3])`` replaces the model."""
    import torch

    tdtype = torch.float64 if dtype == np.float64 else torch.float32
    kind = KINDS[ensemble]
    ptr = np.asarray(ptr, dtype=np.int64)
    n, G = len(pos), len(ptr) - 1
    m = np.asarray(masses, dtype=np.float64)
    free = np.isfinite(m) & (m > 0)
    safe = np.where(free, m, 1.0)
    inv_mass = np.where(free, accel / safe, 0.0).astype(dtype)
    half_mass = np.where(free, safe / (2.0 * accel), 0.0).astype(dtype)
    batch = np.repeat(np.arange(G), np.diff(ptr))
    n_free = np.array([free[a:b].sum() for a, b in zip(ptr[:-1], ptr[1:])])
    if cell is not None:
        cell = np.asarray(cell, dtype=np.float64).reshape(3, 3).astype(dtype).astype(np.float64)
        pbc = [True, True, True] if pbc is None else list(pbc)
    ev = evaluate or (lambda x: mo.evaluate(sd, x, z, ptr, cell, pbc, tdtype))
    sums = lambda e: np.array([e[a:b].sum() for a, b in zip(ptr[:-1], ptr[1:])])
    x = np.asarray(pos, dtype=np.float64).astype(dtype)
    v = (np.zeros((n, 3)) if v0 is None else np.asarray(v0, dtype=np.float64) * free[:, None]).astype(dtype)
    image = np.zeros((n, 3), dtype=np.int32)
    zero = np.zeros((n, 3))
    x, _, image = mo.front(x, zero, zero, image, inv_mass, batch, None, None, None, ensemble=mo.NVE, dt=0.0, cell=cell, pbc=pbc, dtype=dtype)
    e, f = ev(x)
    v, _, per_atom = mo.back(v, f, inv_mass, half_mass, ptr, 0.0, dtype, advance=False)
    state = np.zeros((G, ROW))
    par = dict(kT=kB * temperature, tau=taut, dt=dt, chain_length=chain_length, seed=seed, graph_rng_id=graph_rng_id, dtype=dtype)
    state, ke, _ = join(kind, state, sums(per_atom), n_free, advance=False, **par)
    unw = (lambda: mo.unwrapped(x.astype(np.float64), image, cell).astype(dtype).astype(np.float64)) if cell is not None else (lambda: x.astype(np.float64))
    makers = {"pos": unw, "vel": lambda: (v.astype(np.float64) * state[batch, SCALE][:, None]).astype(dtype).astype(np.float64), "epot": lambda: e,
              "ekin": lambda: ke.astype(np.float64), "bath": lambda: state[:, BATH].copy(), "image": lambda: image.copy(),
              "scale": lambda: state[:, SCALE].copy(), "state": lambda: state.copy()}
    out = {k: [makers[k]()] for k in keep}
    for s in range(first_step, first_step + n_steps):
        scaled = state[batch, SCALE][:, None] * v.astype(np.float64)              # in double, not rounded: the kick follows in the same expression chain
        x, v, image = mo.front(x, scaled, f, image, inv_mass, batch, None, None, None, ensemble=mo.NVE, dt=dt, cell=cell, pbc=pbc, dtype=dtype)
        e, f = ev(x)
        v, _, per_atom = mo.back(v, f, inv_mass, half_mass, ptr, 0.5 * dt, dtype)
        state, ke, _ = join(kind, state, sums(per_atom), n_free, advance=True, step=s, **par)
        for k in keep:
            out[k].append(makers[k]())
    return out
