"""Host side of the molecular-dynamics tests (tests/test_md_host.py, tests/test_gpu_md.py): a numpy Philox4x32-10 with the counter layout
of include/xeq.h (xeq_md_normals), Box-Muller in f64, and an integrator for the three ensembles of xequinet_amd/md.py whose forces come
from the f64 / f32 oracle (oracle/xpainn_oracle.py through tests/hessian_cases.py) by ``autograd.grad`` on a neighbour list rebuilt every
step.  The per-atom updates restate csrc/xeq_md.hip operation by operation: evaluated in f64, rounded to the state's type where stored.
"""
import numpy as np
import torch

from oracle import xpainn_oracle as orc
from tests import hessian_cases as hc

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
NVE, LANGEVIN, BERENDSEN = 0, 1, 2
ENSEMBLES = {"nve": NVE, "langevin": LANGEVIN, "berendsen": BERENDSEN}
DT_FS = 0.4            # the GPU suite's time step: largest omega of its cases (f64 oracle Hessian, "well" weights) 0.270 (ragged), 0.332 (qm9 seed 9),
                        # 0.407 / fs (water box) -> omega dt = 0.108, 0.133, 0.163 < 0.2
MASS = {1: 1.008, 6: 12.011, 7: 14.007, 8: 15.999, 9: 18.998}        # g / mol: the tests' own table (the package carries none)


def philox4x32_10(counter, key):
    """counter [..., 4], key [..., 2] (uint32 values, broadcast together) -> the block [..., 4] as uint32."""
    c = np.asarray(counter, dtype=np.uint64) & MASK
    k = np.asarray(key, dtype=np.uint64) & MASK
    c0, c1, c2, c3 = (c[..., i].copy() for i in range(4))
    k0, k1 = (np.broadcast_to(k[..., i], c0.shape).copy() for i in range(2))
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & MASK, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + np.uint64(W0)) & MASK, (k1 + np.uint64(W1)) & MASK
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def counter_of(rng_id, step, purpose):
    """The layout of include/xeq.h: id low, id high, step low, step bits 32 .. 61 | purpose << 30."""
    ids = np.asarray(rng_id, dtype=np.int64).astype(np.uint64)
    step = int(step)
    assert 0 <= step < 2**62 and purpose in (0, 1)
    out = np.empty(ids.shape + (4,), dtype=np.uint64)
    out[..., 0], out[..., 1] = ids & MASK, ids >> np.uint64(32)
    out[..., 2], out[..., 3] = step & MASK, ((step >> 32) & MASK) | (purpose << 30)
    return out


def words(seed, purpose, step, rng_id):
    seed = int(seed) & (2**64 - 1)
    return philox4x32_10(counter_of(rng_id, step, purpose), np.array([seed & MASK, seed >> 32], dtype=np.uint64))


def box_muller(w, dtype=np.float64):
    """[n, 4] words -> [n, 3] normals: u = (x + 1) 2^-32 rounded once to ``dtype``, the transform in ``dtype`` (numpy's own log / sin / cos)."""
    u = ((w.astype(np.float64) + 1.0) * 2.0**-32).astype(dtype)
    two_pi = dtype(2.0 * np.pi)
    r0, r1 = np.sqrt(dtype(-2.0) * np.log(u[:, 0])), np.sqrt(dtype(-2.0) * np.log(u[:, 2]))
    return np.stack([r0 * np.cos(two_pi * u[:, 1]), r0 * np.sin(two_pi * u[:, 1]), r1 * np.cos(two_pi * u[:, 3])], axis=1).astype(dtype)


def normals(seed, purpose, step, rng_id):
    return box_muller(words(seed, purpose, step, rng_id))


def inverse_cell(cell):
    """The adjugate formula of csrc/xeq_resident.h (md_inverse), in its operation order: frac_k = sum_j x_j inv[j, k]."""
    c = np.asarray(cell, dtype=np.float64).reshape(9)
    det = c[0] * (c[4] * c[8] - c[5] * c[7]) - c[1] * (c[3] * c[8] - c[5] * c[6]) + c[2] * (c[3] * c[7] - c[4] * c[6])
    m = [c[4] * c[8] - c[5] * c[7], c[2] * c[7] - c[1] * c[8], c[1] * c[5] - c[2] * c[4],
         c[5] * c[6] - c[3] * c[8], c[0] * c[8] - c[2] * c[6], c[2] * c[3] - c[0] * c[5],
         c[3] * c[7] - c[4] * c[6], c[1] * c[6] - c[0] * c[7], c[0] * c[4] - c[1] * c[3]]
    return (np.array(m) / det).reshape(3, 3)


def wrap(x, image, cell, inv, pbc, dtype):
    """res_wrap (csrc/xeq_resident.h): two passes of (round to dtype, floor of the fractional coordinate, subtract); x f64 [n, 3] -> (x f64 holding dtype values
    after the caller's final rounding, image)."""
    per = np.asarray(pbc, dtype=bool)
    image = image.copy()
    for _ in range(2):
        x = x.astype(dtype).astype(np.float64)
        fr = (x[:, 0:1] * inv[0] + x[:, 1:2] * inv[1]) + x[:, 2:3] * inv[2]
        s = np.where(per, np.floor(fr), 0.0)
        x = x - ((s[:, 0:1] * cell[0] + s[:, 1:2] * cell[1]) + s[:, 2:3] * cell[2])
        image += s.astype(np.int32)
    return x, image


def unwrapped(x, image, cell):
    i = image.astype(np.float64)
    return x + ((i[:, 0:1] * cell[0] + i[:, 1:2] * cell[1]) + i[:, 2:3] * cell[2])


def berendsen_lambda(ke, tfac, t0, dt_over_tau):
    """lambda_g of xeq_md_front: 1 where T_g = ke tfac is not positive."""
    tg = np.asarray(ke, dtype=np.float64) * np.asarray(tfac, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        lam = np.sqrt(1.0 + dt_over_tau * (t0 / tg - 1.0))
    lam = np.fmin(np.fmax(lam, 0.9), 1.1)
    return np.where(tg > 0.0, lam, 1.0)


def front(x, v, f, image, inv_mass, batch, ke, tfac, z, *, ensemble, dt, c1=1.0, noise2=0.0, dt_over_tau=0.0, t0=0.0, cell=None, pbc=None,
          dtype=np.float64):
    """xeq_md_front on arrays holding ``dtype`` values (any float type): -> (x, v, image) as ``dtype``.  ``z`` [n, 3]: the normals."""
    x, v, f, im = (np.asarray(a, dtype=np.float64) for a in (x, v, f, inv_mass))
    im = im[:, None]
    if ensemble == BERENDSEN:
        v = berendsen_lambda(ke, tfac, t0, dt_over_tau)[np.asarray(batch)][:, None] * v
    h = 0.5 * dt
    free = im > 0.0
    vk = v + h * (f * im)
    if ensemble == LANGEVIN:
        vn = c1 * vk + np.sqrt(noise2 * im) * np.asarray(z, dtype=np.float64)
        xn = x + h * (vk + vn)
    else:
        vn, xn = vk, x + dt * vk
    v, x = np.where(free, vn, 0.0), np.where(free, xn, x)
    image = np.zeros(x.shape, dtype=np.int32) if image is None else image
    if cell is not None and pbc is not None and any(pbc):
        cell = np.asarray(cell, dtype=np.float64).reshape(3, 3)
        x, image = wrap(x, image, cell, inverse_cell(cell), pbc, dtype)
    return x.astype(dtype), v.astype(dtype), image


def back(v, f, inv_mass, half_mass, ptr, half_dt, dtype=np.float64, advance=True):
    """The per-atom half of xeq_md_back and the per-graph kinetic energy (summed here by numpy in f64: the device's order is its own)."""
    v, f = np.asarray(v, dtype=np.float64), np.asarray(f, dtype=np.float64)
    im = np.asarray(inv_mass, dtype=np.float64)[:, None]
    if advance:
        v = np.where(im > 0.0, (v + half_dt * (f * im)).astype(dtype).astype(np.float64), v)
    e = np.asarray(half_mass, dtype=np.float64) * ((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
    ke = np.array([e[a:b].sum() for a, b in zip(ptr[:-1], ptr[1:])])
    return v.astype(dtype), ke.astype(dtype), e


def graph_energies_fn(sd, host, dtype):
    """pos [N, 3] -> the graphs' energies [G] on the oracle's pieces in ``dtype`` (hessian_cases.oracle_energy_fn without its sum)."""
    sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
    oracle = orc.XPaiNNOracle(sd, **hc.SMALL)
    fixed = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in host.items() if k != "pos"}

    def energy(pos):
        data = dict(fixed)
        data["pos"] = pos
        data = orc.compute_edge_data(data, compute_forces=False, compute_virial=False)
        data = oracle.embedding(data)
        for i in range(oracle.blocks):
            data = oracle.message(i, data)
            data = oracle.update(i, data)
        return oracle.energy_out(data)["energy"]

    return energy


def evaluate(sd, x, z, ptr, cell, pbc, tdtype):
    """(graph energies [G], forces [N, 3]) as f64 arrays of ``tdtype`` values, on a neighbour list built for these positions."""
    xs = np.asarray(x, dtype=np.float64)
    if cell is not None:
        c3 = np.asarray(cell, dtype=np.float64).reshape(1, 3, 3)
        ei, off = orc.radius_graph_pbc_oracle(xs, np.array([len(xs)]), list(pbc), c3, hc.CUTOFF)
        host = hc.host_batch(xs, z, ptr, cell=c3, cell_offsets=off, edge_index=ei)
    else:
        host = hc.host_batch(xs, z, ptr)
    pos = host["pos"].to(tdtype).clone().requires_grad_()
    e = graph_energies_fn(sd, host, tdtype)(pos)
    (g,) = torch.autograd.grad(e.sum(), pos)
    return e.detach().double().numpy().reshape(-1), -g.double().numpy()


def integrate(sd, pos, z, ptr, masses, *, dt, n_steps, ensemble="nve", dtype=np.float64, accel, kB, temperature=0.0, friction=0.0, taut=None,
              seed=0, rng_id=None, v0=None, cell=None, pbc=None, first_step=0):
    """The host integrator.  -> dict of per-step lists (entry 0: the start): ``pos`` (unwrapped), ``vel``, ``epot`` [G], ``ekin`` [G],
    ``image``; every array f64 holding ``dtype`` values."""
    tdtype = torch.float64 if dtype == np.float64 else torch.float32
    ens = ENSEMBLES[ensemble]
    ptr = np.asarray(ptr, dtype=np.int64)
    n, G = len(pos), len(ptr) - 1
    m = np.asarray(masses, dtype=np.float64)
    free = np.isfinite(m) & (m > 0)
    safe = np.where(free, m, 1.0)
    inv_mass = np.where(free, accel / safe, 0.0).astype(dtype)
    half_mass = np.where(free, safe / (2.0 * accel), 0.0).astype(dtype)
    batch = np.repeat(np.arange(G), np.diff(ptr))
    n_free = np.array([free[a:b].sum() for a, b in zip(ptr[:-1], ptr[1:])])
    tfac = np.where(n_free > 0, 2.0 / (3.0 * np.maximum(n_free, 1) * kB), 0.0).astype(dtype)
    c1 = float(np.exp(-friction * dt))
    noise2 = (1.0 - c1 * c1) * kB * temperature
    if rng_id is None:
        rng_id = (np.arange(n) - ptr[batch]) | (batch.astype(np.int64) << 32)
    if cell is not None:
        cell = np.asarray(cell, dtype=np.float64).reshape(3, 3).astype(dtype).astype(np.float64)
        pbc = [True, True, True] if pbc is None else list(pbc)
    x = np.asarray(pos, dtype=np.float64).astype(dtype)
    v = (np.zeros((n, 3)) if v0 is None else np.asarray(v0, dtype=np.float64) * free[:, None]).astype(dtype)
    image = np.zeros((n, 3), dtype=np.int32)
    zero = np.zeros((n, 3))
    x, _, image = front(x, zero, zero, image, inv_mass, batch, None, tfac, None, ensemble=NVE, dt=0.0, cell=cell, pbc=pbc, dtype=dtype)
    e, f = evaluate(sd, x, z, ptr, cell, pbc, tdtype)
    v, ke, _ = back(v, f, inv_mass, half_mass, ptr, 0.0, dtype, advance=False)
    unw = (lambda: unwrapped(x.astype(np.float64), image, cell).astype(dtype).astype(np.float64)) if cell is not None else (lambda: x.astype(np.float64))
    out = {"pos": [unw()], "vel": [v.astype(np.float64)], "epot": [e], "ekin": [ke.astype(np.float64)], "image": [image.copy()],
           "frc": [f]}
    for s in range(first_step, first_step + n_steps):
        zz = normals(seed, 0, s, rng_id).astype(dtype) if ens == LANGEVIN else None
        x, v, image = front(x, v, f, image, inv_mass, batch, ke, tfac, zz, ensemble=ens, dt=dt, c1=c1, noise2=noise2,
                            dt_over_tau=(dt / taut if taut else 0.0), t0=temperature, cell=cell, pbc=pbc, dtype=dtype)
        e, f = evaluate(sd, x, z, ptr, cell, pbc, tdtype)
        v, ke, _ = back(v, f, inv_mass, half_mass, ptr, 0.5 * dt, dtype)
        for k, a in (("pos", unw()), ("vel", v.astype(np.float64)), ("epot", e), ("ekin", ke.astype(np.float64)), ("image", image.copy()), ("frc", f)):
            out[k].append(a)
    return out


def masses_of(z):
    return np.array([MASS[int(a)] for a in np.asarray(z)])


def largest_omega(hessian, masses, accel):
    """sqrt of the largest eigenvalue of the mass-weighted Hessian [N, 3, N, 3] (energy / length^2 / (g / mol) * accel = 1 / fs^2)."""
    n = len(masses)
    w = 1.0 / np.sqrt(np.repeat(np.asarray(masses, dtype=np.float64), 3))
    h = np.asarray(hessian, dtype=np.float64).reshape(3 * n, 3 * n) * w[:, None] * w[None, :]
    return float(np.sqrt(max(np.linalg.eigvalsh(0.5 * (h + h.T)).max(), 0.0) * accel))
