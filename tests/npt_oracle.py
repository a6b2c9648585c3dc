"""Host side of the constant-pressure tests (tests/test_npt_host.py, tests/test_gpu_npt.py): the Berendsen barostat of csrc/xeq_md.hip
(xeq_npt_front / xeq_npt_back) restated in numpy on top of tests/md_oracle.py, with energies, forces and the virial from the oracle
(oracle/xpainn_oracle.py, ``compute_virial=True``: minus dE/dstrain) on a neighbour list rebuilt every step.  Per-atom and per-box
arithmetic is evaluated in f64 in the kernels' operation order and rounded to the state's type where the kernels store.
"""
import numpy as np
import torch

from oracle import xpainn_oracle as orc
from tests import hessian_cases as hc
from tests import md_oracle as mo

E_CHARGE = 1.602176634e-19                      # C, exact (SI 2019)
GPA_EV_A3 = 1.0e9 * 1.0e-30 / E_CHARGE          # one GPa in eV / Angstrom^3, by hand: 1e9 J / m^3 x 1e-30 m^3 / A^3 / (e J / eV)
PBC = [True, True, True]


def det(cell):
    """The determinant in the operation order of xeq_md_inverse_cell."""
    c = np.asarray(cell, dtype=np.float64).reshape(9)
    return c[0] * (c[4] * c[8] - c[5] * c[7]) - c[1] * (c[3] * c[8] - c[5] * c[6]) + c[2] * (c[3] * c[7] - c[4] * c[6])


def pressure(ke, virial, cell):
    """P = (2 KE + tr W) / (3 V) in energy / length^3."""
    w = np.asarray(virial, dtype=np.float64).reshape(9)
    return (2.0 * float(ke) + ((w[0] + w[4]) + w[8])) / (3.0 * abs(det(cell)))


def mu_of(p, p0, kappa):
    """ASE's linear form: mu = 1 - (dt / taup) (beta / 3) (P0 - P), kappa = (dt / taup) (beta / 3)."""
    return 1.0 - kappa * (p0 - p)


def kappa_of(dt, taup, compressibility_per_GPa, gpa):
    return (dt / taup) * (compressibility_per_GPa / gpa / 3.0)


def box_back(ke, virial, cell, kappa, p0, dtype):
    """The box half of xeq_npt_back: -> dict(mu, P, V, cell_next (f64 holding ``dtype`` values), bad)."""
    cell = np.asarray(cell, dtype=np.float64).reshape(3, 3)
    p = pressure(ke, virial, cell)
    mu = mu_of(p, p0, kappa)
    bad = not (np.isfinite(mu) and mu > 0.0)
    if bad:
        mu = 1.0
    nxt = (mu * cell).astype(dtype).astype(np.float64)
    return {"mu": mu, "P": p, "V": abs(det(cell)), "cell_next": nxt, "bad": bad}


def front(x, v, f, image, inv_mass, ke, tfac, *, dt, dt_over_tau, t0, mu, cell_next, dtype):
    """xeq_npt_front (dt > 0): lambda, x <- mu x for every atom, the half kick and the drift of the free ones, the wrap against the
    pending cell.  -> (x, v, image) as ``dtype``."""
    batch = np.zeros(len(x), dtype=np.int64)
    return mo.front(mu * np.asarray(x, dtype=np.float64), v, f, image, inv_mass, batch, ke, tfac, None, ensemble=mo.BERENDSEN, dt=dt,
                    dt_over_tau=dt_over_tau, t0=t0, cell=cell_next, pbc=PBC, dtype=dtype)


_ORACLES = {}


def _oracle(sd, tdtype):
    key = (id(sd), tdtype)
    if key not in _ORACLES:
        _ORACLES[key] = orc.XPaiNNOracle({k: (v.to(tdtype) if v.is_floating_point() else v) for k, v in sd.items()}, **hc.SMALL)
    return _ORACLES[key]


def host_of(x, z, cell, cutoff=hc.CUTOFF):
    xs = np.asarray(x, dtype=np.float64)
    c3 = np.asarray(cell, dtype=np.float64).reshape(1, 3, 3)
    ei, off = orc.radius_graph_pbc_oracle(xs, np.array([len(xs)]), PBC, c3, cutoff)
    return hc.host_batch(xs, z, np.array([0, len(xs)]), cell=c3, cell_offsets=off, edge_index=ei)


def evaluate(sd, x, z, cell, tdtype):
    """(energy [1], forces [N, 3], virial [3, 3], n_edges) as f64 arrays of ``tdtype`` values, on a list built for these positions and box."""
    host = host_of(x, z, cell)
    data = {k: (v.to(tdtype) if v.is_floating_point() else v) for k, v in host.items()}
    out = _oracle(sd, tdtype)(data, compute_forces=True, compute_virial=True)
    return (out["energy"].double().numpy().reshape(-1), out["forces"].double().numpy(), out["virial"].double().numpy().reshape(3, 3),
            int(host["edge_index"].shape[1]))


def energy(sd, x, z, cell):
    """The f64 oracle energy of one box (a list of its own)."""
    host = host_of(x, z, cell)
    return float(hc.oracle_energy_fn(sd, host)(host["pos"].clone()))


def integrate(sd, pos, z, masses, cell, *, dt, n_steps, dtype=np.float64, accel, kB, gpa, temperature, taut, pressure_GPa, taup,
              compressibility_per_GPa, v0=None):
    """The host NPT integrator.  -> dict of per-step lists (entry 0: the start): ``pos`` (unwrapped), ``vel``, ``epot`` [1], ``ekin`` [1],
    ``image``, ``frc``, ``cell`` [3, 3], ``pressure`` (GPa), ``virial`` [3, 3], ``mu``, ``volume``."""
    tdtype = torch.float64 if dtype == np.float64 else torch.float32
    n = len(pos)
    ptr = np.array([0, n])
    m = np.asarray(masses, dtype=np.float64)
    free = np.isfinite(m) & (m > 0)
    safe = np.where(free, m, 1.0)
    inv_mass = np.where(free, accel / safe, 0.0).astype(dtype)
    half_mass = np.where(free, safe / (2.0 * accel), 0.0).astype(dtype)
    tfac = np.where(free.sum() > 0, 2.0 / (3.0 * max(free.sum(), 1) * kB), 0.0).reshape(1).astype(dtype)
    kappa, p0 = kappa_of(dt, taup, compressibility_per_GPa, gpa), pressure_GPa * gpa
    cell = np.asarray(cell, dtype=np.float64).reshape(3, 3).astype(dtype).astype(np.float64)
    x = np.asarray(pos, dtype=np.float64).astype(dtype)
    v = (np.zeros((n, 3)) if v0 is None else np.asarray(v0, dtype=np.float64) * free[:, None]).astype(dtype)
    zero, batch = np.zeros((n, 3)), np.zeros(n, dtype=np.int64)
    x, _, image = mo.front(x, zero, zero, np.zeros((n, 3), np.int32), inv_mass, batch, None, tfac, None, ensemble=mo.NVE, dt=0.0, cell=cell, pbc=PBC,
                           dtype=dtype)
    e, f, w, _ = evaluate(sd, x, z, cell, tdtype)
    v, ke, _ = mo.back(v, f, inv_mass, half_mass, ptr, 0.0, dtype, advance=False)
    box = box_back(ke[0], w, cell, kappa, p0, dtype)
    out = {k: [] for k in ("pos", "vel", "epot", "ekin", "image", "frc", "cell", "pressure", "virial", "mu", "volume")}

    def record():
        unw = mo.unwrapped(x.astype(np.float64), image, cell).astype(dtype).astype(np.float64)
        for k, a in (("pos", unw), ("vel", v.astype(np.float64)), ("epot", e), ("ekin", ke.astype(np.float64)), ("image", image.copy()), ("frc", f),
                     ("cell", cell.copy()), ("pressure", box["P"] / gpa), ("virial", w), ("mu", box["mu"]), ("volume", box["V"])):
            out[k].append(a)

    record()
    for _ in range(n_steps):
        x, v, image = front(x, v, f, image, inv_mass, ke, tfac, dt=dt, dt_over_tau=dt / taut, t0=temperature, mu=box["mu"],
                            cell_next=box["cell_next"], dtype=dtype)
        cell = box["cell_next"]
        e, f, w, _ = evaluate(sd, x, z, cell, tdtype)
        v, ke, _ = mo.back(v, f, inv_mass, half_mass, ptr, 0.5 * dt, dtype)
        box = box_back(ke[0], w, cell, kappa, p0, dtype)
        record()
    return out
