"""Final state and trajectory of short runs of the device-resident drivers (md.Dynamics, optimize.FIRE), written to an .npz so that two
builds can be held against each other byte for byte: everything a step uses is a function of the state, so a change that only moves how
arguments reach the kernels leaves every array as it was.

    python profiles/resident_parity.py --out A.npz            (run at one commit)
    python profiles/resident_parity.py --out B.npz            (run at the other)
    python profiles/resident_parity.py --compare A.npz B.npz  (exit status 1 unless the two hold the same arrays with the same bytes)

Runs, all with record_every = 5: 20 steps of Dynamics for nve, langevin and berendsen on a three-molecule open batch and on a 24-atom
water box, f32 and f64; npt_berendsen on that box; one run on the box with an edge capacity far below its list, so that a window is
restored, the arrays grow and the step is captured again; 20 iterations of FIRE on the same two systems.  Model: a small XPaiNN with
seeded weights.  Uses the drivers' public interface and their state tensors alone.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from xequinet_amd import md, optimize  # noqa: E402
from xequinet_amd.data import synthetic as syn  # noqa: E402
from xequinet_amd.nn import resolve_model  # noqa: E402

DEV = "cuda"
STEPS, EVERY = 20, 5
DT, T_K = 0.1, 300.0
MASS = {1: 1.008, 6: 12.011, 7: 14.007, 8: 15.999, 9: 18.998}
SMALL = dict(node_dim=128, node_irreps="128x0e + 64x1o + 32x2e", action_blocks=2, hidden_dim=64)
ENSEMBLES = {"nve": {}, "langevin": dict(temperature_K=T_K, friction_per_fs=0.01), "berendsen": dict(temperature_K=T_K, taut_fs=20.0),
             "npt_berendsen": dict(temperature_K=T_K, taut_fs=20.0, pressure_GPa=0.1, taup_fs=100.0, compressibility_per_GPa=0.05)}


def systems():
    pos, z, ptr = syn.synth_qm9_batch(3, seed=7)
    yield "open", pos, z, ptr, None
    pos, z, ptr, cell = syn.synth_water_box(2, seed=3)
    yield "box", pos, z, ptr, np.asarray(cell).reshape(3, 3)


def place(pos, z, ptr, cell, dtype):
    t = lambda a, dt=None: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).to(DEV)
    where = dict(cell=t(cell, dtype)) if cell is not None else dict(ptr=t(ptr))
    return t(pos, dtype), t(z), where


def dynamics(model, name, pos, z, ptr, cell, dtype, ensemble, **extra):
    x, zz, where = place(pos, z, ptr, cell, dtype)
    masses = torch.tensor([MASS[int(a)] for a in z], dtype=torch.float64, device=DEV)
    dyn = md.Dynamics(model, x, zz, masses, timestep_fs=DT, ensemble=ensemble, seed=11, energy_unit="eV", length_unit="Angstrom", **where,
                      **ENSEMBLES[ensemble], **extra)
    dyn.maxwell_boltzmann(T_K)
    dyn.run(STEPS, check_every=10, record_every=EVERY)
    state = dict(pos=dyn.positions, vel=dyn.vel, image=dyn.image, frc=dyn.frc, ke=dyn.ke, epot=dyn.epot, book=dyn.book,
                 captures=torch.tensor(dyn.step.captures), edge_capacity=torch.tensor(dyn.edge_capacity))
    if ensemble == "npt_berendsen":
        state.update(box=dyn.box, virial=dyn.vir, cell=dyn.cell)
    return state, dyn.trajectory


def fire(model, name, pos, z, ptr, cell, dtype):
    x, zz, where = place(pos, z, ptr, cell, dtype)
    opt = optimize.FIRE(model, x, zz, fmax=0.05, energy_unit="eV", length_unit="Angstrom", **where)
    opt.run(STEPS, check_every=10, record_every=EVERY)
    state = dict(pos=opt.positions, vel=opt.vel, image=opt.image, frc=opt.frc, epot=opt.epot, fmax=opt.fmax, dt=opt.dt, alpha=opt.alpha,
                 n_pos=opt.n_pos, status=opt.status, converged_at=opt.converged_at, coef=opt.coef, book=opt.book)
    return state, opt.trajectory


def collect():
    out = {}

    def keep(tag, result):
        state, trajectory = result
        assert len(trajectory) >= 4 and all(len(v) == STEPS // EVERY for v in trajectory.values()), tag
        for k, v in state.items():
            out[f"{tag}/{k}"] = v.detach().cpu().numpy()
        for k, v in trajectory.items():
            out[f"{tag}/traj_{k}"] = v.detach().cpu().numpy()
        print(tag, "finite" if all(np.isfinite(out[f"{tag}/{k}"]).all() for k in ("pos", "frc", "epot")) else "NOT FINITE", flush=True)

    for dtype in (torch.float32, torch.float64):
        torch.manual_seed(0)
        model = resolve_model("xpainn", **SMALL).to(DEV).to(dtype).eval().requires_grad_(False)
        dn = "f32" if dtype == torch.float32 else "f64"
        for name, pos, z, ptr, cell in systems():
            for ensemble in ("nve", "langevin", "berendsen"):
                keep(f"{dn}/{name}/{ensemble}", dynamics(model, name, pos, z, ptr, cell, dtype, ensemble))
            keep(f"{dn}/{name}/fire", fire(model, name, pos, z, ptr, cell, dtype))
            if cell is not None:
                keep(f"{dn}/{name}/npt_berendsen", dynamics(model, name, pos, z, ptr, cell, dtype, "npt_berendsen"))
                tag = f"{dn}/{name}/langevin, edge_capacity 256"
                keep(tag, dynamics(model, name, pos, z, ptr, cell, dtype, "langevin", edge_capacity=256))
                assert out[tag + "/captures"] >= 2 and out[tag + "/edge_capacity"] > 256, "the restore / grow path did not run"
    return out


def compare(a, b):
    a, b = np.load(a), np.load(b)
    differ = [k for k in a.files if k in b.files and (a[k].dtype != b[k].dtype or a[k].shape != b[k].shape or a[k].tobytes() != b[k].tobytes())]
    one_side = sorted(set(a.files) ^ set(b.files))
    print(f"{len(a.files)} arrays | {len(b.files)} arrays: {len(differ)} differ, {len(one_side)} on one side only")
    for k in differ + one_side:
        print("   ", k)
    return 1 if differ or one_side else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--compare", nargs=2, default=None)
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    arrays = collect()
    np.savez(args.out, **arrays)
    print(f"{len(arrays)} arrays -> {args.out}")
