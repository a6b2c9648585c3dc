"""Per-step time of the device-resident NPT dynamics (xequinet_amd/md.py, ensemble "npt_berendsen") against a host-driven twin and
against the Berendsen thermostat alone, which must not have slowed down.

    python profiles/npt_timing.py --modes npt,twin,berendsen [--steps 1000] [--repeats 5] [--systems water192,water1536] [--tag this]
    python profiles/npt_timing.py --summarise <file with the lines of several runs> --out profiles/npt_timing.txt
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python profiles/npt_timing.py --trace water1536     (300 NPT steps)

Systems: the 192- and 1 536-atom water boxes (periodic).  Model: the default XPaiNN with fresh weights, f32; time step 0.1 fs (the
untrained surface is stiff), start at rest, thermostat 300 K / 20 fs; barostat 100 fs, 1e-3 / GPa, target = the start's own pressure.
  npt        md.Dynamics(ensemble="npt_berendsen"), check_every 100: front, the step's graph (tables kernel, search, model with virial), back
  twin       the same step class with compute_virial=True and a HOST-owned box: thermostat, barostat and velocity Verlet as torch
             operations, ``GraphedStepPBC.__call__`` once per step (the cell read back, the tables formed on the host and uploaded:
             ``_load_cell``; the edge count read back).  It does not wrap the positions (the search does not need it over a window).
  berendsen  md.Dynamics(ensemble="berendsen") -- the figure that is compared between this commit and its parent: the same script runs in
             a checkout of the parent (``--modes berendsen --tag parent``), processes alternating.
Each window is ``--steps`` steps between two device events after a warm-up of 200 steps; the modes of one process alternate and take
turns to go first.  One line per (tag, system, mode): ms per step, median (min .. max) over the windows.
"""
import argparse
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from xequinet_amd import md  # noqa: E402
from xequinet_amd.data import synthetic as syn  # noqa: E402
from xequinet_amd.nn import resolve_model  # noqa: E402
from xequinet_amd.runtime import GraphedStepPBC  # noqa: E402

DEV = "cuda"
DT, T_K, TAUT, TAUP, BETA = 0.1, 300.0, 20.0, 100.0, 1.0e-3
MASS = {1: 1.008, 6: 12.011, 7: 14.007, 8: 15.999, 9: 18.998}


def system(name):
    pos, z, ptr, cell = syn.synth_water_box({"water192": 4, "water1536": 8}[name], seed=5)
    return pos, z, np.asarray(cell).reshape(3, 3)


def t(a, dt=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dt).to(DEV)


class HostTwin:
    """Berendsen NPT in torch around step.__call__ with a box the host owns."""

    def __init__(self, model, pos, z, cell, masses, p0, capacity):
        f = md.unit_factors("eV", "Angstrom")
        self.pos, self.z, self.cell = pos.clone(), z, cell.clone()
        self.pbc = torch.tensor([True, True, True], device=DEV)
        self.step = GraphedStepPBC(model, len(z), capacity, compute_virial=True)
        self.im = (f["accel"] / masses)[:, None].to(pos.dtype)
        self.hm = (masses / (2.0 * f["accel"]))[:, None].to(pos.dtype)
        self.tfac = 2.0 / (3.0 * len(z) * f["kB"])
        self.kappa, self.p0 = (DT / TAUP) * (BETA / f["GPa"] / 3.0), p0 * f["GPa"]
        self.vel = torch.zeros_like(pos)
        self.ke = torch.zeros((), dtype=pos.dtype, device=DEV)
        self._evaluate()

    def _evaluate(self):
        out = self.step(self.pos, self.z, self.cell, self.pbc)
        self.frc, self.vir = out["forces"], out["virial"]

    def run(self, n):
        h = 0.5 * DT
        for _ in range(n):
            tg = self.ke * self.tfac
            lam = torch.where(tg > 0, torch.sqrt(1.0 + (DT / TAUT) * (T_K / tg.clamp_min(1e-30) - 1.0)).clamp(0.9, 1.1), torch.ones_like(tg))
            self.vel *= lam
            c = self.cell
            vol = (c[0] * torch.linalg.cross(c[1], c[2])).sum().abs()
            p = (2.0 * self.ke + self.vir.reshape(3, 3).diagonal().sum()) / (3.0 * vol)
            mu = 1.0 - self.kappa * (self.p0 - p)
            self.cell = c * mu
            self.pos *= mu
            self.vel += h * self.frc * self.im
            self.pos += DT * self.vel
            self._evaluate()
            self.vel += h * self.frc * self.im
            self.ke = (self.hm * self.vel * self.vel).sum()


def window(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn(steps)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps          # ms per step


def make(name, mode, model):
    pos, z, cell = system(name)
    m = torch.tensor([MASS[int(a)] for a in z], dtype=torch.float64, device=DEV)
    kw = dict(timestep_fs=DT, energy_unit="eV", length_unit="Angstrom", temperature_K=T_K, taut_fs=TAUT, cell=t(cell, torch.float32))
    if mode == "berendsen":
        dyn = md.Dynamics(model, t(pos, torch.float32), t(z), m, ensemble="berendsen", **kw)
        return lambda n: dyn.run(n, check_every=100), dyn
    npt = dict(ensemble="npt_berendsen", taup_fs=TAUP, compressibility_per_GPa=BETA)
    probe = md.Dynamics(model, t(pos, torch.float32), t(z), m, pressure_GPa=0.0, **npt, **kw)
    p0 = float(probe.pressure)
    if mode == "npt":
        dyn = md.Dynamics(model, t(pos, torch.float32), t(z), m, pressure_GPa=p0, **npt, **kw)
        return lambda n: dyn.run(n, check_every=100), dyn
    twin = HostTwin(model, t(pos, torch.float32), t(z), t(cell, torch.float32), m, p0, int(1.25 * probe.edge_capacity) + 64)
    return twin.run, twin


def summarise(path, out):
    rows = {}
    for line in open(path):
        w = line.split()
        if len(w) >= 5 and w[0] == "npt_timing":
            rows.setdefault((w[2], w[3], w[1]), []).append([float(v) for v in w[4:]])
    lines = ["npt_timing: ms per step; every process: windows between device events after a 200-step warm-up, its modes alternating;",
             "processes of this commit and of the parent commit alternated in one call.  median (min .. max) over all windows of all processes;",
             "per-process medians behind it (their spread is the run-to-run spread of the same code)."]
    for (system_, mode, tag), runs in sorted(rows.items()):
        allw = [v for r in runs for v in r]
        meds = [float(np.median(r)) for r in runs]
        lines.append(f"{system_:10s} {mode:10s} {tag:7s} {np.median(allw):.4f} ({min(allw):.4f} .. {max(allw):.4f})  process medians: " +
                     " ".join(f"{v:.4f}" for v in meds) + (f"  spread of the process medians {100 * (max(meds) - min(meds)) / np.median(meds):.2f} %" if len(meds) > 1 else ""))
    for system_ in sorted({k[0] for k in rows}):
        this, parent = rows.get((system_, "berendsen", "this")), rows.get((system_, "berendsen", "parent"))
        if this and parent:
            a, b = np.median([np.median(r) for r in this]), np.median([np.median(r) for r in parent])
            lines.append(f"{system_:10s} berendsen  this / parent {a / b:.4f}")
        npt, twin = rows.get((system_, "npt", "this")), rows.get((system_, "twin", "this"))
        if npt and twin and this:
            a, b, c = (np.median([v for r in x for v in r]) for x in (npt, twin, this))
            lines.append(f"{system_:10s} twin / npt {b / a:.3f}   npt / berendsen {a / c:.3f} (the virial, the tables kernel and the barostat inside the step)")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out:
        with open(out, "w") as f:
            f.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--modes", default="npt,twin,berendsen")
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--systems", default="water192,water1536")
    ap.add_argument("--tag", default="this")
    ap.add_argument("--summarise", default=None)
    ap.add_argument("--trace", default=None, help="run 300 resident NPT steps of this system and exit (for a profiler)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.summarise:
        summarise(args.summarise, args.out)
        return
    torch.manual_seed(0)
    model = resolve_model("xpainn").to(DEV).eval().requires_grad_(False)
    if args.trace:
        make(args.trace, "npt", model)[0](300)
        torch.cuda.synchronize()
        return
    modes = args.modes.split(",")
    for name in args.systems.split(","):
        runs = {mode: make(name, mode, model) for mode in modes}
        for fn, _ in runs.values():
            fn(200)
        times = {mode: [] for mode in modes}
        for k in range(args.repeats):              # the modes take turns to go first
            for mode in modes[k % len(modes):] + modes[: k % len(modes)]:
                times[mode].append(window(runs[mode][0], args.steps))
        for mode in modes:
            obj = runs[mode][1]
            ok = bool(torch.isfinite(obj.ke).all()) if mode == "twin" else bool(torch.isfinite(obj.kinetic_energy).all())
            assert ok and math.isfinite(sum(times[mode])), (name, mode)
            print("npt_timing", args.tag, name, mode, " ".join(f"{v:.5f}" for v in times[mode]), flush=True)
        del runs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
