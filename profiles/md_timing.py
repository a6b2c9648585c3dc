"""Per-step time of the device-resident dynamics (xequinet_amd/md.py) against what a user could write before it: the same step object
driven through its ``__call__`` once per step, with velocity Verlet (or the same BAOAB update with torch.randn noise) as torch tensor
operations on the device.

    python profiles/md_timing.py [--out profiles/md_timing.txt] [--steps 2000] [--repeats 5] [--systems aspirin,water192,water1536,qm9x1024]
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python profiles/md_timing.py --trace water192
    python profiles/md_timing.py --share <kernel_stats.csv>          (the share of xeq_md_front / xeq_md_back in that trace)

Systems: aspirin (open), 192- and 1 536-atom water boxes (periodic), 1 024 QM9-shaped molecules as one batch (open).  Model: the default
XPaiNN with fresh weights, f32; time step 0.1 fs (the untrained surface is stiff), start at rest, Langevin at 300 K with 0.01 / fs.
Each window is ``--steps`` steps between two device events; baseline and resident windows alternate in one process and take turns to go
first, ``--repeats`` of each after a warm-up of 200 steps each; the host time to enqueue 500 resident steps with no check is taken apart.  The resident run checks every 100 steps (its default); the baseline's ``__call__`` does what it does
at the parent commit (positions copied in, the box compared, the edge count read back).
"""
import argparse
import csv
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from xequinet_amd import md  # noqa: E402
from xequinet_amd.data import synthetic as syn  # noqa: E402
from xequinet_amd.nn import resolve_model  # noqa: E402
from xequinet_amd.runtime import GraphedStep, GraphedStepPBC, pair_capacity  # noqa: E402

DEV = "cuda"
DT, T_K, GAMMA = 0.1, 300.0, 0.01
MASS = {1: 1.008, 6: 12.011, 7: 14.007, 8: 15.999, 9: 18.998}


def system(name):
    if name == "aspirin":
        pos, z, ptr = syn.synth_aspirin()
        return pos, z, ptr, None
    if name == "qm9x1024":
        pos, z, ptr = syn.synth_qm9_batch(1024, seed=1234)
        return pos, z, ptr, None
    pos, z, ptr, cell = syn.synth_water_box({"water192": 4, "water1536": 8}[name], seed=5)
    return pos, z, ptr, np.asarray(cell).reshape(3, 3)


class Baseline:
    """Velocity Verlet / BAOAB in torch around step.__call__."""

    def __init__(self, model, pos, z, ptr, cell, masses, ensemble, capacity):
        f = md.unit_factors("eV", "Angstrom")
        self.pos, self.z, self.ptr = pos.clone(), z, ptr
        self.cell, self.pbc = cell, (torch.tensor([True, True, True], device=DEV) if cell is not None else None)
        self.step = GraphedStepPBC(model, len(z), capacity) if cell is not None else GraphedStep(model, (len(z), len(ptr) - 1, capacity))
        self.im = (f["accel"] / masses)[:, None].to(pos.dtype)
        self.vel = torch.zeros_like(pos)
        self.ensemble = ensemble
        self.c1 = math.exp(-GAMMA * DT)
        self.sigma = torch.sqrt((1.0 - self.c1**2) * f["kB"] * T_K * self.im)
        self.frc = self._forces().clone()

    def _forces(self):
        out = self.step(self.pos, self.z, self.cell, self.pbc) if self.cell is not None else self.step(self.pos, self.z, self.ptr)
        return out["forces"]

    def run(self, n):
        h = 0.5 * DT
        for _ in range(n):
            self.vel += h * self.frc * self.im
            if self.ensemble == "langevin":
                vn = self.c1 * self.vel + self.sigma * torch.randn_like(self.vel)
                self.pos += h * (self.vel + vn)
                self.vel = vn
            else:
                self.pos += DT * self.vel
            self.frc = self._forces()
            self.vel += h * self.frc * self.im


HOST = {}


def window(fn, steps, who=None):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    fn(steps)
    b.record()
    HOST.setdefault(who, []).append((time.perf_counter() - t0) * 1e3 / steps)      # ms of host time per step until the last enqueue
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps          # ms per step


def make(name, ensemble, model):
    pos, z, ptr, cell = system(name)
    m = torch.tensor([MASS[int(a)] for a in z], dtype=torch.float64, device=DEV)
    t = lambda a, dt=None: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).to(DEV)
    kw = dict(timestep_fs=DT, ensemble=ensemble, energy_unit="eV", length_unit="Angstrom")
    if ensemble == "langevin":
        kw.update(temperature_K=T_K, friction_per_fs=GAMMA)
    if cell is not None:
        kw["cell"] = t(cell, torch.float32)
    else:
        kw["ptr"] = t(ptr)
    dyn = md.Dynamics(model, t(pos, torch.float32), t(z), m, **kw)
    dyn.run(0)
    cap = int(1.25 * dyn.edge_capacity) + 64 if cell is not None else pair_capacity(ptr)
    base = Baseline(model, t(pos, torch.float32), t(z), t(ptr), None if cell is None else t(cell, torch.float32), m, ensemble, cap)
    return dyn, base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--systems", default="aspirin,water192,water1536,qm9x1024")
    ap.add_argument("--check-every", type=int, default=100, help="check_every of the resident run")
    ap.add_argument("--trace", default=None, help="run 300 resident Langevin steps of this system and exit (for a profiler)")
    ap.add_argument("--share", default=None, help="a rocprofv3 kernel_stats.csv: print the share of the md kernels")
    args = ap.parse_args()
    if args.share:
        rows = list(csv.DictReader(open(args.share)))
        name = next(k for k in rows[0] if k.lower() in ("name", "kernelname", "kernel_name"))
        dur = next(k for k in rows[0] if "total" in k.lower() and "duration" in k.lower())
        total = sum(float(r[dur]) for r in rows)
        for key in ("k_md_front", "k_md_back", "k_md_join"):
            part = sum(float(r[dur]) for r in rows if key in r[name])
            print(f"{key}: {100.0 * part / total:.2f} % of the kernel time of the trace")
        return
    torch.manual_seed(0)
    model = resolve_model("xpainn").to(DEV).eval().requires_grad_(False)
    if args.trace:
        dyn, _ = make(args.trace, "langevin", model)
        dyn.run(300)
        torch.cuda.synchronize()
        return
    lines = [f"md_timing: {args.steps} steps per window, {args.repeats} windows each, alternating and taking turns to go first; ms per step, median (min .. max)"]
    for name in args.systems.split(","):
        for ensemble in ("nve", "langevin"):
            dyn, base = make(name, ensemble, model)
            dyn.run(200)
            base.run(200)
            caps = dyn.step.captures
            res, ref = [], []
            resident = lambda n: dyn.run(n, check_every=args.check_every)
            for k in range(args.repeats):          # the two take turns to go first: clocks settle over the first windows of a process
                if k % 2 == 0:
                    ref.append(window(base.run, args.steps, (name, ensemble, "baseline")))
                    res.append(window(resident, args.steps, (name, ensemble, "resident")))
                else:
                    res.append(window(resident, args.steps, (name, ensemble, "resident")))
                    ref.append(window(base.run, args.steps, (name, ensemble, "baseline")))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dyn._enqueue(500)                     # no check inside: what the host needs to enqueue a step, nothing waited for
            enq = (time.perf_counter() - t0) * 1e3 / 500
            torch.cuda.synchronize()
            dyn.run(0)
            fmt = lambda v: f"{np.median(v):.4f} ({min(v):.4f} .. {max(v):.4f})"
            gain = [b / r for b, r in zip(ref, res)]
            lines.append(f"{name:10s} {ensemble:9s} baseline {fmt(ref)}  resident {fmt(res)}  baseline / resident {np.median(gain):.3f} ({min(gain):.3f} .. {max(gain):.3f})"
                         f"  re-captures inside the windows {dyn.step.captures - caps}  finite {bool(torch.isfinite(dyn.kinetic_energy).all())}"
                         f"  host ms/step until the last enqueue: baseline {np.median(HOST[(name, ensemble, 'baseline')]):.4f} resident incl. its read-backs {np.median(HOST[(name, ensemble, 'resident')]):.4f}, resident enqueue alone (500 steps, no check) {enq:.4f}")
            lines.append("           windows in order, baseline | resident: " + " ".join(f"{b:.4f}|{r:.4f}" for b, r in zip(ref, res)))
            print(lines[-2], flush=True)
            print(lines[-1], flush=True)
            del dyn, base
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
