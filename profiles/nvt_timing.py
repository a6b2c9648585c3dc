"""Per-step time of the canonical thermostats of md.Dynamics (ensembles "nose_hoover" and "bussi") next to the Berendsen thermostat,
whose entries this change leaves alone and which must not have slowed down.

    python profiles/nvt_timing.py --modes nose_hoover,bussi,berendsen [--steps 1000] [--repeats 5] [--systems aspirin,water192,water1536,qm9x1024] [--tag this]
    python profiles/nvt_timing.py --summarise <file with the lines of several runs> --out profiles/nvt_timing.txt

Systems: aspirin (open), the 192- and 1 536-atom water boxes (periodic), 1 024 QM9-shaped molecules as one batch (open).  Model: the
default XPaiNN with fresh weights, f32; time step 0.1 fs (the untrained surface is stiff), start at rest, 300 K / 20 fs, chain length 3.
  nose_hoover, bussi   the new ensembles: xeq_nvt_front, the step's graph, xeq_nvt_back
  berendsen            md.Dynamics(ensemble="berendsen") -- also the figure that is compared between this commit and its parent: the same
                       script runs in a checkout of the parent (``--modes berendsen --tag parent``), processes alternating.
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

DEV = "cuda"
DT, T_K, TAUT, CHAIN = 0.1, 300.0, 20.0, 3
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


def t(a, dt=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dt).to(DEV)


def window(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn(steps)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps          # ms per step


def make(name, mode, model):
    pos, z, ptr, cell = system(name)
    m = torch.tensor([MASS[int(a)] for a in z], dtype=torch.float64, device=DEV)
    kw = dict(timestep_fs=DT, energy_unit="eV", length_unit="Angstrom", temperature_K=T_K, taut_fs=TAUT, ensemble=mode)
    kw.update(dict(ptr=t(ptr)) if cell is None else dict(cell=t(cell, torch.float32)))
    if mode == "nose_hoover":
        kw["chain_length"] = CHAIN
    dyn = md.Dynamics(model, t(pos, torch.float32), t(z), m, **kw)
    return lambda n: dyn.run(n, check_every=100), dyn


def summarise(path, out):
    rows = {}
    for line in open(path):
        w = line.split()
        if len(w) >= 5 and w[0] == "nvt_timing":
            rows.setdefault((w[2], w[3], w[1]), []).append([float(v) for v in w[4:]])
    lines = ["nvt_timing: ms per step; every process: windows between device events after a 200-step warm-up, its modes alternating;",
             "processes of this commit and of the parent commit alternated in one call.  median (min .. max) over all windows of all processes;",
             "per-process medians behind it (their spread is the run-to-run spread of the same code)."]
    for (system_, mode, tag), runs in sorted(rows.items()):
        allw = [v for r in runs for v in r]
        meds = [float(np.median(r)) for r in runs]
        lines.append(f"{system_:10s} {mode:11s} {tag:7s} {np.median(allw):.4f} ({min(allw):.4f} .. {max(allw):.4f})  process medians: " +
                     " ".join(f"{v:.4f}" for v in meds) + (f"  spread of the process medians {100 * (max(meds) - min(meds)) / np.median(meds):.2f} %" if len(meds) > 1 else ""))
    for system_ in sorted({k[0] for k in rows}):
        this, parent = rows.get((system_, "berendsen", "this")), rows.get((system_, "berendsen", "parent"))
        if this and parent:
            a, b = np.median([np.median(r) for r in this]), np.median([np.median(r) for r in parent])
            lines.append(f"{system_:10s} berendsen    this / parent {a / b:.4f}")
        for mode in ("nose_hoover", "bussi"):
            new = rows.get((system_, mode, "this"))
            if new and this:
                a, b = np.median([np.median(r) for r in new]), np.median([np.median(r) for r in this])
                lines.append(f"{system_:10s} {mode:11s}  / berendsen {a / b:.4f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if out:
        with open(out, "w") as f:
            f.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--modes", default="nose_hoover,bussi,berendsen")
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--systems", default="aspirin,water192,water1536,qm9x1024")
    ap.add_argument("--tag", default="this")
    ap.add_argument("--summarise", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.summarise:
        summarise(args.summarise, args.out)
        return
    torch.manual_seed(0)
    model = resolve_model("xpainn").to(DEV).eval().requires_grad_(False)
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
            assert bool(torch.isfinite(runs[mode][1].kinetic_energy).all()) and math.isfinite(sum(times[mode])), (name, mode)
            print("nvt_timing", args.tag, name, mode, " ".join(f"{v:.5f}" for v in times[mode]), flush=True)
        del runs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
