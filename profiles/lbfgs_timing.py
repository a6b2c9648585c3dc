"""Evaluations and wall time to convergence of the device-resident L-BFGS minimiser (optimize.LBFGS, memory 4 / 16 / 32) against the
device-resident FIRE minimiser (optimize.FIRE) from the same starts, the time per iteration of each, and the share of an L-BFGS iteration
that is spent in its own launches.

    python profiles/lbfgs_timing.py [--out profiles/lbfgs_timing.txt] [--systems aspirin,qm9x1024,water192,water1536] [--max-steps 3000]

Systems and model as profiles/fire_timing.py: aspirin (open), 1 024 QM9-shaped molecules as one batch (open), 192- and 1 536-atom water
boxes (periodic); the default XPaiNN with fresh weights, f32; ASE's defaults of both minimisers.

Convergence.  Every minimiser first runs once to the target (warm: the step's graph captured, the edge capacity settled); then the start
positions are put back, the minimiser is reset and the run is timed between two host clock readings with the device idle at both, in
windows of 20 iterations (the default; the run ends at the first check that finds no active graph, so the iterations done are a multiple
of 20 while "slowest graph" is the evaluation at which the last graph converged).  Three timed runs; they must repeat the warm run's
evaluation counts (the runs are deterministic).

Time per iteration.  FIRE as in profiles/fire_timing.txt: windows of 1 000 iterations between two device events at fmax = 1e-7 (every graph
stays active).  Both minimisers, like for like: the first 100 iterations from the start (every graph active: asserted), five windows each,
taking turns.  The L-BFGS launches alone: 200 x (xeq_lbfgs_front, xeq_lbfgs_back) enqueued without the step's graph between them on a
spent minimiser with a full ring (the back then sees an unchanged force, so every pair is rejected: the sums, the recursion and the move
run, the ring rows are not rewritten); that time over the time of a whole iteration is the share.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from xequinet_amd import lib, optimize  # noqa: E402
from xequinet_amd.data import synthetic as syn  # noqa: E402
from xequinet_amd.nn import resolve_model  # noqa: E402

DEV = "cuda"
METHODS = [("fire", {}), ("lbfgs m=4", {"memory": 4}), ("lbfgs m=16", {"memory": 16}), ("lbfgs m=32", {"memory": 32})]


def system(name):
    if name == "aspirin":
        pos, z, ptr = syn.synth_aspirin()
        return pos, z, ptr, None
    if name == "qm9x1024":
        pos, z, ptr = syn.synth_qm9_batch(1024, seed=1234)
        return pos, z, ptr, None
    pos, z, ptr, cell = syn.synth_water_box({"water192": 4, "water1536": 8}[name], seed=5)
    return pos, z, ptr, np.asarray(cell).reshape(3, 3)


def make(name, model, method, fmax, **kw):
    pos, z, ptr, cell = system(name)
    t = lambda a, dt=None: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).to(DEV)
    kw = dict(kw, fmax=fmax, energy_unit="eV", length_unit="Angstrom")
    if cell is not None:
        kw["cell"] = t(cell, torch.float32)
    else:
        kw["ptr"] = t(ptr)
    cls = optimize.FIRE if method == "fire" else optimize.LBFGS
    return cls(model, t(pos, torch.float32), t(z), **kw)


def restart(opt, start, image):
    """The start positions back into the step's static buffer, every graph fresh."""
    opt._pos.copy_(start)
    opt.image.copy_(image)
    opt.reset()


def timed_run(opt, max_steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    try:
        done = opt.run(max_steps, check_every=20)
    except FloatingPointError as e:
        return None, str(e)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, done


def window(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn(steps)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--systems", default="aspirin,qm9x1024,water192,water1536")
    ap.add_argument("--max-steps", type=int, default=3000)
    args = ap.parse_args()
    torch.manual_seed(0)
    model = resolve_model("xpainn").to(DEV).eval().requires_grad_(False)
    fmt = lambda v: f"{np.median(v):.4f} ({min(v):.4f} .. {max(v):.4f})"
    lines = [f"lbfgs_timing: runs to convergence in windows of 20 iterations, at most {args.max_steps}; wall ms = host clock with the device idle at both ends, "
             "median (min .. max) of 3 timed runs behind a warm one"]

    def say(s):
        lines.append(s)
        print(s, flush=True)

    for name in args.systems.split(","):
        for fmax in (0.05, 0.005):
            for label, kw in METHODS:
                opt = make(name, model, label.split()[0], fmax, **kw)
                start, image = opt.positions, opt.image.clone()
                e0 = opt.potential_energy
                wall, done = timed_run(opt, args.max_steps)
                if wall is None:
                    say(f"{name:10s} fmax {fmax:<6} {label:11s} FAILED: {done}")
                    continue
                at = opt.converged_at.cpu().numpy()
                steps, walls, same = opt.step_count, [], True
                for _ in range(3):
                    restart(opt, start, image)
                    w, d = timed_run(opt, args.max_steps)
                    same = same and d == done and opt.step_count == steps and np.array_equal(opt.converged_at.cpu().numpy(), at)
                    walls.append(w)
                conv = at >= 0
                de = (opt.potential_energy - e0).double().cpu().numpy()
                extra = "" if label == "fire" else f"  pairs rejected (all graphs) {int(opt.dropped_pairs.sum())}"
                say(f"{name:10s} fmax {fmax:<6} {label:11s} converged {int(conv.sum())} of {len(at)}  iterations done {steps}  slowest graph at evaluation "
                    f"{int(at.max()) if conv.all() else -1}  mean over graphs {at[conv].mean() if conv.any() else -1:.1f}  wall ms {fmt(walls)}  "
                    f"ms / iteration done {np.median(walls) / max(steps, 1):.4f}  energy change min {de.min():.4f} max {de.max():.4f}  "
                    f"timed runs repeat the warm one {same}{extra}")
                del opt
                torch.cuda.empty_cache()
        # time per iteration
        fire = make(name, model, "fire", 1e-7)
        fire.run(100)
        say(f"{name:10s} FIRE as in fire_timing.txt (fmax 1e-7, windows of 1000 iterations): ms / iteration {fmt([window(lambda n: fire.run(n, check_every=20), 1000) for _ in range(3)])}")
        del fire
        opts = {label: make(name, model, label.split()[0], 1e-7, **kw) for label, kw in METHODS}
        starts = {label: (o.positions, o.image.clone()) for label, o in opts.items()}
        for o in opts.values():
            o.run(100)
        times = {label: [] for label in opts}
        for k in range(5):
            order = list(opts) if k % 2 == 0 else list(opts)[::-1]
            for label in order:
                o = opts[label]
                restart(o, *starts[label])
                o.run(0)
                times[label].append(window(lambda n: o.run(n, check_every=20), 100))
                assert o._active_host == o.n_graphs
        say(f"{name:10s} first 100 iterations from the start, every graph active, ms / iteration: " + "  ".join(f"{label} {fmt(v)}" for label, v in times.items()))
        for label, o in opts.items():
            if label == "fire":
                continue
            L = lib.load()
            front, back, stream = L.xeq_lbfgs_front, L.xeq_lbfgs_back, lib.stream()
            fa, ba = (*o._front_args(), stream), (*o._back_args(True), stream)

            def own(n):
                for _ in range(n):
                    assert front(*fa) == 0 and back(*ba) == 0

            own(20)
            alone = [window(own, 200) for _ in range(3)]
            say(f"{name:10s} {label}: ring holds {int(o.history_length.min())} .. {int(o.history_length.max())} pairs; its launches alone "
                f"({2 if o._max_graph_chunks <= 1 else 4} per iteration) ms / iteration {fmt(alone)} = {100 * np.median(alone) / np.median(times[label]):.1f} % of an iteration")
        del opts
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
