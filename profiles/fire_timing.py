"""Time per iteration of the device-resident FIRE minimiser (xequinet_amd/optimize.py) against what a user could write before it: the same
per-graph algorithm as torch tensor operations (segment sums by index_add_ / index_reduce_, ``where``s) around the same step object's
``__call__``, reading convergence back every ``check_every`` iterations.

    python profiles/fire_timing.py [--out profiles/fire_timing.txt] [--steps 1000] [--repeats 5] [--systems aspirin,water192,water1536,qm9x1024]

Systems: aspirin (open), 192- and 1 536-atom water boxes (periodic), 1 024 QM9-shaped molecules as one batch (open).  Model: the default
XPaiNN with fresh weights, f32; ASE's FIRE defaults; fmax = 1e-7, which no graph reaches in f32, so that every window does exactly
``--steps`` iterations with every graph active (a converged graph costs the same launches: it is masked, not removed).  Each window is
``--steps`` iterations between two device events; baseline and resident windows alternate in one process and take turns to go first,
``--repeats`` of each after a warm-up of 100 iterations each.  Both check every 20 iterations (the resident default); the baseline's
``__call__`` does what it does elsewhere (positions copied in; for a periodic box also the box compared and the edge count read back).
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from xequinet_amd import optimize  # noqa: E402
from xequinet_amd.data import synthetic as syn  # noqa: E402
from xequinet_amd.nn import resolve_model  # noqa: E402
from xequinet_amd.runtime import GraphedStep, GraphedStepPBC, pair_capacity  # noqa: E402

DEV = "cuda"
FMAX = 1e-7
PAR = dict(dt=0.1, maxstep=0.2, dtmax=1.0, n_min=5, f_inc=1.1, f_dec=0.5, alpha_start=0.1, f_alpha=0.99)


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
    """Per-graph FIRE in torch around step.__call__: the arithmetic of DESIGN.md section 13 in the state's type."""

    def __init__(self, model, pos, z, ptr, cell, capacity):
        self.pos, self.z, self.ptr = pos.clone(), z, ptr
        self.cell, self.pbc = cell, (torch.tensor([True, True, True], device=DEV) if cell is not None else None)
        G = len(ptr) - 1
        self.G = G
        self.step = GraphedStepPBC(model, len(z), capacity) if cell is not None else GraphedStep(model, (len(z), G, capacity))
        self.batch = torch.repeat_interleave(torch.arange(G, device=DEV), ptr[1:] - ptr[:-1])
        self.vel = torch.zeros_like(pos)
        f = lambda v, dt=pos.dtype: torch.full((G,), v, dtype=dt, device=DEV)
        self.dt, self.alpha, self.n_pos = f(PAR["dt"]), f(PAR["alpha_start"]), f(0, torch.int32)
        self.fresh, self.active = f(True, torch.bool), f(True, torch.bool)

    def _forces(self):
        out = self.step(self.pos, self.z, self.cell, self.pbc) if self.cell is not None else self.step(self.pos, self.z, self.ptr)
        return out["forces"]

    def run(self, n, check_every=20):
        G, b = self.G, self.batch
        seg = lambda a: torch.zeros(G, dtype=a.dtype, device=DEV).index_add_(0, b, a)
        for k in range(n):
            f, v = self._forces(), self.vel
            f2 = (f * f).sum(1)
            P, ff, vv = seg((f * v).sum(1)), seg(f2), seg((v * v).sum(1))
            fmax2 = torch.zeros(G, dtype=f.dtype, device=DEV).index_reduce_(0, b, f2, "amax", include_self=True)
            self.active = self.active & ~(fmax2 < FMAX * FMAX)
            up = (P > 0) & ~self.fresh
            down = ~up & ~self.fresh
            grow = up & (self.n_pos > PAR["n_min"])
            dt = torch.where(grow, torch.clamp(self.dt * PAR["f_inc"], max=PAR["dtmax"]), torch.where(down, self.dt * PAR["f_dec"], self.dt))
            alpha = torch.where(grow, self.alpha * PAR["f_alpha"], torch.where(down, torch.full_like(self.alpha, PAR["alpha_start"]), self.alpha))
            n_pos = torch.where(up, self.n_pos + 1, torch.zeros_like(self.n_pos))
            cv = torch.where(up, 1.0 - self.alpha, torch.zeros_like(dt))
            cf = torch.where(up, self.alpha * torch.sqrt(vv) / torch.sqrt(ff), torch.zeros_like(dt)) + dt
            norm = dt * torch.sqrt(torch.clamp(cv * cv * vv + 2.0 * cv * cf * P + cf * cf * ff, min=0.0))
            d = torch.where(norm > PAR["maxstep"], dt * (PAR["maxstep"] / norm), dt)
            act = self.active
            self.dt, self.alpha, self.n_pos = torch.where(act, dt, self.dt), torch.where(act, alpha, self.alpha), torch.where(act, n_pos, self.n_pos)
            self.fresh = self.fresh & ~act
            m = act[b][:, None]
            vn = cv[b][:, None] * v + cf[b][:, None] * f
            self.vel = torch.where(m, vn, v)
            self.pos = torch.where(m, self.pos + d[b][:, None] * vn, self.pos)
            if (k + 1) % check_every == 0 and not bool(self.active.any()):      # the read-back
                break


HOST = {}


def window(fn, steps, who=None):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    fn(steps)
    b.record()
    HOST.setdefault(who, []).append((time.perf_counter() - t0) * 1e3 / steps)      # ms of host time per iteration until the last enqueue
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps          # ms per iteration


def make(name, model):
    pos, z, ptr, cell = system(name)
    t = lambda a, dt=None: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).to(DEV)
    kw = dict(fmax=FMAX, energy_unit="eV", length_unit="Angstrom", **PAR)
    if cell is not None:
        kw["cell"] = t(cell, torch.float32)
    else:
        kw["ptr"] = t(ptr)
    opt = optimize.FIRE(model, t(pos, torch.float32), t(z), **kw)
    opt.run(0)
    cap = int(1.25 * opt.edge_capacity) + 64 if cell is not None else pair_capacity(ptr)
    base = Baseline(model, t(pos, torch.float32), t(z), t(ptr), None if cell is None else t(cell, torch.float32), cap)
    return opt, base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--systems", default="aspirin,water192,water1536,qm9x1024")
    ap.add_argument("--check-every", type=int, default=20)
    args = ap.parse_args()
    torch.manual_seed(0)
    model = resolve_model("xpainn").to(DEV).eval().requires_grad_(False)
    lines = [f"fire_timing: {args.steps} iterations per window, {args.repeats} windows each, alternating and taking turns to go first; "
             f"check every {args.check_every}; ms per iteration, median (min .. max)"]
    for name in args.systems.split(","):
        opt, base = make(name, model)
        opt.run(10, check_every=args.check_every)          # the two are the same algorithm: ten moves from the same start
        base.run(10, args.check_every)
        same = float((opt.unwrapped_positions - base.pos).abs().max())
        opt.run(90, check_every=args.check_every)
        base.run(90, args.check_every)
        caps = opt.step.captures
        res, ref = [], []
        resident = lambda n: opt.run(n, check_every=args.check_every)
        baseline = lambda n: base.run(n, args.check_every)
        first = opt.step_count
        for k in range(args.repeats):          # the two take turns to go first: clocks settle over the first windows of a process
            if k % 2 == 0:
                ref.append(window(baseline, args.steps, (name, "baseline")))
                res.append(window(resident, args.steps, (name, "resident")))
            else:
                res.append(window(resident, args.steps, (name, "resident")))
                ref.append(window(baseline, args.steps, (name, "baseline")))
        done = opt.step_count - first
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        opt._enqueue(500)                     # no check inside: what the host needs to enqueue an iteration, nothing waited for
        enq = (time.perf_counter() - t0) * 1e3 / 500
        torch.cuda.synchronize()
        fmt = lambda v: f"{np.median(v):.4f} ({min(v):.4f} .. {max(v):.4f})"
        gain = [b / r for b, r in zip(ref, res)]
        lines.append(f"{name:10s} baseline {fmt(ref)}  resident {fmt(res)}  baseline / resident {np.median(gain):.3f} ({min(gain):.3f} .. {max(gain):.3f})"
                     f"  resident iterations done {done} of {args.steps * args.repeats}, baseline graphs still active {int(base.active.sum())} of {base.G}"
                     f"  re-captures inside the windows {opt.step.captures - caps}  max |resident - baseline| position after 10 moves {same:.2e}  finite {bool(torch.isfinite(opt.potential_energy).all())}"
                     f"  host ms/iteration until the last enqueue: baseline {np.median(HOST[(name, 'baseline')]):.4f} resident incl. its read-backs "
                     f"{np.median(HOST[(name, 'resident')]):.4f}, resident enqueue alone (500 iterations, no check) {enq:.4f}")
        lines.append("           windows in order, baseline | resident: " + " ".join(f"{b:.4f}|{r:.4f}" for b, r in zip(ref, res)))
        print(lines[-2], flush=True)
        print(lines[-1], flush=True)
        del opt, base
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
