"""Timing of the Hessian front (xequinet_amd/hessian.py) on one aspirin-shaped molecule (21 atoms) and 64 QM9-shaped molecules, f32 / f64.

    python profiles/hessian_timing.py [--out profiles/hessian_timing.txt]

Forms:
  (a) the reference's procedure (run/geometry.py:59-99): model.train(), one force evaluation with its graph kept, one autograd.grad per
      force component (3 N passes).  The training pass it runs on is the parent commit's, unchanged here.  On the 64-molecule batch only
      the first 48 of its 3 N passes are run and the total is extrapolated from their mean.
  (b) hessian(replicas=1)
  (c) hessian() with the default replicas, plus a sweep of the atom budget behind that default
  (d) (c) with the edge kernel off (training.NATIVE_EDGE = False)
Every shape is warmed up; a device synchronise ends each timed window.  Wall time is the best of --repeats windows; launches are counted
by the library's own counter (xeq_* entry points) and, where the profiler is available, as all device kernels of one call; peak memory is
the caching allocator's high-water mark of one call.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import xpainn_oracle as orc  # noqa: E402
from xequinet_amd import hessian as hz  # noqa: E402
from xequinet_amd import keys, lib  # noqa: E402
from xequinet_amd.data import synthetic as syn  # noqa: E402
from xequinet_amd.nn import resolve_model, training  # noqa: E402

DEV = "cuda"
SAMPLE_PASSES = 48


def batch(name, dtype):
    pos, z, ptr = syn.synth_aspirin() if name == "aspirin" else syn.synth_qm9_batch(64, seed=5)
    ei = orc.radius_graph_canonical(pos, ptr, 5.0)
    b = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
    return {"pos": torch.tensor(pos, dtype=dtype, device=DEV), "atomic_numbers": torch.tensor(z.astype(np.int64), device=DEV),
            "edge_index": torch.tensor(ei, device=DEV), "batch": torch.tensor(b, device=DEV), "ptr": torch.tensor(ptr, device=DEV)}


def reference_procedure(model, data, max_passes=None):
    """-> (rows done, seconds of the passes alone): the loop of calc_analytical_hessian."""
    data = {k: v.clone() for k, v in data.items()}
    model.train().requires_grad_(True)
    out = model(data, compute_forces=True, compute_virial=False)
    grad = -out[keys.FORCES]
    pos = data[keys.POSITIONS]
    n = pos.shape[0]
    H = torch.zeros((n, n, 3, 3), dtype=pos.dtype, device=pos.device)
    rows = [(i, j) for i in range(n) for j in range(3)][:max_passes]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i, j in rows:
        H[i, :, j, :] = torch.autograd.grad(grad[i, j], pos, retain_graph=True)[0]
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    model.eval().requires_grad_(False)
    return len(rows), dt


def timed(fn, repeats):
    fn()
    fn()        # warm-up: allocator, packed weights, library handles
    best = float("inf")
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    torch.cuda.reset_peak_memory_stats()
    first = lib.launch_count()
    fn()
    torch.cuda.synchronize()
    own = lib.launch_count() - first
    peak = torch.cuda.max_memory_allocated()
    kernels = None
    try:
        from torch.profiler import ProfilerActivity, profile

        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        kernels = sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA"))
    except Exception as exc:      # the profiler is optional: the library's own count stands
        kernels = f"n/a ({type(exc).__name__})"
    return best, own, kernels, peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "hessian_timing.txt"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--budgets", type=int, nargs="*", default=[256, 1024, 4096, 8192, 16384, 32768])
    args = ap.parse_args()
    lines = [f"hessian_timing.py on {torch.cuda.get_device_name(0)}; XPaiNN default configuration (3 blocks, 128x0e + 64x1o + 32x2e, 20 Bessel functions)",
             f"best of {args.repeats} windows after two warm-up calls; ATOM_BUDGET at the time of the run: {hz.ATOM_BUDGET}", ""]

    def say(s):
        print(s, flush=True)
        lines.append(s)

    default_budget = hz.ATOM_BUDGET
    for dtype in (torch.float32, torch.float64):
        torch.manual_seed(0)
        model = resolve_model("xpainn").to(dtype).to(DEV).eval().requires_grad_(False)
        for name in ("aspirin", "qm9 x 64"):
            data = batch(name, dtype)
            n = data["pos"].shape[0]
            cols = 3 * int((data["ptr"][1:] - data["ptr"][:-1]).max())
            say(f"== {name}, {str(dtype).split('.')[-1]}: {n} atoms, {data['edge_index'].shape[1]} edges, {cols} columns ==")
            sample = None if name == "aspirin" else SAMPLE_PASSES
            reference_procedure(model, data, 6)
            done, dt = reference_procedure(model, data, sample)
            total = dt * (3 * n) / done
            note = "" if done == 3 * n else f" (extrapolated from {done} passes)"
            say(f"(a) reference procedure, {3 * n} passes: {total * 1e3:9.1f} ms{note}; {dt / done * 1e3:.2f} ms per pass")
            t_a = total
            results = {}
            for label, kw, native in (("(b) replicas=1", dict(replicas=1), True), ("(c) default replicas", {}, True),
                                      ("(d) default replicas, edge kernel off", {}, False)):
                training.NATIVE_EDGE = native
                R = hz.default_replicas(n, cols) if "replicas" not in kw else kw["replicas"]
                passes = len(hz.pass_plan(cols, R))
                best, own, kernels, peak = timed(lambda: hz.hessian(model, data, **kw), args.repeats)
                training.NATIVE_EDGE = True
                results[label[:3]] = best
                per_pass = kernels / passes if isinstance(kernels, int) else kernels
                say(f"{label}: R={R}, {passes} passes: {best * 1e3:9.1f} ms; library launches {own} ({own / passes:.0f} per pass incl. the first order), "
                    f"device kernels {kernels} ({per_pass if isinstance(per_pass, str) else format(per_pass, '.0f')} per pass); peak memory {peak / 2**20:.0f} MiB; "
                    f"(a) / this = {t_a / best:.1f}")
            say(f"share of a default call that the edge kernel removes: (d) - (c) = {(results['(d)'] - results['(c)']) * 1e3:.1f} ms = "
                f"{100 * (results['(d)'] - results['(c)']) / results['(d)']:.0f} % of (d)")
            for budget in args.budgets:
                hz.ATOM_BUDGET = budget
                R = hz.default_replicas(n, cols)
                best, own, kernels, peak = timed(lambda: hz.hessian(model, data), max(1, args.repeats - 1))
                say(f"    budget {budget:6d}: R={R:3d}, {len(hz.pass_plan(cols, R)):3d} passes: {best * 1e3:9.1f} ms, peak memory {peak / 2**20:.0f} MiB")
            hz.ATOM_BUDGET = default_budget
            say("")
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
