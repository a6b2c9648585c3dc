"""Time one energy + force evaluation of PaiNN on a qm9_1024-shape batch (neighbour list given): the native kernels, the same model
through its tensor form (ATen) on the same card, and XPaiNN on the same batch for scale.

    python profiles/painn_timing.py [out_file]

Ten warm-up evaluations, then the median and the spread of 9 groups of 5 evaluations between device events.  Writes
profiles/painn_timing.txt (or out_file) with the commit hash.  The one condition: the native path is not slower than the tensor form."""
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from xequinet_amd.data import NeighborTransform, XequiBatch  # noqa: E402
from xequinet_amd.data import synthetic as syn  # noqa: E402
from xequinet_amd.nn import resolve_model  # noqa: E402
from xequinet_amd.nn import painn  # noqa: E402


def measure(fn, warmup=10, groups=9, per_group=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(groups):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(per_group):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / per_group)
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def main():
    out_file = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "painn_timing.txt")
    torch.manual_seed(0)
    pos, z, ptr = syn.synth_qm9_batch(1024, seed=0)
    model = resolve_model("painn").cuda().eval().requires_grad_(False)
    xmodel = resolve_model("xpainn").cuda().eval().requires_grad_(False)
    batch = XequiBatch(torch.tensor(pos, dtype=torch.float32), torch.tensor(z), torch.tensor(ptr)).to("cuda")
    data = NeighborTransform(model.cutoff_radius)(batch).to_dict()

    def run(m):
        with torch.enable_grad():
            return m(dict(data), compute_forces=True)

    native = measure(lambda: run(model))
    ref = run(model)
    painn_native_supported = painn.native_supported
    painn.native_supported = lambda *a, **k: False   # the same model through its tensor form
    try:
        aten = measure(lambda: run(model))
        alt = run(model)
    finally:
        painn.native_supported = painn_native_supported
    xp = measure(lambda: run(xmodel))
    try:
        commit = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or "unknown"
    except OSError:
        commit = "unknown"
    lines = [
        f"commit {commit}",
        f"device {torch.cuda.get_device_name(0)}; qm9_1024 shape: {len(z)} atoms, {data['edge_index'].shape[1]} edges; energy + forces, neighbour list given",
        "ms per evaluation: median (min .. max) of 9 groups of 5, after 10 warm-up evaluations",
        f"PaiNN native kernels   {native[0]:8.3f} ({native[1]:.3f} .. {native[2]:.3f})",
        f"PaiNN tensor form ATen {aten[0]:8.3f} ({aten[1]:.3f} .. {aten[2]:.3f})",
        f"XPaiNN (for scale)     {xp[0]:8.3f} ({xp[1]:.3f} .. {xp[2]:.3f})",
        f"max |F native - F tensor form| = {float((ref['forces'] - alt['forces']).abs().max()):.3e}",
        f"native not slower than the tensor form: {native[0] <= aten[0]}",
    ]
    with open(out_file, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
