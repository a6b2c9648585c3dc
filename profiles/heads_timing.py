"""Workload of profiles/heads_timing.txt: one QM9-1024-shape batch (neighbour list given), energy + forces, f32, for

    python profiles/heads_timing.py energy        XPaiNN(output_modes=["energy"])
    python profiles/heads_timing.py polar         XPaiNN(output_modes=["energy", "polar"]) on the head kernels
    python profiles/heads_timing.py polar-tensor  the same model with PolarOut forced to its tensor form on the same f32 inputs

Ten warm-up evaluations, then the median of 9 groups of 5 evaluations between device events (printed as one line).  Run it under
`rocprofv3 --kernel-trace --stats -- python profiles/heads_timing.py polar` for the per-kernel times."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from xequinet_amd.data import NeighborTransform, XequiBatch  # noqa: E402
from xequinet_amd.data import synthetic as syn  # noqa: E402
from xequinet_amd.nn import resolve_model  # noqa: E402


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "polar"
    torch.manual_seed(0)
    modes = ["energy"] if mode == "energy" else ["energy", "polar"]
    model = resolve_model("xpainn", output_modes=modes).to("cuda").eval().requires_grad_(False)
    if mode == "polar-tensor":
        head = model.mods["output_polar"]
        head._kernel_ok = lambda s, x, data: False
    pos, z, ptr = syn.synth_qm9_batch(1024, seed=0)
    batch = NeighborTransform(model.cutoff_radius)(XequiBatch(torch.tensor(pos, dtype=torch.float32), torch.tensor(z), torch.tensor(ptr)).to("cuda"))
    data = batch.to_dict()

    def step():
        with torch.enable_grad():
            return model(dict(data), compute_forces=True, compute_virial=False)

    for _ in range(10):
        step()
    torch.cuda.synchronize()
    ms = []
    for _ in range(9):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(5):
            step()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / 5)
    print(f"heads_timing {mode}: nodes {int(ptr[-1])} median {np.median(ms):.3f} ms (min {min(ms):.3f}, max {max(ms):.3f}) per eager evaluation")


if __name__ == "__main__":
    main()
