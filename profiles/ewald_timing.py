"""Time one EwaldBlock (node_dim 128), forward plus the force reverse pass (dL/dpos and dL/ds of a random cotangent), in its kernel
form (csrc/xeq_ewald.hip) against the tensor form of the same module (the reference's op sequence on device tensor operations) on
the same GPU, with the peak device memory of each:

    python profiles/ewald_timing.py > profiles/ewald_timing.txt

Workloads: the QM9-1024 batch (non-periodic, K = 13, 1024 graphs of ~18 atoms) and the 1 536-atom water box (periodic, [3, 3, 3]:
K = 171, ONE graph: the parallelism of the structure factor comes from its 24 atom chunks and 6 k-tiles only).  Device events around
a window of about one second of evaluations after the warm-up ones; the two forms alternate; three repeats to show the spread.  No threshold: a record."""
import numpy as np
import torch

from xequinet_amd import keys
from xequinet_amd.data import synthetic as syn
from xequinet_amd.nn.ewald import EwaldBlock, EwaldInitialNonPBC, EwaldInitialPBC

DEV = "cuda"
F = 128


def workload(name):
    if name == "qm9_1024":
        pos, z, ptr = syn.synth_qm9_batch(1024)
        return EwaldInitialNonPBC(0.4, 0.2, 20), pos, ptr, None
    pos, z, ptr, cell = syn.synth_water_box(8, seed=5)
    return EwaldInitialPBC([3, 3, 3]), pos, ptr, np.asarray(cell, dtype=np.float32).reshape(1, 3, 3)


def evaluate(block, init, s, pos, ptr, batch, cell, probe):
    s = s.clone().requires_grad_(True)
    pos = pos.clone().requires_grad_(True)
    data = {keys.BATCH: batch, keys.BATCH_PTR: ptr, keys.NODE_INVARIANT: s, keys.POSITIONS: pos}
    if cell is not None:
        data[keys.CELL] = cell
    out = block(init(data))[keys.NODE_INVARIANT]
    return (out,) + torch.autograd.grad((out * probe).sum(), [s, pos])


def timed(fn, warmup=5, window_s=1.0):
    """ms per evaluation over a window of about `window_s` seconds of device time (sized from a first short run), and the peak memory."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(5):
        fn()
    b.record()
    torch.cuda.synchronize()
    iters = max(10, int(window_s * 1e3 / max(a.elapsed_time(b) / 5, 1e-3)))
    torch.cuda.reset_peak_memory_stats()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters, torch.cuda.max_memory_allocated() / 2**20


def main():
    print(f"device: {torch.cuda.get_device_name(0)}; EwaldBlock(node_dim={F}), f32, forward + reverse (dL/ds, dL/dpos)")
    for name in ("qm9_1024", "water_1536"):
        torch.manual_seed(0)
        init, pos, ptr, cell = workload(name)
        block = EwaldBlock(node_dim=F).to(DEV).eval().requires_grad_(False)
        with torch.no_grad():
            block.up.weight.mul_(100.0)
        init = init.to(DEV).eval().requires_grad_(False)
        n = pos.shape[0]
        ptr_t = torch.tensor(ptr, device=DEV)
        batch = torch.repeat_interleave(torch.arange(len(ptr) - 1, device=DEV), ptr_t[1:] - ptr_t[:-1])
        pos_t = torch.tensor(pos, dtype=torch.float32, device=DEV)
        cell_t = None if cell is None else torch.tensor(cell, device=DEV)
        s, probe = torch.randn(n, F, device=DEV), torch.randn(n, F, device=DEV)
        K = (init.k_grid if cell is None else init.k_index_product_set).shape[0]
        base = torch.cuda.memory_allocated() / 2**20
        results = {}
        for form in ("kernel", "tensor"):
            init.kernel_consumers = form == "kernel"
            results[form] = evaluate(block, init, s, pos_t, ptr_t, batch, cell_t, probe)
        diff = [float((a - b).abs().max()) for a, b in zip(results["kernel"], results["tensor"])]
        scale = [float(b.abs().max()) for b in results["tensor"]]
        print(f"\n{name}: {n} atoms, {len(ptr) - 1} graphs, K = {K}; [n, K, F] tensor = {n * K * F * 4 / 2**20:.0f} MiB; resident before: {base:.0f} MiB")
        print(f"  kernel form vs tensor form, max |diff| (out, dL/ds, dL/dpos): {diff[0]:.2e} {diff[1]:.2e} {diff[2]:.2e}  (max |value| {scale[0]:.2e} {scale[1]:.2e} {scale[2]:.2e})")
        for rep in range(3):
            row = []
            for form in ("kernel", "tensor"):
                init.kernel_consumers = form == "kernel"
                ms, peak = timed(lambda: evaluate(block, init, s, pos_t, ptr_t, batch, cell_t, probe))
                row.append(f"{form} {ms:8.3f} ms  peak {peak:7.0f} MiB")
            print(f"  repeat {rep}: " + "   ".join(row))


if __name__ == "__main__":
    main()
