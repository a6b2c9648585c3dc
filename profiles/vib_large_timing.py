"""Time of ``harmonic_analysis(..., large="kernel")`` (xeq_vib_eigh_large: one launch for every graph with 96 < 3 n <= 768) against
``large="tensor"`` (one ``torch.linalg.eigh`` per such graph: the default, and all there was before the keyword) on the same Hessians.

    python profiles/vib_large_timing.py [--out profiles/vib_large_timing.txt] [--repeats 5]

Systems: synthetic molecules (random geometries, H / C / N / O masses) with Hessians m^1/2 U diag(lambda) U^T m^1/2 (random orthogonal
U, lambda between 0.05 and 1, fixed seeds): 1 024 molecules of 33 to 64 atoms, 256 molecules of 100 atoms, one 192-atom box (3 n = 576,
analysed as periodic) and one 33-atom molecule.  Measured, each between two device events around calls that end in the analysis' own
read-back, after two warm-up calls of each form, ``--repeats`` windows per form with the two forms taking turns, median (min .. max) in ms:

  kernel       ``harmonic_analysis(..., large="kernel")`` whole: packing, three launches, the one read-back
  tensor       ``harmonic_analysis(..., large="tensor")`` whole: packing, two launches, a torch.linalg.eigh and five tensor operations
               per graph, the one read-back
  eigh_large   xeq_vib_eigh_large alone on the M matrices of that call (longest first, as the analysis launches it)
  eigh loop    torch.linalg.eigh alone, once per graph, on the same matrices

and the largest relative difference of a wavenumber between the two forms (the results must not change with the solver).  The last
column of eigh_large is a rate by ESTIMATE, not a counter: 16 m^3 bytes for the reduction and the accumulation of Q (each reads the
block once for the product and reads and writes it once for the update, over blocks of 1 .. m) plus 16 m bytes per rotation of two
rows of Q^T, the rotations counted as 1.7 m QL iterations over half the rows on average (13.6 m^3), over the kernel's time.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from vib_timing import fmt, project, windows  # noqa: E402
from xequinet_amd import lib, vibrations  # noqa: E402

DEV = "cuda"
MASSES = np.array([1.008, 12.011, 14.007, 15.999])
UNITS = dict(energy_unit="eV", length_unit="Angstrom")


def molecules(sizes, seed):
    """(blocks [n, n, 3, 3] on the device, pos [N, 3], mass [N]) of synthetic molecules of the given atom counts."""
    rng = np.random.default_rng(seed)
    blocks, pos, mass = [], [], []
    for n in sizes:
        m = 3 * n
        ms = MASSES[rng.integers(0, 4, n)]
        U = np.linalg.qr(rng.standard_normal((m, m)))[0]
        lam = 0.05 + 0.95 * (np.arange(m) + 0.3 * rng.random(m)) / m
        w = np.sqrt(np.repeat(ms, 3))
        S = (U * lam) @ U.T
        F = 0.5 * (S + S.T) * np.outer(w, w)
        blocks.append(torch.tensor(F.reshape(n, 3, n, 3).transpose(0, 2, 1, 3).copy(), device=DEV))
        pos.append(1.5 * n ** (1.0 / 3.0) * rng.standard_normal((n, 3)))
        mass.append(ms)
    return blocks, torch.tensor(np.concatenate(pos), dtype=torch.float64, device=DEV), torch.tensor(np.concatenate(mass), device=DEV)


def eigh_large_launch(M, mat_off, dims):
    """xeq_vib_eigh_large on the flat M of a project call, longest first."""
    order = sorted(range(len(dims)), key=lambda g: -dims[g])
    val_off = np.concatenate([[0], np.cumsum(dims)])[:-1]
    t = lambda a, dt=torch.int64: torch.tensor(np.asarray(a)[order], dtype=dt, device=DEV)
    mo, vo, dm = t(mat_off[:-1]), t(val_off), t(dims, torch.int32)
    w, v = torch.empty(int(sum(dims)), dtype=torch.float64, device=DEV), torch.empty_like(M)
    sw, st = torch.zeros(len(dims), dtype=torch.int32, device=DEV), torch.zeros(len(dims), dtype=torch.int32, device=DEV)

    def run():
        lib.call("xeq_vib_eigh_large", lib.ptr(M), lib.ptr(mo), lib.ptr(vo), lib.ptr(dm), len(dims), max(dims), lib.ptr(w), lib.ptr(v), lib.ptr(sw), lib.ptr(st),
                 lib.stream())

    return run, (mo, vo, dm, w, v, sw, st)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    rng = np.random.default_rng(2024)
    cases = [("1024 molecules of 33 to 64 atoms", [int(n) for n in rng.integers(33, 65, 1024)], False),
             ("256 molecules of 100 atoms", [100] * 256, False),
             ("one 192-atom box", [192], True),
             ("one 33-atom molecule", [33], False)]
    lines = [f"vib_large_timing.py on {torch.cuda.get_device_name(0)}; ms per call between two device events, median (min .. max) of {args.repeats} windows per form, "
             "the forms taking turns, after two warm-up calls of each; f64 throughout"]
    for c, (name, sizes, periodic) in enumerate(cases):
        blocks, pos, mass = molecules(sizes, 500 + c)
        kw = dict(UNITS, periodic=periodic)
        forms = {large: (lambda large=large: vibrations.harmonic_analysis(blocks, pos, mass, large=large, **kw)) for large in ("kernel", "tensor")}
        res = {large: fn() for large, fn in forms.items()}
        assert set(res["kernel"].solver) == {"large"} and set(res["tensor"].solver) == {"tensor"}
        worst = float(((res["kernel"].freq_wavenumber - res["tensor"].freq_wavenumber).abs() / res["tensor"].freq_wavenumber.abs()).max())
        sweeps = res["kernel"].sweeps.cpu().numpy()
        for fn in forms.values():
            fn()
        times = {large: [] for large in forms}
        for k in range(args.repeats):
            for large in (("kernel", "tensor") if k % 2 == 0 else ("tensor", "kernel")):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                a.record()
                forms[large]()
                b.record()
                torch.cuda.synchronize()
                times[large].append(a.elapsed_time(b))
        M, mat_off, dims, aptr = project(blocks, pos, mass)            # (the translations-only projection of the box is not needed for a time)
        run, keep = eigh_large_launch(M, mat_off, dims)
        mats = [M[mat_off[g] : mat_off[g + 1]].view(dims[g], dims[g]) for g in range(len(dims))]
        loop = lambda: [torch.linalg.eigh(a) for a in mats]
        t_k, t_l = [], []
        run(), loop()
        for k in range(args.repeats):
            t_k += windows(run, 1) if k % 2 == 0 else []
            t_l += windows(loop, 1)
            t_k += windows(run, 1) if k % 2 == 1 else []
        model = sum(29.6 * float(d) ** 3 for d in dims)
        lines += [f"== {name}: {len(sizes)} graphs, {int(aptr[-1])} atoms, 3 n from {min(dims)} to {max(dims)} (mean {np.mean(dims):.1f}); most QL iterations of one "
                  f"eigenvalue {int(sweeps.min())} .. {int(sweeps.max())} ==",
                  f"kernel       {fmt(times['kernel'])}   large=\"kernel\": xeq_vib_project, xeq_vib_eigh_large, xeq_vib_finish, packing and read-back",
                  f"tensor       {fmt(times['tensor'])}   large=\"tensor\": xeq_vib_project, {len(sizes)} x torch.linalg.eigh and its tensor operations, xeq_vib_finish",
                  f"eigh_large   {fmt(t_k)}   the launch alone; {model / 1e9:.2f} GB by the estimate: {model / 1e6 / np.median(t_k):.0f} GB/s over {len(sizes)} workgroups",
                  f"eigh loop    {fmt(t_l)}   {len(sizes)} calls of torch.linalg.eigh alone",
                  f"ratios of medians: tensor / kernel {np.median(times['tensor']) / np.median(times['kernel']):.2f}, eigh loop / eigh_large {np.median(t_l) / np.median(t_k):.2f}; "
                  f"largest relative difference of a wavenumber between the forms {worst:.2e}"]
        for ln in lines[-6:]:
            print(ln, flush=True)
        del keep
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
