"""Time of the batched harmonic analysis (xequinet_amd/vibrations.py) against what a user of ``hessian()`` could do before it on the same
device with the same matrices.

    python profiles/vib_timing.py [--out profiles/vib_timing.txt] [--repeats 7] [--molecules 1024]

Systems: synthetic Hessians m^1/2 U diag(lambda) U^T m^1/2 (random orthogonal U, fixed seed) on the size distribution and geometries of
``data/synthetic.synth_qm9_batch(1024)`` (3 n from 9 to 87), and a single aspirin (3 n = 63).  Measured, each between two device events
around calls that end enqueued on one stream, after two warm-up calls, ``--repeats`` windows, median (min .. max) in ms:

  analysis     ``harmonic_analysis`` whole: the packing of the blocks, three launches, the one read-back
  eigh         xeq_vib_eigh alone on the M matrices of that call, as ONE launch whose LDS is sized by the largest matrix
  eigh split   the same matrices as up to three launches by LDS footprint (3 n <= 32, <= 64, <= 96): the A/B of a size-class split
  padded       the projection as batched tensor operations on the [G, 87, 87] zero-padded f64 batch (mass weighting, the six rigid-body
               vectors, batched QR, P S P + sigma Q Q^T by batched products, pad rows shifted above sigma) and ONE batched torch.linalg.eigh
  padded eigh  that torch.linalg.eigh alone
  loop         torch.linalg.eigh once per graph on the ragged M matrices (the projection not counted)
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from xequinet_amd import lib, vibrations  # noqa: E402
from xequinet_amd.data import synthetic as syn  # noqa: E402

DEV = "cuda"
AMU = {1: 1.008, 6: 12.011, 7: 14.007, 8: 15.999, 9: 18.998}
UNITS = dict(energy_unit="eV", length_unit="Angstrom")


def hessians_of(pos, z, ptr, seed=0):
    rng = np.random.default_rng(seed)
    mass = np.array([AMU.get(int(v), 12.011) for v in z])
    blocks = []
    for a, b in zip(ptr[:-1], ptr[1:]):
        n = int(b - a)
        m = 3 * n
        U = np.linalg.qr(rng.standard_normal((m, m)))[0]
        lam = 0.05 + 0.95 * (np.arange(m) + 0.3 * rng.random(m)) / m
        w = np.sqrt(np.repeat(mass[a:b], 3))
        S = (U * lam) @ U.T
        F = 0.5 * (S + S.T) * np.outer(w, w)
        blocks.append(torch.tensor(F.reshape(n, 3, n, 3).transpose(0, 2, 1, 3).copy(), device=DEV))
    return blocks, torch.tensor(pos, dtype=torch.float64, device=DEV), torch.tensor(mass, device=DEV)


def windows(fn, repeats):
    for _ in range(2):
        fn()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return out


def fmt(v):
    return f"{np.median(v):9.3f} ({min(v):.3f} .. {max(v):.3f})"


def eigh_launches(M, mat_off, dims, classes):
    """xeq_vib_eigh on the flat M of a project call: one launch per non-empty class of dimensions (lo, hi]."""
    out = []
    w = torch.empty(int(sum(dims)), dtype=torch.float64, device=DEV)
    v = torch.empty_like(M)
    val_off = np.concatenate([[0], np.cumsum(dims)])[:-1]
    for lo, hi in classes:
        sel = [g for g, d in enumerate(dims) if lo < d <= hi]
        if not sel:
            continue
        t = lambda a, dt=torch.int64: torch.tensor(np.asarray(a)[sel], dtype=dt, device=DEV)
        out.append((t(mat_off[:-1]), t(val_off), t(dims, torch.int32), len(sel), max(dims[g] for g in sel),
                    torch.zeros(len(sel), dtype=torch.int32, device=DEV), torch.zeros(len(sel), dtype=torch.int32, device=DEV)))

    def run():
        for mo, vo, dm, n, top, sw, st in out:
            lib.call("xeq_vib_eigh", lib.ptr(M), lib.ptr(mo), lib.ptr(vo), lib.ptr(dm), n, top, lib.ptr(w), lib.ptr(v), lib.ptr(sw), lib.ptr(st), lib.stream())

    return run, out, w


def project(blocks, pos, mass):
    """The M matrices of the batch by the library's own projection (what ``harmonic_analysis`` hands its solver), flat + offsets."""
    sizes = [int(b.shape[0]) for b in blocks]
    dims = [3 * n for n in sizes]
    ptr = np.concatenate([[0], np.cumsum(sizes)])
    mat_off = np.concatenate([[0], np.cumsum([d * d for d in dims])])
    hess_off = np.concatenate([[0], np.cumsum([9 * n * n for n in sizes])])
    G, N = len(sizes), int(ptr[-1])
    f64 = dict(dtype=torch.float64, device=DEV)
    M, q, work = torch.empty(int(mat_off[-1]), **f64), torch.empty(18 * N, **f64), torch.empty(18 * N, **f64)
    i32 = dict(dtype=torch.int32, device=DEV)
    keep = [torch.zeros((G, 3), **f64), torch.zeros((G, 9), **f64), torch.zeros(G, **f64), torch.zeros(G, **i32), torch.zeros(G, **i32), torch.zeros(G, **f64)]
    t = lambda a: torch.tensor(a, dtype=torch.int64, device=DEV)
    # every argument tensor has a name until the synchronise: a temporary would be freed, and its memory handed out again, before the launch
    flat, d_hess_off, d_ptr, d_mat_off = torch.cat([b.reshape(-1) for b in blocks]), t(hess_off[:-1]), t(ptr), t(mat_off[:-1])
    lib.call("xeq_vib_project", lib.XEQ_F64, lib.ptr(flat), lib.ptr(d_hess_off), lib.ptr(pos), lib.ptr(mass), lib.ptr(d_ptr), G, 0, lib.ptr(d_mat_off),
             lib.ptr(M), lib.ptr(q), lib.ptr(work), *[lib.ptr(k) for k in keep], lib.stream())
    torch.cuda.synchronize()
    del flat, d_hess_off, d_ptr, d_mat_off
    return M, mat_off, dims, ptr


def padded_inputs(blocks, pos, mass, ptr, pad):
    G = len(blocks)
    H = torch.zeros((G, pad, pad), dtype=torch.float64, device=DEV)
    P = torch.zeros((G, pad // 3, 3), dtype=torch.float64, device=DEV)
    W = torch.zeros((G, pad // 3), dtype=torch.float64, device=DEV)
    for g, b in enumerate(blocks):
        n = b.shape[0]
        H[g, : 3 * n, : 3 * n] = b.permute(0, 2, 1, 3).reshape(3 * n, 3 * n)
        P[g, :n] = pos[ptr[g] : ptr[g + 1]]
        W[g, :n] = mass[ptr[g] : ptr[g + 1]]
    return H, P, W


def padded_analysis(H, P, W):
    """The projection and ONE batched eigh as tensor operations; pad rows (mass 0) are pushed above sigma."""
    G, pad, _ = H.shape
    real = (W > 0).repeat_interleave(3, dim=1)
    w3 = W.repeat_interleave(3, dim=1)
    inv = torch.where(real, w3.clamp_min(1e-300).rsqrt(), torch.zeros_like(w3))
    S = 0.5 * (H + H.transpose(1, 2)) * inv[:, :, None] * inv[:, None, :]
    com = (W[:, :, None] * P).sum(1) / W.sum(1, keepdim=True)
    r = (P - com[:, None, :]) * (W > 0)[:, :, None]
    sm = W.sqrt()
    eye = torch.eye(3, dtype=H.dtype, device=H.device)
    trans = (sm[:, :, None, None] * eye[None, None]).reshape(G, pad, 3)                       # [G, 3 n, 3]: column a = translation along a
    rot = torch.stack([torch.linalg.cross(eye[a].expand_as(r), r) * sm[:, :, None] for a in range(3)], dim=-1).reshape(G, pad, 3)
    Q = torch.linalg.qr(torch.cat([trans, rot], dim=2)).Q                                      # [G, pad, 6]
    QQt = Q @ Q.transpose(1, 2)
    Pm = torch.eye(pad, dtype=H.dtype, device=H.device)[None] - QQt
    PSP = Pm @ S @ Pm
    sigma = 2.0 * torch.linalg.matrix_norm(PSP)
    M = PSP + sigma[:, None, None] * QQt + torch.diag_embed(torch.where(real, torch.zeros_like(w3), 2.0 * sigma[:, None].expand_as(w3)))
    return torch.linalg.eigh(M), M


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--molecules", type=int, default=1024)
    args = ap.parse_args()
    lines = [f"vib_timing.py on {torch.cuda.get_device_name(0)}; ms per call between two device events, median (min .. max) of {args.repeats} windows after "
             "two warm-up calls; f64 throughout"]
    for name in ("qm9", "aspirin"):
        pos, z, ptr = syn.synth_qm9_batch(args.molecules, seed=1234) if name == "qm9" else syn.synth_aspirin()
        blocks, dpos, dmass = hessians_of(pos, z, ptr)
        G = len(blocks)
        res = vibrations.harmonic_analysis(blocks, dpos, dmass, **UNITS)
        sweeps = res.sweeps.cpu().numpy()
        M, mat_off, dims, aptr = project(blocks, dpos, dmass)
        lines.append(f"== {name}: {G} graphs, {int(aptr[-1])} atoms, 3 n from {min(dims)} to {max(dims)} (mean {np.mean(dims):.1f}); "
                     f"sweeps {int(sweeps.min())} .. {int(sweeps.max())} (mean {sweeps.mean():.2f}) ==")
        one, _, w_one = eigh_launches(M, mat_off, dims, [(0, 96)])
        split, parts, w_split = eigh_launches(M, mat_off, dims, [(0, 32), (32, 64), (64, 96)])
        one()
        split()
        torch.cuda.synchronize()
        same = bool(torch.equal(w_one, w_split))
        t_all = windows(lambda: vibrations.harmonic_analysis(blocks, dpos, dmass, **UNITS), args.repeats)
        t_one, t_split = [], []
        for k in range(args.repeats):                    # the two forms take turns
            t_one += windows(one, 1) if k % 2 == 0 else []
            t_split += windows(split, 1)
            t_one += windows(one, 1) if k % 2 == 1 else []
        pad = max(dims)
        Hp, Pp, Wp = padded_inputs(blocks, dpos, dmass, aptr, pad)
        (wp, _), Mp = padded_analysis(Hp, Pp, Wp)
        worst = 0.0
        for g in range(G):
            k = dims[g] - 6
            worst = max(worst, float((wp[g, :k] - res.eigenvalues(g)).abs().max()))
        t_pad = windows(lambda: padded_analysis(Hp, Pp, Wp), args.repeats)
        t_pad_eigh = windows(lambda: torch.linalg.eigh(Mp), args.repeats)
        mats = [M[mat_off[g] : mat_off[g + 1]].view(dims[g], dims[g]) for g in range(G)]
        t_loop = windows(lambda: [torch.linalg.eigh(a) for a in mats], max(3, args.repeats // 2))
        lines += [f"analysis     {fmt(t_all)}   (3 launches: xeq_vib_project, xeq_vib_eigh, xeq_vib_finish, and the host's packing and read-back)",
                  f"eigh         {fmt(t_one)}   one launch, LDS for 3 n = {max(dims)}",
                  f"eigh split   {fmt(t_split)}   {len(parts)} launches of {[p[3] for p in parts]} matrices up to {[p[4] for p in parts]}; same eigenvalue bits as one launch: {same}",
                  f"padded       {fmt(t_pad)}   tensor projection + one batched torch.linalg.eigh on [{G}, {pad}, {pad}]; max |eigenvalue - analysis| {worst:.2e}",
                  f"padded eigh  {fmt(t_pad_eigh)}   that torch.linalg.eigh alone",
                  f"loop         {fmt(t_loop)}   {G} calls of torch.linalg.eigh on the ragged matrices",
                  f"ratios of medians: padded / analysis {np.median(t_pad) / np.median(t_all):.2f}, padded eigh / eigh {np.median(t_pad_eigh) / np.median(t_one):.2f}, "
                  f"loop / analysis {np.median(t_loop) / np.median(t_all):.2f}, eigh / eigh split {np.median(t_one) / np.median(t_split):.2f}"]
        if name == "aspirin":
            lines.append("next to it: the f32 Hessian of aspirin by hessian() takes 10.1 ms (profiles/hessian_timing.txt, (c) default replicas)")
        for ln in lines[-9:]:
            print(ln, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
