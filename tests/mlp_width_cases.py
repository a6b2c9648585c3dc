"""Cases and f64 / f32 restatements for the two-layer MLP kernels at a run-time hidden width (xeq_mlp2h_fwd / _bwd, csrc/xeq_mlp.hip).
CPU only; no test functions here.  tests/test_gpu_mlp_widths.py runs them on the GPU, tests/test_mlp_width_cases_host.py checks the
predicate table and the POWER of the comparison on the host.

A case is (hidden H, k1, n2, n rows): the first n rows of one master draw per (H, k1, n2), so a row means the same numbers whatever the
row count.  Every input is drawn in f64 and rounded to f32 once: the kernels, the f32 restatement and the f64 reference see the same
numbers.  x, g ~ N(0, 1); W1 ~ N(0, 1) / sqrt(k1), W2 ~ N(0, 1) / sqrt(H); b1, b2 ~ N(0, 1/4), so that a lost bias group is O(1/2).

  forward   pre = x W1^T + b1,  y = silu(pre) W2^T + b2
  reverse   gx  = ((g W2) * silu'(pre)) W1                   (pre: the forward's; the GPU test hands over what the forward kernel saved)

Bound per output tensor: the project's rule, max(1e-4 max(1, max|ref|), 1.5 err32), err32 = |f32 restatement - f64 reference| on the
rows of the case (tests/test_gpu_painn.py::_bound)."""
import functools
from types import SimpleNamespace

import numpy as np
import torch

WIDTHS = (32, 64, 96, 160, 192, 224, 256)          # the new widths (128 is xeq_mlp2_fwd / _bwd itself)
ROWS = (1, 15, 16, 17, 31, 32, 33, 65)
# The new widths have ONE row form (32 rows per workgroup).  What changes with the row count is how TileSplit (csrc/xeq_common.h) deals
# row tiles to workgroups: up to 128 tiles every tile is shared by several workgroups, from 129 on (n >= 4097) a tile has one workgroup,
# and a short last round (tiles % 256 in 1 .. 128: n = 8200 is 257 tiles) is shared again.  One n on each side of each.
THRESHOLD_ROWS = (4096, 4097, 8192, 8200)
ROWS_MAX = {H: (max(THRESHOLD_ROWS) if H in (32, 256) else 300) for H in WIDTHS + (128,)}
OUTPUTS = ("pre", "y", "gx")


def stacks(H):
    """PaiNN's two stacks at node_dim H: scalar_mlp (H -> H -> 3H) and update_mlp (2H -> H -> 3H)."""
    return ((H, 3 * H), (2 * H, 3 * H))


# (k1, hidden, n2) the predicate admits / refuses, with dtype F32 unless stated
SUPPORTED = tuple((k1, H, n2) for H in range(32, 257, 32) for k1, n2 in ((H, 3 * H), (2 * H, 3 * H), (H, H + 2 * 128)))
REFUSED = (("hidden 0", 0, 64, 0, 192), ("hidden 16", 0, 64, 16, 192), ("hidden 48", 0, 64, 48, 192), ("hidden 288", 0, 64, 288, 192),
           ("k1 40", 0, 40, 64, 192), ("n2 144", 0, 64, 64, 144), ("f64", 1, 64, 64, 192))   # (what, dtype code, k1, hidden, n2)


def bound(ref, ref32):
    return max(1e-4 * max(1.0, float(ref.abs().max())), 1.5 * float((ref32.double() - ref).abs().max()))


def _f32(a):
    return torch.tensor(np.asarray(a, dtype=np.float32).astype(np.float64))


def _silu_grad(p):
    sig = torch.sigmoid(p)
    return sig * (1 + p * (1 - sig))


def evaluate(c, dtype, mutation=None):
    """pre, y, gx of the case in ``dtype``.  ``mutation`` restates it with one defect a kernel could have:
      "last_hidden_tile"   the last 32 hidden columns are never formed (pre and the activation are 0 there)
      "bias1" / "bias2"    the bias k-group of that layer is lost
      "swap_hidden_tiles"  hidden tiles 0 and 4 change places on their way into the second product (H >= 160)
      "k1_tail"            the last 32 columns of the input are not read (forward: of x; reverse: of g)
      "last_row"           the last row of every output is not written (reads back as 0)"""
    t = lambda v: v.detach().to(dtype).clone()
    x, g, w1, b1, w2, b2 = (t(getattr(c, k)) for k in ("x", "g", "w1", "b1", "w2", "b2"))
    H = c.H
    xf, gr = x, g
    if mutation == "k1_tail":
        xf, gr = x.clone(), g.clone()
        xf[:, -32:] = 0
        gr[:, -32:] = 0
    pre = xf @ w1.T + (0 if mutation == "bias1" else b1)
    act = torch.nn.functional.silu(pre)
    gh = (gr @ w2) * _silu_grad(x @ w1.T + b1)   # the reverse pass reads the saved (correct) pre
    if mutation == "last_hidden_tile":
        pre, act, gh = pre.clone(), act.clone(), gh.clone()
        pre[:, -32:] = 0
        act[:, -32:] = 0
        gh[:, -32:] = 0
    if mutation == "swap_hidden_tiles":
        assert H >= 160
        perm = torch.arange(H)
        perm[0:32], perm[128:160] = torch.arange(128, 160), torch.arange(0, 32)
        act, gh = act[:, perm], gh[:, perm]
    y = act @ w2.T + (0 if mutation == "bias2" else b2)
    gx = gh @ w1
    out = {"pre": pre, "y": y, "gx": gx}
    if mutation == "last_row":
        out = {k: v.clone() for k, v in out.items()}
        for v in out.values():
            v[-1] = 0
    return out


# which outputs a defect must move (the reverse pass carries no bias; pre is formed before the second product)
MUTATIONS = {"last_hidden_tile": ("pre", "y", "gx"), "bias1": ("pre", "y"), "bias2": ("y",), "swap_hidden_tiles": ("y", "gx"),
             "k1_tail": ("pre", "y", "gx"), "last_row": ("pre", "y", "gx")}


@functools.lru_cache(maxsize=None)
def master(H, k1, n2):
    rng = np.random.default_rng([2025, H, k1, n2])
    n = ROWS_MAX[H]
    c = SimpleNamespace(H=H, k1=k1, n2=n2, n=n, x=_f32(rng.standard_normal((n, k1))), g=_f32(rng.standard_normal((n, n2))),
                        w1=_f32(rng.standard_normal((H, k1)) / np.sqrt(k1)), b1=_f32(0.5 * rng.standard_normal(H)),
                        w2=_f32(rng.standard_normal((n2, H)) / np.sqrt(H)), b2=_f32(0.5 * rng.standard_normal(n2)))
    c.ref = evaluate(c, torch.float64)      # row by row: a case of n rows is a slice (computed once, never modified)
    c.ref32 = evaluate(c, torch.float32)
    return c


def case(H, k1, n2, n):
    m = master(H, k1, n2)
    assert n <= m.n
    c = SimpleNamespace(H=H, k1=k1, n2=n2, n=n, w1=m.w1, b1=m.b1, w2=m.w2, b2=m.b2, x=m.x[:n], g=m.g[:n])
    c.ref = {k: v[:n] for k, v in m.ref.items()}
    c.ref32 = {k: v[:n] for k, v in m.ref32.items()}
    return c
