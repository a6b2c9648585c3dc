"""Cases and f64 / f32 restatements for the update kernels: the first half of XPainnUpdate.forward on the matrix cores and its reverse
(xeq_update_uv_fwd / _bwd, csrc/xeq_update.hip), the chain kernels of csrc/xeq_node.hip (xeq_norm_fwd / _bwd, xeq_uv_reduce_fwd / _bwd,
xeq_update_out_fwd / _bwd) and xeq_norm_param_grad (csrc/xeq_train.hip).  CPU only; no test functions here.
tests/test_gpu_update_kernels.py runs the cases on the GPU, tests/test_update_cases_host.py checks the layout table against the built
library, that the restatement composes to XPaiNNOracle.update, and the POWER of the comparison on the host.

A case is (layout (m0, m1, m2), node_dim F, n rows): the first n rows of one master draw per (layout, F), so a row means the same
numbers whatever the row count.  Every input is drawn in f64 and rounded to f32 once: the kernels, the f32 restatement and the f64
reference see the same numbers.  s, x, g_s_out, g_x_out, a (the update MLP's output), ip, g_cat, g_p ~ N(0, 1); the weights of
update_U / update_V ~ N(0, 1) per block; their biases and the four norm parameters are moved by N(0, 1/4), so that a lost bias group
or affine term is O(1/2).  Row ZERO_ROW of every master draw is all zero (s = 0, x = 0: the capacity padding of the whole-step
graphs), row BIG_ROW is scaled by 1e3; both are compared in groups of their own with bounds of their own.

The reference is written with the functions of oracle/xpainn_oracle.py (equivariant_layer_norm, o3_linear, invariant,
equivariant_dot, elementwise_tp, F.layer_norm); gradients come from autograd.  Every tensor the entry points write is restated in
the entry point's layout: cat = [shat | v], p, the U|V pair buffer and g_xhat in the BT layout (nn/fused.py::_bt_blocks),
stats = (mean, rstd, mean0, r), g_s, g_x; for the output stage s_out, x_out, g_a, g_ip.

Bound per output tensor and row group: the project's rule, max(1e-4 max(1, max|ref|), 1.5 err32), err32 = |f32 restatement - f64
reference| on the rows of the group (tests/test_gpu_painn.py::_bound, tests/mlp_width_cases.py::bound)."""
import functools
import itertools
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

from oracle import xpainn_oracle as xo

EPS = 1e-5                       # Invariant's eps (nn/o3layer.py:15)
MULS = (0, 32, 64, 128)
D_MAX = 480
ROWS = (1, 15, 16, 17, 31, 32, 33, 65)
THRESHOLD_ROWS = (4096, 4097, 8192, 8200)        # as mlp_width_cases.THRESHOLD_ROWS: all tiles split, none split, a split short last round
THRESHOLD_LAYOUTS = ((32, 0, 0), (64, 32, 64))
ZERO_ROW, BIG_ROW = 5, 11
BIG = 1e3


def dims(mul):
    return mul[0] + 3 * mul[1] + 5 * mul[2], sum(mul)            # D, C


def admitted(node_dim, mul, f64=False):
    """xeq_update_uv_supported's rule, restated."""
    D, C = dims(mul)
    return (not f64 and all(m in MULS for m in mul) and C > 0 and D <= D_MAX and node_dim > 0 and node_dim % 4 == 0 and node_dim <= 128)


def default_node_dim(mul):
    return mul[0] if mul[0] > 0 else 64


LAYOUTS = tuple(mul for mul in itertools.product(MULS, repeat=3) if admitted(default_node_dim(mul), mul))
NODE_DIMS_EXTRA = (4, 36, 100, 128)
EXTRA_LAYOUTS = ((0, 128, 0), (32, 0, 64), (64, 32, 64), (64, 128, 0))
# every (layout, node_dim) the entry-level tests run
CONFIGS = tuple((mul, default_node_dim(mul)) for mul in LAYOUTS) + tuple(
    (mul, f) for mul in EXTRA_LAYOUTS for f in NODE_DIMS_EXTRA if f != default_node_dim(mul))
# (what, f64, node_dim, layout)
REFUSED = (("node_dim 0", 0, 0, (128, 64, 32)), ("node_dim 2", 0, 2, (128, 64, 32)), ("node_dim 132", 0, 132, (128, 64, 32)),
           ("node_dim 256", 0, 256, (128, 64, 32)), ("mul 96", 0, 96, (96, 32, 0)), ("mul 16", 0, 64, (64, 16, 0)),
           ("mul 96 at l = 2", 0, 64, (64, 0, 96)), ("D 544", 0, 128, (128, 128, 32)), ("D 640", 0, 64, (0, 0, 128)),
           ("empty", 0, 64, (0, 0, 0)), ("f64", 1, 128, (128, 64, 32)))

FWD_OUTPUTS = ("cat", "p", "uv", "stats")
BWD_OUTPUTS = ("g_xhat", "g_s", "g_x")
OUT_OUTPUTS = ("s_out", "x_out", "g_a", "g_ip")
CHAIN_OUTPUTS = ("shat", "xhat", "stats", "nb_g_s", "nb_g_x", "v", "p", "g_uv", "s_out", "x_out", "g_a", "g_ip")


def config_id(mul, node_dim):
    return f"{mul[0]}-{mul[1]}-{mul[2]}/{node_dim}"


def irreps_of(mul):
    return "+".join(f"{m}x{l}{'eoe'[l]}" for l, m in enumerate(mul) if m > 0)


def mul_of(irreps):
    mul = [0, 0, 0]
    for m, l, _ in xo.parse_irreps(irreps):
        mul[l] += m
    return tuple(mul)


def bound(ref, ref32):
    return max(1e-4 * max(1.0, float(ref.abs().max())), 1.5 * float((ref32.double() - ref).abs().max()))


def groups(n):
    """Row groups of a case of n rows: name -> row indices."""
    special = [r for r in (ZERO_ROW, BIG_ROW) if r < n]
    out = {"ordinary": [r for r in range(n) if r not in special]}
    if ZERO_ROW < n:
        out["zero"] = [ZERO_ROW]
    if BIG_ROW < n:
        out["big"] = [BIG_ROW]
    return out


# ------------------------------------------------------------------------------------------------------------------- the BT layout
def to_bt(t, mul, pair=None, l2_m_major=False):
    """[n, D] in the e3nn layout (channel-major, m-minor) -> the flat BT buffer: per block a row-major [n (2l+1), mul_l] matrix, blocks
    one behind the other (nn/fused.py::_bt_blocks).  ``pair``: a second tensor V; the rows are then [U | V], 2 mul_l wide.
    ``l2_m_major``: the rows of the l = 2 block ordered (m, node) instead of (node, m) -- a defect, for the power check."""
    n = t.shape[0]
    parts, off = [], 0
    for l, m in enumerate(mul):
        d = 2 * l + 1
        if m == 0:
            continue
        blk = t[:, off:off + m * d].reshape(n, m, d).transpose(1, 2)            # (node, m, channel)
        if pair is not None:
            blk = torch.cat([blk, pair[:, off:off + m * d].reshape(n, m, d).transpose(1, 2)], -1)
        if l == 2 and l2_m_major:
            blk = blk.transpose(0, 1)
        parts.append(blk.reshape(-1))
        off += m * d
    return torch.cat(parts)


def from_bt(buf, n, mul, width=1):
    """The flat BT buffer -> rows per node, [n, width D]: per block (m, [U | V], channel) of the node, blocks side by side."""
    parts, base = [], 0
    for l, m in enumerate(mul):
        d = 2 * l + 1
        if m == 0:
            continue
        parts.append(buf[n * base * width:n * (base + d * m) * width].reshape(n, d * width * m))
        base += d * m
    return torch.cat(parts, 1)


def rows_of(name, t, n, mul):
    """An output as the entry point lays it out -> one row per node (what the row groups index)."""
    if name in ("uv", "g_uv"):
        return from_bt(t, n, mul, 2)
    if name in ("g_xhat", "xhat"):
        return from_bt(t, n, mul, 1)
    return t


# ------------------------------------------------------------------------------------------------------------------- the reference
def _eq_layer_norm(irreps, mul, x, w, b, centre=True, over_d=False):
    """EquivariantLayerNorm (nn/o3layer.py:145-171) with its statistics: -> xhat, mean0, r.  Unchanged it IS
    oracle.equivariant_layer_norm; ``centre`` / ``over_d`` restate two defects (0e channels not centred, rms over D instead of C)."""
    m0 = mul[0]
    mean0 = x[:, :m0].mean(1) if m0 > 0 else torch.zeros_like(x[:, 0])
    xc = torch.cat([x[:, :m0] - mean0[:, None], x[:, m0:]], 1) if (m0 > 0 and centre) else x
    sq = xo.invariant(irreps, xc, squared=True)
    r = torch.reciprocal(torch.sqrt(sq.sum(1) / (x.shape[1] if over_d else sq.shape[1]) + 1e-5))
    if centre and not over_d:
        xhat = xo.equivariant_layer_norm(irreps, x, w, b)
    else:
        xhat = xo.elementwise_tp(irreps, xc * r[:, None], w.unsqueeze(0))
        xhat = torch.cat([xhat[:, :m0] + b, xhat[:, m0:]], 1)
    return xhat, (mean0 if centre else torch.zeros_like(mean0)), r


def _widest(mul):
    """(l, flat offset, mul) of the widest block (the highest l among equals)."""
    l = max(range(3), key=lambda k: (mul[k], k))
    return l, (0, mul[0], mul[0] + 3 * mul[1])[l], mul[l]


def evaluate(c, dtype, do_norm=1, has_bias=1, gx=1, mutation=None):
    """Everything xeq_update_uv_fwd and xeq_update_uv_bwd write for the case, in ``dtype``: cat, p, uv (BT pair buffer), stats; g_xhat
    (BT), g_s, g_x.  ``gx`` = 0: g_x_out is NULL (zero).  ``mutation`` restates the case with one defect a kernel could have:
      "swap_uv"        the U and V halves of the pair buffer change places
      "last_tile"      the last 32 channels of the widest block are never formed (U = V = 0 there)
      "bt_m_major"     the BT rows of the l = 2 block are taken as (m, node) instead of (node, m)
      "bias0"          the l = 0 bias group is lost
      "no_centre"      the 0e channels are not centred
      "rms_over_d"     the rms is taken over D instead of C
      "gate_offset_l2" the gate offset of l = 2 is taken as m0 + 3 m1 instead of m0 + m1 (modulo C: the kernel would leave the row; where that
                       is the right offset again, m0)
      "no_gxout"       g_x_out is ignored in g_U
      "no_eps2"        eps^2 is dropped under the square root of g_V
      "last_row"       the last row of every output is not written (reads back as 0)"""
    t = lambda v: v.detach().to(dtype).clone()
    mul, Fd, ir = c.mul, c.F, c.irreps
    m0, m1, m2 = mul
    D, C = dims(mul)
    n = c.s.shape[0]
    s, x = t(c.s).requires_grad_(), t(c.x).requires_grad_()
    a, g_cat, g_p, g_s_out, g_x_out = (t(getattr(c, k)) for k in ("a", "g_cat", "g_p", "g_s_out", "g_x_out"))
    wu, wv, bu, bv, lnw, lnb, eqw, eqb = (t(getattr(c, k)) for k in ("wu", "wv", "bu", "bv", "lnw", "lnb", "eqw", "eqb"))
    if not (has_bias and m0 > 0) or mutation == "bias0":
        bu = bv = None
    if do_norm:
        shat = F.layer_norm(s, (Fd,), lnw, lnb, 1e-5)
        xhat, mean0, r = _eq_layer_norm(ir, mul, x, eqw, eqb, centre=mutation != "no_centre", over_d=mutation == "rms_over_d")
        mean = s.mean(1)
        rstd = torch.reciprocal(torch.sqrt(s.var(1, unbiased=False) + 1e-5))
        stats = torch.stack([mean, rstd, mean0, r], 1).detach()
    else:
        shat, xhat = s * 1, x * 1
        stats = torch.tensor([0.0, 1.0, 0.0, 1.0], dtype=dtype).repeat(n, 1)
    U = xo.o3_linear(ir, xhat, wu, bu)
    V = xo.o3_linear(ir, xhat, wv, bv)
    if mutation == "swap_uv":
        U, V = V, U
    if mutation == "last_tile":
        l, off, m = _widest(mul)
        keep = torch.ones(D, dtype=dtype)
        keep[off + (m - 32) * (2 * l + 1):off + m * (2 * l + 1)] = 0
        U, V = U * keep, V * keep
    v = xo.invariant(ir, V, eps=EPS)
    p = xo.equivariant_dot(ir, U, V)
    gate = torch.arange(C)
    if mutation == "gate_offset_l2":
        wrong = (m0 + 3 * m1) % C
        gate[m0 + m1:] = ((m0 if wrong == m0 + m1 else wrong) + torch.arange(m2)) % C
    v_out, p_out = v, p
    if mutation == "gate_offset_l2":
        v_out, p_out = torch.zeros_like(v), torch.zeros_like(p)
        v_out[:, :m0 + m1], p_out[:, :m0 + m1] = v[:, :m0 + m1], p[:, :m0 + m1]
        v_out[:, gate[m0 + m1:]], p_out[:, gate[m0 + m1:]] = v[:, m0 + m1:], p[:, m0 + m1:]
    # the reverse pass: L = <cat, g_cat> + <p, g_p> + <x_out, g_x_out> + <s, g_s_out> with x_out = x + U (x) a_vv
    v_l = (torch.sqrt(xo.equivariant_dot(ir, V, V)) - EPS) if mutation == "no_eps2" else v
    L = (shat * g_cat[:, :Fd]).sum() + (v_l * g_cat[:, Fd:][:, gate]).sum() + (p * g_p[:, gate]).sum() + (s * g_s_out).sum()
    if gx:
        L = L + (x * g_x_out).sum()
        if mutation != "no_gxout":
            L = L + (xo.elementwise_tp(ir, U, a[:, :C][:, gate]) * g_x_out).sum()
    g_s, g_x, g_xhat = torch.autograd.grad(L, [s, x, xhat])
    cat = torch.cat([shat, v_out], 1).detach()
    U, V, p_out = U.detach(), V.detach(), p_out.detach()
    if mutation == "last_row":
        cat, p_out, stats, g_s, g_x, U, V, g_xhat = (w.clone() for w in (cat, p_out, stats, g_s, g_x, U, V, g_xhat))
        for w in (cat, p_out, stats, g_s, g_x, U, V, g_xhat):
            w[-1] = 0
    bad_bt = mutation == "bt_m_major"
    return {"cat": cat, "p": p_out, "uv": to_bt(U, mul, pair=V, l2_m_major=bad_bt), "stats": stats,
            "g_xhat": to_bt(g_xhat, mul, l2_m_major=bad_bt), "g_s": g_s, "g_x": g_x, "_U": U, "_V": V}


# which outputs a defect must move, and the layouts / settings it applies to
MUTATIONS = {
    "swap_uv": (("uv", "cat", "g_xhat", "g_x"), lambda mul: True),
    "last_tile": (("uv", "cat", "p", "g_xhat", "g_x"), lambda mul: True),
    "bt_m_major": (("uv", "g_xhat"), lambda mul: mul[2] > 0),
    "bias0": (("uv", "cat", "p", "g_xhat", "g_x"), lambda mul: mul[0] > 0),
    "no_centre": (("stats", "uv", "cat", "p", "g_xhat", "g_x"), lambda mul: mul[0] > 0),
    "rms_over_d": (("stats", "uv", "cat", "p", "g_xhat", "g_x"), lambda mul: mul[1] + mul[2] > 0),
    "gate_offset_l2": (("cat", "p", "g_xhat", "g_x"), lambda mul: mul[2] > 0 and mul[1] > 0),
    "no_gxout": (("g_xhat", "g_x"), lambda mul: True),
    "no_eps2": (("g_xhat",), lambda mul: True),          # judged on the zero row without norms and bias: V = 0 there
    "last_row": (FWD_OUTPUTS + BWD_OUTPUTS, lambda mul: True),
}


def evaluate_out(c, dtype, U=None):
    """xeq_update_out_fwd / _bwd: s_out = s + a_sv ip + a_ss, x_out = x + U (x) a_vv; g_a = [sum_m U g_x_out | g_s_out ip | g_s_out],
    g_ip = g_s_out a_sv.  U: [n, D] in the e3nn layout (the case's independent draw unless given)."""
    t = lambda v: v.detach().to(dtype).clone()
    C = dims(c.mul)[1]
    s, x, g_s_out, g_x_out = (t(getattr(c, k)) for k in ("s", "x", "g_s_out", "g_x_out"))
    a, ip = t(c.a).requires_grad_(), t(c.ip).requires_grad_()
    U = t(c.U_in if U is None else U)
    a_vv, a_sv, a_ss = torch.split(a, [C, c.F, c.F], -1)
    s_out = s + a_sv * ip + a_ss
    x_out = x + xo.elementwise_tp(c.irreps, U, a_vv)
    g_a, g_ip = torch.autograd.grad((s_out * g_s_out).sum() + (x_out * g_x_out).sum(), [a, ip])
    return {"s_out": s_out.detach(), "x_out": x_out.detach(), "g_a": g_a, "g_ip": g_ip}


def evaluate_chain(c, dtype):
    """What the chain kernels of csrc/xeq_node.hip write, each from the case's independent inputs:
      xeq_norm_fwd       shat, xhat (BT), stats            xeq_norm_bwd       nb_g_s, nb_g_x from g_cat[:, :F], g_xh (BT), g_s_out, g_x_out
      xeq_uv_reduce_fwd  v, p from U_in, V_in              xeq_uv_reduce_bwd  g_uv (BT pair) from g_p, g_cat[:, F:], g_x_out, a
      xeq_update_out_*   s_out, x_out, g_a, g_ip           (evaluate_out)"""
    t = lambda v: v.detach().to(dtype).clone()
    mul, Fd, ir = c.mul, c.F, c.irreps
    C = dims(mul)[1]
    s, x = t(c.s).requires_grad_(), t(c.x).requires_grad_()
    lnw, lnb, eqw, eqb, g_cat, g_p, g_xh, g_s_out, g_x_out, a = (t(getattr(c, k)) for k in (
        "lnw", "lnb", "eqw", "eqb", "g_cat", "g_p", "g_xh", "g_s_out", "g_x_out", "a"))
    out = {}
    if c.do_norm:
        shat = F.layer_norm(s, (Fd,), lnw, lnb, 1e-5)
        xhat, mean0, r = _eq_layer_norm(ir, mul, x, eqw, eqb)
        stats = torch.stack([s.mean(1), torch.reciprocal(torch.sqrt(s.var(1, unbiased=False) + 1e-5)), mean0, r], 1).detach()
    else:
        shat, xhat = s * 1, x * 1
        stats = torch.tensor([0.0, 1.0, 0.0, 1.0], dtype=dtype).repeat(s.shape[0], 1)
    nb_g_s, nb_g_x = torch.autograd.grad((shat * g_cat[:, :Fd]).sum() + (xhat * g_xh).sum() + (s * g_s_out).sum() + (x * g_x_out).sum(), [s, x])
    out.update(shat=shat.detach(), xhat=to_bt(xhat.detach(), mul), stats=stats, nb_g_s=nb_g_s, nb_g_x=nb_g_x)
    U, V = t(c.U_in).requires_grad_(), t(c.V_in).requires_grad_()
    v, p = xo.invariant(ir, V, eps=EPS), xo.equivariant_dot(ir, U, V)
    L = (v * g_cat[:, Fd:]).sum() + (p * g_p).sum() + (xo.elementwise_tp(ir, U, a[:, :C]) * g_x_out).sum()
    g_U, g_V = torch.autograd.grad(L, [U, V])
    out.update(v=v.detach(), p=p.detach(), g_uv=to_bt(g_U, mul, pair=g_V))
    out.update(evaluate_out(c, dtype))
    return out


def norm_param_grads(c, dtype):
    """dL/d(ln_w, ln_b, eq_w, eq_b) for L = <shat, g_cat[:, :F]> + <xhat, g_xh>, by autograd."""
    t = lambda v: v.detach().to(dtype).clone()
    prm = [t(getattr(c, k)).requires_grad_() for k in ("lnw", "lnb", "eqw", "eqb")]
    s, x, g_cat, g_xh = (t(getattr(c, k)) for k in ("s", "x", "g_cat", "g_xh"))
    shat = F.layer_norm(s, (c.F,), prm[0], prm[1], 1e-5)
    xhat = xo.equivariant_layer_norm(c.irreps, x, prm[2], prm[3])
    L = (shat * g_cat[:, :c.F]).sum() + (xhat * g_xh).sum()
    if c.mul[0] == 0:
        L = L + 0 * prm[3].sum()
    return torch.cat(torch.autograd.grad(L, prm))


# ----------------------------------------------------------------------------------------------------------------------- the draws
def _f32(a):
    return torch.tensor(np.asarray(a, dtype=np.float32).astype(np.float64))


INPUTS = ("s", "x", "g_s_out", "g_x_out", "a", "ip", "g_cat", "g_p", "U_in", "V_in", "g_xh")
PARAMS = ("wu", "wv", "bu", "bv", "lnw", "lnb", "eqw", "eqb")


ROWS_MASTER = max(ROWS)


@functools.lru_cache(maxsize=None)
def master(mul, node_dim, n=ROWS_MASTER, do_norm=1):
    """The master draw of (layout, node_dim), ``n`` rows of it.  Every tensor has a random stream of its own and is drawn row by row, so
    a longer draw (the TileSplit thresholds, the parameter-gradient sums) starts with the rows of a shorter one."""
    mul = tuple(mul)
    D, C = dims(mul)
    c = SimpleNamespace(mul=mul, F=node_dim, n=n, irreps=irreps_of(mul), do_norm=do_norm)
    N = lambda k, *shape: np.random.default_rng([2026, *mul, node_dim, k]).standard_normal(shape)
    nw = sum(m * m for m in mul)
    c.wu, c.wv, c.bu, c.bv = _f32(N(0, nw)), _f32(N(1, nw)), _f32(0.5 * N(2, mul[0])), _f32(0.5 * N(3, mul[0]))
    c.lnw, c.lnb = _f32(1 + 0.5 * N(4, node_dim)), _f32(0.5 * N(5, node_dim))
    c.eqw, c.eqb = _f32(1 + 0.5 * N(6, C)), _f32(0.5 * N(7, mul[0]))
    for i, (k, w) in enumerate((("s", node_dim), ("x", D), ("g_s_out", node_dim), ("g_x_out", D), ("a", C + 2 * node_dim), ("ip", node_dim),
                                ("g_cat", node_dim + C), ("g_p", C), ("U_in", D), ("V_in", D), ("g_xh", D))):
        v = N(8 + i, n, w)
        if k in ("s", "x", "U_in", "V_in"):
            if n > ZERO_ROW:
                v[ZERO_ROW] = 0
            if n > BIG_ROW:
                v[BIG_ROW] *= BIG
        setattr(c, k, _f32(v))
    return c


def take(c, n, **over):
    """The first n rows of a draw (parameters shared), with inputs replaced by ``over``."""
    assert n <= c.n
    d = SimpleNamespace(**vars(c))
    d.n = n
    for k in INPUTS:
        setattr(d, k, getattr(c, k)[:n])
    for k, v in over.items():
        setattr(d, k, v)
    return d


@functools.lru_cache(maxsize=None)
def reference(mul, node_dim, n_master, do_norm, has_bias, gx, f32):
    """Row forms of evaluate() on a whole master draw: a case of n rows is a slice (computed once, never modified)."""
    m = master(mul, node_dim, n_master)
    out = evaluate(m, torch.float32 if f32 else torch.float64, do_norm, has_bias, gx)
    return {k: rows_of(k, v, m.n, m.mul) for k, v in out.items()}


def case(mul, node_dim, n, do_norm=1, has_bias=1, gx=1):
    """-> the inputs of the case, ref / ref32: name -> [n, .] rows (rows_of form)."""
    mul = tuple(mul)
    n_master = ROWS_MASTER if n <= ROWS_MASTER else max(THRESHOLD_ROWS)
    c = take(master(mul, node_dim, n_master), n)
    c.ref = {k: v[:n] for k, v in reference(mul, node_dim, n_master, do_norm, has_bias, gx, False).items()}
    c.ref32 = {k: v[:n] for k, v in reference(mul, node_dim, n_master, do_norm, has_bias, gx, True).items()}
    return c


def judge(ref, ref32, got, names, n):
    """Per output and row group: (name, group, err, err32, bound).  ref / ref32 / got: name -> [n, .] rows."""
    res = []
    for k in names:
        for grp, idx in groups(n).items():
            if not idx:
                continue
            r, r32, g = ref[k][idx], ref32[k][idx], got[k][idx].double()
            err = float((g - r).abs().max()) if bool(torch.isfinite(g).all()) else float("inf")
            res.append((k, grp, err, float((r32.double() - r).abs().max()), bound(r, r32)))
    return res
