"""Cases and f64 / f32 restatements for the node kernels of the twice-differentiable training pass (csrc/xeq_train_node.hip;
nn/training_ops.py: xeq_train_norm, xeq_train_uv, xeq_train_out, each as forward, reverse, forward with tangents, reverse with
tangents).  CPU only; no test functions here.  tests/test_gpu_train_node.py runs the cases on the GPU, tests/test_train_node_cases_host.py
checks the restatement against torch / nn.training, the properties of the case list and the POWER of the comparison on the host.

The restatement takes tensors in the entry points' layouts: ``norm``, ``uv``, ``out``.  ``three_orders`` differentiates one of them twice
with torch's double backward and returns what the four kernel forms write: the values (forward), J^T g (reverse), d<u, J^T g>/dg (forward
with tangents), d<u, J^T g>/d inputs (reverse with tangents).  For the norm the four parameters are inputs with a copy per ROW, so that the
per-row parameter gradients the reverse kernel writes (``rows`` [N, 2F + C + mul0]) are judged row by row.

A case is (F, mul, n rows, near): the first n rows of one master draw per (F, mul), every tensor from a random stream of its own, drawn
row by row in f64 and rounded to f32 once (update_cases.master's scheme): a row means the same numbers whatever the row count and whatever
the precision.  Row ZERO_ROW of s, x, U, V is zero, row BIG_ROW scaled by 1e3 (update_cases); both are judged as groups of their own.

Condition in f32.  Invariant(V) = sqrt(V^2 + eps^2) - eps has the second derivative eps^2 / (V^2 + eps^2)^(3/2): for a scalar channel with
|V| near eps = 1e-5 it reaches 1 / eps.  Among N(0, 1) draws a few such channels give entries of 1e4 ... 1e5 on
which the f32 tensor chain itself is off by 1e-2, a thousand times the 4-ulp floor of the output's other entries, and their size would
set the bound for all of them.  Every draw therefore has |V| >= V0_MIN = 0.5 in the l = 0 block (the zero row apart, where V = 0
exactly); the values 0, 1e-7, 1e-5, 1e-3 stand in the rows NEAR_ROWS of the f64-only variant (``near=True``), where they are well
resolved, and are judged as the group "near".  tests/test_train_node_cases_host.py asserts both facts and the figures.

Bounds (tests/test_gpu_train_edge.py's), per output and row group:
  f64  values 1e-12, derivatives of both orders 1e-9, of the largest entry of the output in the group, at least the ordinary group's;
  f32  max(4 x the f32 restatement's own error against f64 on the same inputs, 4 ulp of that largest entry)."""
import functools
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as tf
from torch.autograd.functional import jvp

from tests.update_cases import BIG, BIG_ROW, ZERO_ROW, _f32, dims, from_bt, groups as _row_groups, to_bt

EPS_LN = EPS_EQ = 1e-5          # nn.LayerNorm's and EquivariantLayerNorm's defaults
EPS_INV = 1e-5                  # Invariant's (nn/o3layer.py:15)
V0_MIN = 0.5
NEAR_ROWS = (20, 21, 22, 23)
NEAR_VALUES = (0.0, 1e-7, 1e-5, 1e-3)
GRID_ROWS = 4 * 4096            # rows one round of k_norm_fwd / k_norm_bwd covers: 4096 blocks of four waves

CONFIGS = (
    (128, (128, 64, 32)),       # the default model
    (256, (256, 64, 32)),       # widest model the suite runs; D = 608: ten lane rounds, the last one half full
    (32, (32, 0, 64)),          # no l = 1
    (64, (64, 32, 0)),          # no l = 2
    (96, (96, 33, 7)),          # F and D = 230 leave a partial lane round; odd multiplicities
    (32, (0, 16, 8)),           # no scalar channels, eq_b empty
    (64, (8, 4, 4)),            # C = 16 < F: the threads t >= C of k_out
    (6, (5, 3, 2)),             # the toy of tests/test_gpu_training_ops.py
)
# both sides of a four-wave block; 257 C is no multiple of the 256 threads of a k_uv / k_out block for any C here
ROWS = (1, 3, 4, 5, 63, 257)
ROWS_MASTER = max(ROWS)
LONG = (32, (32, 16, 8))        # 152 floats per row
LONG_ROWS = GRID_ROWS + 5       # a second grid-stride round with a partial last block
FUNCTION_CONFIGS = ((128, (128, 64, 32)), (96, (96, 33, 7)))

KINDS = ("norm0", "norm1", "uv", "out")           # norm0 / norm1: xeq_train_norm with xhat as e3nn rows / in the BT layout
# kernel form -> the outputs it writes
FORMS = {
    "norm0": {"fwd": ("o_s", "o_x"), "bwd": ("d_s", "d_x", "rows"), "fwd_dual": ("dg_s", "dg_x"), "bwd_dual": ("dd_s", "dd_x", "dd_rows")},
    "uv": {"fwd": ("o",), "bwd": ("d_uv",), "fwd_dual": ("dg",), "bwd_dual": ("dd_uv",)},
    "out": {"fwd": ("o_s", "o_x"), "bwd": ("d_uv", "d_a", "d_in"), "fwd_dual": ("dg_s", "dg_x"), "bwd_dual": ("dd_uv", "dd_a", "dd_in")},
}
FORMS["norm1"] = FORMS["norm0"]
VALUES = ("o", "o_s", "o_x")                      # judged to 1e-12 in f64; everything else is a derivative: 1e-9


def outputs(kind):
    return tuple(k for names in FORMS[kind].values() for k in names)


def config_id(F, mul):
    return f"{F}/{mul[0]}-{mul[1]}-{mul[2]}"


def channel_of(mul):
    """Channel of every element of an e3nn row."""
    ch, c = [], 0
    for l, m in enumerate(mul):
        ch += [c + k for k in range(m) for _ in range(2 * l + 1)]
        c += m
    return torch.tensor(ch, dtype=torch.long)


# ------------------------------------------------------------------------------------------------------------------ the uv layout
def uv_list(U, V, mul):
    """U, V [n, D] e3nn rows -> the three tensors the entries take: uv_l [n (2l+1), 2 mul_l] = (U | V) BT rows; an absent l is empty."""
    n = U.shape[0]
    flat, out, off = to_bt(U, mul, pair=V), [], 0
    for l, m in enumerate(mul):
        size = n * (2 * l + 1) * 2 * m
        out.append(flat[off:off + size].reshape(n * (2 * l + 1), 2 * m) if m else flat.new_zeros(0))
        off += size
    return out


def uv_rows(ts, n):
    """-> one row per node: per l (m, [U | V], channel)."""
    return torch.cat([t.reshape(n, -1) for t in ts if t.numel()], 1)


def v_half(mul):
    """Columns of ``uv_rows`` that hold V."""
    parts = []
    for l, m in enumerate(mul):
        if m:
            blk = torch.zeros(2 * l + 1, 2 * m, dtype=torch.bool)
            blk[:, m:] = True
            parts.append(blk.reshape(-1))
    return torch.cat(parts)


def _halves(uv_l, l, m):
    blk = uv_l.reshape(-1, 2 * l + 1, 2 * m)
    return blk[:, :, :m], blk[:, :, m:]


# ------------------------------------------------------------------------------------------------------------------ the restatement
def _centred(x, M0, m0_const=False):
    if M0 == 0:
        return x
    m0 = x[:, :M0].mean(1, keepdim=True)
    return torch.cat([x[:, :M0] - (m0.detach() if m0_const else m0), x[:, M0:]], 1)


def eq_norm(x, eq_w, eq_b, mul, eps, over_d=False, m0_const=False):
    """EquivariantLayerNorm (nn/o3layer.py:145-171) on e3nn rows; eq_w [C] or [n, C], eq_b [mul0] or [n, mul0].  ``over_d``: the rms over
    D instead of C, ``m0_const``: the mean of the 0e channels taken as a constant when differentiated -- two defects."""
    D, C = dims(mul)
    c = _centred(x, mul[0], m0_const)
    inv = torch.rsqrt((c * c).sum(1, keepdim=True) / (D if over_d else C) + eps)
    y = c * inv * eq_w[..., channel_of(mul)]
    return torch.cat([y[:, :mul[0]] + eq_b, y[:, mul[0]:]], 1) if mul[0] else y


def eq_norm_reverse(x, g, eq_w, mul, eps, m0_const=False, k3_const=False):
    """The reverse of ``eq_norm`` written out, with the intermediates of k_norm_bwd: -> dL/dx, dL/d eq_w per row [n, C]."""
    D, C = dims(mul)
    ch = channel_of(mul)
    c = _centred(x, mul[0], m0_const)
    inv = torch.rsqrt((c * c).sum(1, keepdim=True) / C + eps)
    t = g * eq_w[..., ch]
    k3 = inv ** 3 * (c * t).sum(1, keepdim=True) / C
    cb = inv * t - (k3.detach() if k3_const else k3) * c
    if mul[0]:
        cb = torch.cat([cb[:, :mul[0]] - cb[:, :mul[0]].mean(1, keepdim=True), cb[:, mul[0]:]], 1)
    return cb, torch.zeros(x.shape[0], C, dtype=x.dtype).index_add(1, ch, c * g) * inv


def norm(s, x, ln_w, ln_b, eq_w, eq_b, F, mul, eps_ln, eps_eq, over_d=False):
    """-> (LayerNorm(s), EquivariantLayerNorm(x)), both as rows; the parameters shared ([F], [C], [mul0]) or one copy per row."""
    return tf.layer_norm(s, (F,), None, None, eps_ln) * ln_w + ln_b, eq_norm(x, eq_w, eq_b, mul, eps_eq, over_d)


def uv(uv0, uv1, uv2, mul, eps):
    """-> [n, 2C] = [Invariant(V) | sum_m U V]"""
    vn, dot = [], []
    for l, (t, m) in enumerate(zip((uv0, uv1, uv2), mul)):
        if m:
            U, V = _halves(t, l, m)
            vn.append(torch.sqrt((V * V).sum(1) + eps ** 2) - eps)
            dot.append((U * V).sum(1))
    return torch.cat(vn + dot, 1)


def out(uv0, uv1, uv2, a, inner, F, mul):
    """-> (a_sv inner + a_ss [n, F], U (x) a_vv [n, D] e3nn rows); a = [a_vv | a_sv | a_ss]"""
    C = sum(mul)
    a_vv, a_sv, a_ss = torch.split(a, [C, F, F], -1)
    parts, ch = [], 0
    for l, (t, m) in enumerate(zip((uv0, uv1, uv2), mul)):
        if m:
            U = _halves(t, l, m)[0]
            parts.append((U * a_vv[:, None, ch:ch + m]).transpose(1, 2).reshape(a.shape[0], m * (2 * l + 1)))
            ch += m
    return a_sv * inner + a_ss, torch.cat(parts, 1)


def three_orders(fn, inputs, g, u):
    """fn(*inputs) -> outputs; g: a cotangent per output; u: a cotangent per input gradient (None: that gradient is not differentiated).
    -> (values, J^T g per input, d<u, J^T g>/dg per output, d<u, J^T g>/d inputs per input), by torch's double backward; a gradient
    nothing depends on is zeros."""
    inputs = [t.detach().clone().requires_grad_() for t in inputs]
    g = [t.detach().clone().requires_grad_() for t in g]
    vals = fn(*inputs)
    vals = list(vals) if isinstance(vals, (tuple, list)) else [vals]
    zeros = lambda got, like: [torch.zeros_like(b) if a is None else a.detach() for a, b in zip(got, like)]
    first = torch.autograd.grad(vals, inputs, g, create_graph=True, allow_unused=True)
    pairs = [(f, w) for f, w in zip(first, u) if f is not None and w is not None and f.requires_grad]
    second = torch.autograd.grad([f for f, _ in pairs], g + inputs, [w for _, w in pairs], allow_unused=True)
    return [v.detach() for v in vals], zeros(first, inputs), zeros(second[:len(g)], g), zeros(second[len(g):], inputs)


# ----------------------------------------------------------------------------------------------------------------------- the draws
ROW_TENSORS = ("s", "x", "U", "V", "a", "inner", "g_s", "g_x", "g_vd", "g_os", "g_ox", "u_s", "u_x", "u_U", "u_V", "u_a", "u_in")
PARAMS = ("lnw", "lnb", "eqw", "eqb")
SPECIAL = ("s", "x", "U", "V")


def master(F, mul, n=ROWS_MASTER, near=False):
    """The master draw of (F, mul), ``n`` rows of it; ``near``: the f64-only variant with the near-zero V_0 rows.  (Kept for the row
    counts of ROWS; the long draw, 200 MB, is made anew for whoever asks.)"""
    return _kept(F, tuple(mul), n, near) if n <= ROWS_MASTER else _draw(F, tuple(mul), n, near)


def _draw(F, mul, n, near):
    D, C = dims(mul)
    c = SimpleNamespace(F=F, mul=mul, n=n, near=near)
    N = lambda k, *shape: np.random.default_rng([2027, F, *mul, k]).standard_normal(shape)
    c.lnw, c.lnb = _f32(1 + 0.5 * N(0, F)), _f32(0.5 * N(1, F))
    c.eqw, c.eqb = _f32(1 + 0.5 * N(2, C)), _f32(0.5 * N(3, mul[0]))
    width = dict(s=F, x=D, U=D, V=D, a=C + 2 * F, inner=F, g_s=F, g_x=D, g_vd=2 * C, g_os=F, g_ox=D, u_s=F, u_x=D, u_U=D, u_V=D, u_a=C + 2 * F, u_in=F)
    for i, k in enumerate(ROW_TENSORS):
        v = N(4 + i, n, width[k])
        if k == "V":
            v[:, :mul[0]] = np.sign(v[:, :mul[0]]) * (V0_MIN + np.abs(v[:, :mul[0]]))
            if near:
                for r, val in zip(NEAR_ROWS, NEAR_VALUES):
                    if r < n:
                        v[r, :mul[0]] = val
        if k in SPECIAL:
            if n > ZERO_ROW:
                v[ZERO_ROW] = 0
            if n > BIG_ROW:
                v[BIG_ROW] *= BIG
        setattr(c, k, _f32(v))
    return c


_kept = functools.lru_cache(maxsize=None)(_draw)


def take(c, n):
    """The first n rows of a draw (parameters shared)."""
    assert n <= c.n
    d = SimpleNamespace(**vars(c))
    d.n = n
    for k in ROW_TENSORS:
        setattr(d, k, getattr(c, k)[:n])
    return d


def groups(n, near=False):
    """Row groups of a case: name -> row indices (update_cases.groups, and the near-zero rows of the f64-only variant)."""
    out_ = _row_groups(n)
    rows = [r for r in NEAR_ROWS if r < n] if near else []
    if rows:
        out_["ordinary"] = [r for r in out_["ordinary"] if r not in rows]
        out_["near"] = rows
    return out_


# --------------------------------------------------------------------------------------------------------------------- evaluation
def _per_row(p, n):
    return p.expand(n, p.shape[0]).contiguous()


def call_spec(kind, c, dtype, over_d=False, l2_m_major=False):
    """(fn, inputs, g, u) of ``three_orders`` for the case, in ``dtype``, in the entry's layouts."""
    t = lambda v: v.detach().to(dtype).clone()
    F, mul, n = c.F, c.mul, c.n
    if kind in ("norm0", "norm1"):
        bt = (lambda v: to_bt(v, mul, l2_m_major=l2_m_major)) if kind == "norm1" else (lambda v: v)
        inputs = [t(c.s), t(c.x)] + [_per_row(t(getattr(c, k)), n) for k in PARAMS]

        def fn(s, x, lw, lb, ew, eb):
            o_s, o_x = norm(s, x, lw, lb, ew, eb, F, mul, EPS_LN, EPS_EQ, over_d)
            return o_s, bt(o_x)

        g_x = to_bt(t(c.g_x), mul) if kind == "norm1" else t(c.g_x)
        return fn, inputs, [t(c.g_s), g_x], [t(c.u_s), t(c.u_x), None, None, None, None]
    U = uv_list(t(c.U), t(c.V), mul)
    u_uv = uv_list(t(c.u_U), t(c.u_V), mul)
    if kind == "uv":
        return (lambda a, b, d: uv(a, b, d, mul, EPS_INV)), U, [t(c.g_vd)], u_uv
    return ((lambda p, q, r, a, i: out(p, q, r, a, i, F, mul)), U + [t(c.a), t(c.inner)], [t(c.g_os), t(c.g_ox)],
            u_uv + [t(c.u_a), t(c.u_in)])


def as_rows(kind, forms, n, mul):
    """What the four forms returned -> name -> [n, .] rows.  forms = (values, first, d_g, d_in) in the layouts of ``call_spec``."""
    vals, first, d_g, d_in = forms
    if kind in ("norm0", "norm1"):
        x_rows = (lambda v: from_bt(v, n, mul)) if kind == "norm1" else (lambda v: v)
        return {"o_s": vals[0], "o_x": x_rows(vals[1]), "d_s": first[0], "d_x": first[1], "rows": torch.cat(list(first[2:6]), 1),
                "dg_s": d_g[0], "dg_x": x_rows(d_g[1]), "dd_s": d_in[0], "dd_x": d_in[1], "dd_rows": torch.cat(list(d_in[2:6]), 1)}
    if kind == "uv":
        return {"o": vals[0], "d_uv": uv_rows(first, n), "dg": d_g[0], "dd_uv": uv_rows(d_in, n)}
    return {"o_s": vals[0], "o_x": vals[1], "d_uv": uv_rows(first[:3], n), "d_a": first[3], "d_in": first[4],
            "dg_s": d_g[0], "dg_x": d_g[1], "dd_uv": uv_rows(d_in[:3], n), "dd_a": d_in[3], "dd_in": d_in[4]}


def evaluate(kind, c, dtype, mutation=None):
    """Every output of the four kernel forms for the case, as rows, in ``dtype``.  ``mutation`` restates the case with one defect a
    kernel could have (MUTATIONS)."""
    F, mul, n = c.F, c.mul, c.n
    D, C = dims(mul)
    spec = call_spec(kind, c, dtype, over_d=mutation == "rms_over_d", l2_m_major=mutation == "bt_m_major")
    res = as_rows(kind, three_orders(*spec), n, mul)
    if mutation in ("mean_tangent", "k3_tangent"):
        t = lambda v: v.detach().to(dtype).clone()
        x, u_x, g_x, ew, eb = t(c.x), t(c.u_x), t(c.g_x), _per_row(t(c.eqw), n), _per_row(t(c.eqb), n)
        const = dict(m0_const=mutation == "mean_tangent", k3_const=mutation == "k3_tangent")
        d_x, d_ew = jvp(lambda v: eq_norm_reverse(v, g_x, ew, mul, EPS_EQ, **const), x, u_x)[1]
        res["dd_x"] = d_x
        if mutation == "mean_tangent":
            res["dg_x"] = jvp(lambda v: eq_norm(v, ew, eb, mul, EPS_EQ, m0_const=True), x, u_x)[1]
            res["dd_rows"] = res["dd_rows"].clone()
            res["dd_rows"][:, 2 * F:2 * F + C] = d_ew
    hole = float("nan")
    if mutation == "stride_tail":
        res = {k: v.clone() for k, v in res.items()}
        for v in res.values():
            v[GRID_ROWS:] = hole
    if mutation == "v_half_unwritten":
        for k in ("d_uv", "dd_uv"):
            res[k] = res[k].clone()
            res[k][:, v_half(mul)] = hole
    if mutation == "skip_t_ge_c":
        res = {k: v.clone() for k, v in res.items()}
        for k in ("o_s", "dg_s", "d_in", "dd_in"):
            res[k][:, C:] = hole
        for k in ("d_a", "dd_a"):
            res[k][:, 2 * C:C + F] = hole
            res[k][:, C + F + C:] = hole
    return res


# defect -> (kind it is judged on, the outputs it must move, the smallest case (F, mul, n) it applies to)
MUTATIONS = {
    # the tangent of the 0e mean is dropped in both dual bodies: values and first order are right, the second order is not
    "mean_tangent": ("norm0", ("dg_x", "dd_x", "dd_rows"), (6, (5, 3, 2), 1)),
    # the rms runs over D instead of C
    "rms_over_d": ("norm0", ("o_x", "d_x", "rows", "dg_x", "dd_x", "dd_rows"), (6, (5, 3, 2), 1)),
    # the l = 2 block of the BT layout is ordered (m, node) instead of (node, m): xhat is written and its cotangent read out of place
    "bt_m_major": ("norm1", ("o_x", "d_x", "rows", "dg_x", "dd_x", "dd_rows"), (6, (5, 3, 2), 3)),
    # the grid-stride loop makes one round only: rows from 16 384 on are left as the buffer's fill
    "stride_tail": ("norm0", outputs("norm0"), (*LONG, LONG_ROWS)),
    # the reverse body on dual numbers omits the tangent of k3 = inv^3 <c, g w> / C
    "k3_tangent": ("norm0", ("dd_x",), (6, (5, 3, 2), 1)),
    # k_out's reverse leaves the V half of d_uv unwritten
    "v_half_unwritten": ("out", ("d_uv", "dd_uv"), (6, (5, 3, 2), 1)),
    # the threads t >= C of k_out (C < F), which do the scalar part only, are skipped
    "skip_t_ge_c": ("out", ("o_s", "d_a", "d_in", "dg_s", "dd_a", "dd_in"), (64, (8, 4, 4), 1)),
}


@functools.lru_cache(maxsize=None)
def reference(kind, F, mul, n_master, near, f32):
    """``evaluate`` on a whole master draw: a case of n rows is a slice of it (every function works row by row).  Computed once, never
    modified."""
    return evaluate(kind, master(F, mul, n_master, near), torch.float32 if f32 else torch.float64)


def case(kind, F, mul, n, near=False):
    """-> the inputs of the case with ref / ref32: name -> [n, .] rows."""
    mul = tuple(mul)
    if n > ROWS_MASTER:          # the long case: evaluated for the caller alone, nothing of its size is kept
        c = master(F, mul, n, near)
        c.ref, c.ref32 = evaluate(kind, c, torch.float64), evaluate(kind, c, torch.float32)
        return c
    c = take(master(F, mul, ROWS_MASTER, near), n)
    c.ref = {k: v[:n] for k, v in reference(kind, F, mul, ROWS_MASTER, near, False).items()}
    c.ref32 = {k: v[:n] for k, v in reference(kind, F, mul, ROWS_MASTER, near, True).items()}
    return c


# -------------------------------------------------------------------------------------------------------------------------- bounds
EPS32 = float(torch.finfo(torch.float32).eps)
F32_FACTOR = 4.0


def f64_tolerance(name):
    return 1e-12 if name in VALUES else 1e-9


def judge(ref, ref32, got, names, n, f64, near=False):
    """Per output and row group: (name, group, err, chain error, bound).  ref / ref32 / got: name -> [n, .] rows; the chain error is
    the f32 restatement's own error against the f64 one on the same rows."""
    res = []
    grp = groups(n, near)
    for k in names:
        floor = float(ref[k][grp["ordinary"]].abs().max())
        for name, idx in grp.items():
            r, r32, g = ref[k][idx], ref32[k][idx].double(), got[k][idx].double()
            top = max(floor, float(r.abs().max()))
            err = float((g - r).abs().max()) if bool(torch.isfinite(g).all()) else float("inf")
            chain = float((r32 - r).abs().max())
            bound = f64_tolerance(k) * top if f64 else max(F32_FACTOR * chain, F32_FACTOR * EPS32 * top)
            res.append((k, name, err, chain, bound))
    return res
