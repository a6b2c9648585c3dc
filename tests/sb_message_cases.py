"""Cases and f64 references for the scalar-broadcast ("sb") message kernels (csrc/xeq_message_sb.hip), run through the public ops by
tests/test_gpu_sb_message.py at every basis count the family admits (1 .. 32) and at channel layouts the matrix-core family refuses.
CPU only; no test functions here (tests/test_sb_message_cases_host.py checks this module).

Shared with tests/wq_message_cases.py, not copied: ``message_ref`` (the arithmetic of tests/test_gpu_parity.py::_message_case), the
BT layout maps, ``bound``, the radial parameters, and the rule that every input is drawn in f64 and rounded to f32 once, so that the
kernels, the f32 restatement and the f64 reference see the same numbers.  A case here has its scalar width ``node_dim`` independent of
mul[0].  Reverse quantities are torch.autograd's for the cotangents (g_s, g_x) of the case.

Edge lists (numpy views, independent of the library's sort):
  degrees   the 69-node list of wq_message_cases with six more nodes of out-degree 63, 64, 65, 127, 128, 129 -- both sides of one and of
            two groups of 64 edges (the forward walk's ``pb += 64``, the reverse walk's SB_RED) -- whose neighbours come from a pool of
            139 further nodes and SKIN_NODE (so every long segment holds a dead edge), and a last node without any edge: 215 nodes,
            1 941 directed edges.  Nobody lists the six, so the symmetric list keeps their degrees; the transpose puts them on the
            reverse walk.  Edge vectors as there: one per unordered pair, lengths in (0.7, cutoff), every pair that touches CUTOFF_NODE
            exactly at the f32 cutoff, every pair that touches SKIN_NODE beyond it.
  walk      node i lists i % 4 neighbours (i + 4, i + 8, i + 12 modulo n), so every fourth node has none; a tiny layout (node_dim 5,
            mul (3, 2, 1), 6 basis functions) at node counts on both sides of every form of the persistent walk (``XcdWalk``): a grid
            below 8 and not a multiple of 8, the first looping grid (2 049), chunks of 2 and 3 with a ragged tail, the constant chunk 32.

Second order: ``diff_message_ref`` is the definition written out in tests/test_gpu_training_ops.py::
test_message_kernels_first_and_second_order (records as free inputs), ``diff_message_eval`` the triple that
test_message_kernels_every_basis_width_in_both_precisions forms: values, the first-order gradients of a quadratic in them, and the
gradients of a quadratic in those.

Bounds: ``wq_message_cases.bound`` -- 2e-5 max(1, max|ref|) in f32 (tests/test_gpu_parity.py::test_fused_message_fwd_bwd,
test_gpu_training_ops.py), widened only to 1.5 x the CPU f32 restatement's own error; 1e-11 max(1, max|ref|) in f64."""
import functools
import math
from types import SimpleNamespace

import numpy as np
import torch

from tests import painn_kernel_cases as pc
from tests import wq_message_cases as wc

CUTOFF = wc.CUTOFF
CUTOFF_NODE, SKIN_NODE = wc.CUTOFF_NODE, wc.SKIN_NODE
BIG_DEGREES = (63, 64, 65, 127, 128, 129)
BIG_FIRST = wc.N_NODES                                   # nodes 69 .. 74, listed by nobody
POOL_FIRST = BIG_FIRST + len(BIG_DEGREES)                # nodes 75 .. 213: listed by the six, list nobody themselves
POOL_NODES = 139
N_NODES = POOL_FIRST + POOL_NODES + 1                    # 215: node 214 has no edge in any list
ISOLATED = wc.ISOLATED + (N_NODES - 1,)
LIST_KINDS = wc.LIST_KINDS
FEW_ROW_NODES = 512                                      # the few-row (STAGE) form's node limit, csrc/xeq_message_sb.hip
TOL_F32, TOL_F64 = 2e-5, 1e-11
OUTPUTS = wc.OUTPUTS

MAIN = (128, (128, 64, 32))
LAYOUTS = ((12, (8, 4, 2)), (16, (0, 16, 0)), (7, (5, 0, 3)), (200, (40, 30, 20)), (256, (86, 85, 85)), (256, (1, 0, 0)), (1, (1, 0, 0)),
           (3, (0, 0, 256)))
LAYOUT_COUNTS = (4, 8, 16, 20, 32, 5, 17, 21, 29)        # the instantiation limits, and counts whose padded head BP = roundup(B, 4) != B
KIND_COUNTS = (4, 8, 16, 20, 32)                         # the other list kinds and the BT layout

# (node_dim, mul, num_basis, rbf kind, envelope)
TABLE = tuple([(*MAIN, B, "bessel", "cosine") for B in range(1, 33)]
              + [(*MAIN, B, "gaussian", "polynomial") for B in (8, 18, 32)]
              + [(*MAIN, 13, "expbern", "cosine"), (*MAIN, 23, "expnorm", "polynomial")]
              + [(F, mul, B, "bessel", "cosine") for F, mul in LAYOUTS for B in LAYOUT_COUNTS])

WALK_LAYOUT = (5, (3, 2, 1), 6)
WALK_NODES = (1, 2, 7, 8, 9, 15, 2047, 2048, 2049, 3071, 3073, 5000, 32773)

DIFF_LAYOUTS = (MAIN, (256, (86, 85, 85)))
DIFF_COUNTS = (4, 5, 8, 9, 16, 17, 20, 21, 32)
DIFF_NAMES = ("ds", "dx", "g_h", "g_xhat", "g_rec", "gg_h", "gg_xhat", "gg_rec", "gg_w", "gg_b")


def case_id(F, mul, B, rbf_kind, cutoff_kind):
    return f"F{F}_{mul[0]}-{mul[1]}-{mul[2]}_{rbf_kind}{B}_{cutoff_kind}"


def maxb(B):
    """the record length the general kernels are instantiated for at this basis count (XEQ_SB_DISPATCH), from the count alone"""
    return 8 if B <= 8 else 16 if B <= 16 else 20 if B <= 20 else 32


# ---------------------------------------------------------------------------------------------------------------- edge lists
@functools.lru_cache(maxsize=None)
def _directed():
    base = wc.edge_list("directed").edge_index
    rng = np.random.default_rng(31)
    pool = np.concatenate([[SKIN_NODE], np.arange(POOL_FIRST, POOL_FIRST + POOL_NODES)])
    assert len(pool) >= max(BIG_DEGREES)
    rows = [base]
    for k, deg in enumerate(BIG_DEGREES):
        nbrs = np.concatenate([[SKIN_NODE], rng.choice(pool[1:], size=deg - 1, replace=False)])     # distinct, the dead edge among them
        rows.append(np.stack([np.full(deg, BIG_FIRST + k), rng.permutation(nbrs)]))
    return np.concatenate(rows, axis=1).astype(np.int64)


def _views(ei, n, kind):
    ei = np.ascontiguousarray(ei, dtype=np.int64)
    c_rowptr, c_perm = pc.csr_view(ei[0], n)
    if kind == "symmetric":
        n_rowptr, n_perm = c_rowptr, pc.reverse_edge_map(ei, n)
    else:
        n_rowptr, n_perm = pc.csr_view(ei[1], n)
    return SimpleNamespace(kind=kind, n_nodes=n, n_edges=ei.shape[1], edge_index=ei, c_rowptr=c_rowptr, c_perm=c_perm, n_rowptr=n_rowptr,
                           n_perm=n_perm, symmetric=kind == "symmetric")


@functools.lru_cache(maxsize=None)
def edge_list(kind, extra_isolated=0):
    """The degrees list as wq_message_cases.edge_list hands its own out: edge_index [2, E] int64 with the forward view (c_rowptr, c_perm)
    and the reverse view (n_rowptr, n_perm).  ``extra_isolated``: that many nodes without an edge appended (the few-row limit)."""
    n, base = N_NODES, _directed()
    if kind == "directed":
        ei = base
    elif kind == "transpose":
        ei = base[::-1][:, np.random.default_rng(21).permutation(base.shape[1])]
    elif kind == "shuffled":
        ei = base[:, np.random.default_rng(22).permutation(base.shape[1])]
    elif kind == "symmetric":
        key = np.unique(np.concatenate([base[0] * n + base[1], base[1] * n + base[0]]))
        ei = np.stack([key // n, key % n])
    else:
        raise KeyError(kind)
    return _views(ei, n + extra_isolated, kind)


@functools.lru_cache(maxsize=None)
def walk_list(n):
    """Node i lists i % 4 nodes: i + 4, i + 8, i + 12 (modulo n; below 16 nodes i + 1, i + 2, i + 3).  Center-sorted, every fourth node
    without a walked edge -- on the reverse walk too, where away from the wrap-around node j is listed by j % 4 nodes."""
    i = np.arange(n, dtype=np.int64)
    center = np.repeat(i, i % 4)
    k = np.arange(len(center)) - np.repeat(np.cumsum(i % 4) - i % 4, i % 4)
    nbr = (center + (1 + k) * (4 if n >= 16 else 1)) % max(n, 1)
    assert np.all(center != nbr)
    return _views(np.stack([center, nbr]), n, "walk")


@functools.lru_cache(maxsize=None)
def _pair_vectors():
    """[n, n, 3] f32: the vector of edge (i, j), antisymmetric in (i, j) (wq_message_cases._pair_vectors over the 215 nodes)"""
    n, rng = N_NODES, np.random.default_rng(32)
    u = rng.standard_normal((n, n, 3))
    u /= np.linalg.norm(u, axis=2, keepdims=True)
    length = rng.uniform(0.7, CUTOFF, size=(n, n))
    skin = np.zeros((n, n), dtype=bool)
    skin[SKIN_NODE, :] = skin[:, SKIN_NODE] = True
    length[skin] = rng.uniform(1.0, 1.2, size=int(skin.sum())) * CUTOFF
    vec = (u * length[:, :, None]).astype(np.float32)
    c32 = np.float32(CUTOFF)
    for j in range(n):                                    # along an axis: the f32 norm is the f32 cutoff itself
        vec[CUTOFF_NODE, j] = vec[j, CUTOFF_NODE] = 0.0
        vec[CUTOFF_NODE, j, j % 3] = vec[j, CUTOFF_NODE, j % 3] = c32 if j % 2 == 0 else -c32
    upper = np.triu(np.ones((n, n), dtype=bool), 1)
    return np.where(upper[:, :, None], vec, -np.transpose(vec, (1, 0, 2)))


def edge_vectors(el):
    """(vec [E, 3] f64 holding f32 values, mask of the edges at or beyond the cutoff)"""
    ei = el.edge_index
    if el.kind == "walk":                                 # free inputs per edge; every eleventh edge in the skin
        rng = np.random.default_rng([33, el.n_nodes])
        u = rng.standard_normal((el.n_edges, 3))
        u /= np.maximum(np.linalg.norm(u, axis=1, keepdims=True), 1e-300)
        length = rng.uniform(0.7, 0.99 * CUTOFF, size=el.n_edges)
        skin = np.arange(el.n_edges) % 11 == 5
        length[skin] = 1.1 * CUTOFF
        vec = (u * length[:, None]).astype(np.float32)
        exact = np.zeros(el.n_edges, dtype=bool)
    else:
        vec = _pair_vectors()[ei[0], ei[1]]
        exact = (ei[0] == CUTOFF_NODE) | (ei[1] == CUTOFF_NODE)
        skin = ((ei[0] == SKIN_NODE) | (ei[1] == SKIN_NODE)) & ~exact
        assert exact.any() and skin.any()
    d = np.linalg.norm(vec.astype(np.float64), axis=1)
    beyond = d >= CUTOFF
    assert np.array_equal(beyond, exact | skin) and np.all(d[exact] == CUTOFF) and (el.n_edges == 0 or d.min() > 0.69)
    assert np.all(np.linalg.norm(vec, axis=1)[~beyond] < np.float32(CUTOFF))          # ... in f32 arithmetic too
    return torch.tensor(vec.astype(np.float64)).reshape(-1, 3), torch.tensor(beyond)


# ---------------------------------------------------------------------------------------------------------------- references
@functools.lru_cache(maxsize=None)
def radial_params(rbf_kind, cutoff_kind, B):
    """(what the oracle's functions take, p0, p1 for the kernels), f64 holding f32 values.  Bessel / Gaussian / expnorm: the jittered
    parameters of wq_message_cases.radial_params.  expbern: the project's module as it stands; its kernel arguments are
    softplus(alpha) per basis function and log C(B - 1, k), and the oracle is handed the raw alpha whose softplus that is."""
    if rbf_kind != "expbern":
        p0, p1 = wc.radial_params(rbf_kind, cutoff_kind, B)
        return ((p0,) if p1 is None else (p0, p1)), p0, p1
    sp = pc.radial_spec(rbf_kind, cutoff_kind, B, CUTOFF)
    f = lambda p: pc._f32(p.double().numpy())
    p0, p1 = f(sp["p0"]).reshape(1, -1), f(sp["p1"]).reshape(1, -1)
    assert torch.all(p0 == p0[0, 0])
    alpha_raw = torch.log(torch.expm1(p0[0, 0]))          # the oracle applies softplus itself: its f64 alpha is the kernels' f32 p0
    _, logc, n, v = (f(p) for p in sp["rbf_params"])
    assert torch.equal(logc.reshape(-1), p1.reshape(-1))
    return (alpha_raw, logc, n, v), p0, p1


def _case(F, mul, B, rbf_kind, cutoff_kind, el, tag):
    mul = tuple(int(m) for m in mul)
    n, C, D = el.n_nodes, sum(mul), mul[0] + 3 * mul[1] + 5 * mul[2]
    H = F + 2 * C
    rng = np.random.default_rng([F, *mul, B, pc.RBF_NAMES.index(rbf_kind), pc.CUTOFF_NAMES.index(cutoff_kind)])
    vec, beyond = edge_vectors(el)
    params, p0, p1 = radial_params(rbf_kind, cutoff_kind, B)
    r = lambda *shape: pc._f32(rng.standard_normal(shape))
    c = SimpleNamespace(mul=mul, B=B, F=F, C=C, D=D, H=H, n=n, rbf_kind=rbf_kind, cutoff_kind=cutoff_kind, cutoff=CUTOFF, edges=el, vec=vec,
                        beyond=beyond, params=params, p0=p0, p1=p1, h=r(n, H), xhat=r(n, D), s=r(n, F), x=r(n, D),
                        W=pc._f32(rng.standard_normal((H, B)) / math.sqrt(B)), b=r(H), g_s=r(n, F), g_x=r(n, D))
    c.id = case_id(F, mul, B, rbf_kind, cutoff_kind) + tag
    c.ref = message_eval(c, torch.float64)
    c.ref32 = message_eval(c, torch.float32)
    return c


@functools.lru_cache(maxsize=None)
def message_case(F, mul, B, rbf_kind="bessel", cutoff_kind="cosine", list_kind="directed", extra_isolated=0):
    """A case on the degrees list (``extra_isolated``: a case of its own, with its own draws, on the list with that many more nodes)."""
    tag = "" if list_kind == "directed" else f"_{list_kind}"
    return _case(F, mul, B, rbf_kind, cutoff_kind, edge_list(list_kind, extra_isolated), tag + (f"_n{N_NODES + extra_isolated}" if extra_isolated else ""))


@functools.lru_cache(maxsize=None)
def walk_case(n):
    F, mul, B = WALK_LAYOUT
    return _case(F, mul, B, "bessel", "cosine", walk_list(n), f"_walk{n}")


def message_eval(c, dtype, W=None, edge_index=None, vec=None, y00=None, residual=True):
    """Forward outputs and autograd's gradients w.r.t. (h, xhat, vec, s, x) in ``dtype`` (OUTPUTS).  ``W`` / ``edge_index`` with its
    ``vec`` restate the case with one thing changed (the power checks of the host test); ``y00`` / ``residual=False``: the forward with
    another l = 0 harmonic / without the residual terms (XEQ_SB_Y0_ZERO, s_in = x_in = NULL)."""
    t = lambda v: v.detach().to(dtype).clone().requires_grad_()
    h, xhat, vec, s, x = t(c.h), t(c.xhat), t(c.vec if vec is None else vec), t(c.s), t(c.x)
    if not residual:
        s, x = t(torch.zeros_like(c.s)), t(torch.zeros_like(c.x))
    ei = torch.tensor(c.edges.edge_index if edge_index is None else edge_index)
    out = wc.message_ref(c.mul, h, xhat, vec, s, x, (c.W if W is None else W).to(dtype), c.b.to(dtype), tuple(p.to(dtype) for p in c.params), ei,
                         c.rbf_kind, c.cutoff_kind, c.cutoff, y00=y00)
    g = torch.autograd.grad(out, [h, xhat, vec, s, x], [c.g_s.to(dtype), c.g_x.to(dtype)])
    return dict(zip(OUTPUTS, [o.detach() for o in out] + list(g)))


# ------------------------------------------------------------------------------------------------------------- second order
def diff_message_ref(h, xhat, rec, w, b, edge_index, B, F, mul):
    """(sum_e msg_s, sum_e msg_x) of ops.DiffMessage: the records [head (B) | 0 to BP | f | Y_1 (3) | Y_2 (5) | 3 unused] are free inputs"""
    n, E, C, bp = h.shape[0], rec.shape[0], sum(mul), (B + 3) & ~3
    center, nbr = edge_index[0].long(), edge_index[1].long()
    filt = rec[:, :B] @ w.t() + rec[:, bp:bp + 1] * b
    g = h[nbr] * filt
    ds = torch.zeros(n, F, dtype=h.dtype).index_add(0, center, g[:, 2 * C:])
    y = [torch.ones(E, 1, dtype=h.dtype), rec[:, bp + 1:bp + 4], rec[:, bp + 4:bp + 9]]
    xj, parts, ch, off = xhat[nbr], [], 0, 0
    for l in range(3):
        k, m = 2 * l + 1, mul[l]
        parts.append((xj[:, off:off + m * k].view(E, m, k) * g[:, ch:ch + m, None] + y[l][:, None, :] * g[:, C + ch:C + ch + m, None]).reshape(E, m * k))
        ch, off = ch + m, off + m * k
    D = off
    return ds, torch.zeros(n, D, dtype=h.dtype).index_add(0, center, torch.cat(parts, 1))


@functools.lru_cache(maxsize=None)
def diff_case(F, mul, B):
    """Inputs of ops.DiffMessage on the directed degrees list with the f64 triple ``ref`` and its f32 restatement ``ref32`` (DIFF_NAMES)"""
    mul = tuple(int(m) for m in mul)
    el = edge_list("directed")
    n, E, C, D, bp = el.n_nodes, el.n_edges, sum(mul), mul[0] + 3 * mul[1] + 5 * mul[2], (B + 3) & ~3
    H = F + 2 * C
    rng = np.random.default_rng([77, F, *mul, B])
    r = lambda *shape: pc._f32(rng.standard_normal(shape))
    c = SimpleNamespace(F=F, mul=mul, B=B, C=C, D=D, H=H, n=n, edges=el, h=r(n, H), xhat=r(n, D), rec=r(E, bp + 12),
                        w=pc._f32(rng.standard_normal((H, B)) / math.sqrt(B)), b=r(H), id=f"diff_F{F}_{mul[0]}-{mul[1]}-{mul[2]}_B{B}")
    c.ref = diff_message_eval(c, torch.float64)
    c.ref32 = diff_message_eval(c, torch.float32)
    return c


def diff_triple(fn, leaves):
    """values, d/d(h, xhat, rec) of sum(values^2) with the graph kept, d/d(h, xhat, rec, w, b) of the sum of their squares"""
    ds, dx = fn(*leaves)
    first = torch.autograd.grad((ds * ds).sum() + (dx * dx).sum(), leaves[:3], create_graph=True)
    second = torch.autograd.grad(sum((t * t).sum() for t in first), leaves)
    return dict(zip(DIFF_NAMES, [t.detach() for t in (ds, dx, *first, *second)]))


def diff_message_eval(c, dtype, w=None, edge_index=None, rec=None):
    leaves = [v.detach().to(dtype).clone().requires_grad_() for v in (c.h, c.xhat, c.rec if rec is None else rec, c.w if w is None else w, c.b)]
    ei = torch.tensor(c.edges.edge_index if edge_index is None else edge_index)
    return diff_triple(lambda *a: diff_message_ref(*a, ei, c.B, c.F, c.mul), leaves)
