"""Cases and f64 references for the wave / quad matrix-core message kernels (csrc/xeq_message_wq.hip) and the matrix-core
filter-gradient kernel (csrc/xeq_train.hip), run through the public ops by tests/test_gpu_wq_message.py at every basis count and
channel layout that ``xeq_message_wq_supported`` admits.  CPU only; no test functions here (tests/test_wq_message_cases_host.py
checks this module).

Every input is drawn in f64 and rounded to f32 once: the kernels, the f32 restatement and the f64 reference see the same numbers.

Reference (plain torch, dtype-generic): the arithmetic of tests/test_gpu_parity.py::_message_case -- the radial basis, envelope and
harmonics of oracle/xpainn_oracle.py, the filter rbf W^T + b times the envelope, the two gated products, ``index_add`` -- with every
reverse quantity (dL/d{h, xhat, vec, s, x, W, b, p0, p1}) from torch.autograd for the cotangents (g_s, g_x) of the case.

Edge lists: the 64-node lists of tests/painn_kernel_cases.py (out-degrees {0, 1, 15, 16, 17, 31, 32, 33, 48}) with four more nodes of
degree 2, 3, 4, 5 that nobody lists -- with them every residue of the quad padding (a node's edges are padded to whole quads of four
slots) occurs on consecutive walked rows -- and a last node without any edge: 69 nodes, 1 365 directed edges.  Kinds as there:
directed / transpose / shuffled / symmetric.  Edge vectors are free inputs, one per unordered pair of nodes (negated for the other
direction, so the symmetric list is one the mirror walk may be used on): random directions, lengths in (0.7, cutoff); pairs that
touch CUTOFF_NODE exactly at the cutoff, pairs that touch SKIN_NODE beyond it.

Bound per tensor (tests/test_gpu_parity.py: 2e-5 for outputs and first-order gradients, 3e-5 for filter gradients, of
max(1, max|ref|)), widened only to 1.5 x the f32 restatement's own error (tests/test_gpu_tile_edges.py): ``bound``."""
import functools
import math
from types import SimpleNamespace

import numpy as np
import torch

from oracle import xpainn_oracle as orc
from tests import painn_kernel_cases as pc

CUTOFF = 4.0
CUTOFF_NODE, SKIN_NODE = pc.CUTOFF_NODE, pc.SKIN_NODE
SMALL_DEGREES = (2, 3, 4, 5)                       # nodes 64 .. 67, listed by nobody
N_NODES = pc.N_NODES + len(SMALL_DEGREES) + 1      # 69: node 68 has no edge in any list
ISOLATED = pc.ISOLATED + (N_NODES - 1,)
LIST_KINDS = pc.LIST_KINDS
TOL_OUT, TOL_PARAM = 2e-5, 3e-5                    # tests/test_gpu_parity.py: fused message / its parameter gradients, f32

OUTPUTS = ("s_out", "x_out", "grad_h", "grad_xhat", "grad_vec", "grad_s", "grad_x")
PARAM_GRADS = ("grad_W", "grad_b", "grad_p0", "grad_p1")

MUL_MAIN = (128, 64, 32)
BESSEL_COUNTS = (1, 7, 8, 9, 11, 12, 15, 16, 17, 20, 21, 22, 23, 24, 25, 27, 28, 29, 30, 31)   # 11 / 12: the filter-gradient limit
LAYOUTS = ((32, 0, 0), (32, 32, 0), (32, 0, 32), (64, 64, 64), (160, 96, 64), (256, 32, 32))
PER_INSTANTIATION = (8, 20, 22, 26)                # one basis count per instantiated KS 1, 3, 4, 8

# (mul, num_basis, rbf kind, envelope)
TABLE = tuple([(MUL_MAIN, B, "bessel", "cosine") for B in BESSEL_COUNTS]
              + [(MUL_MAIN, B, "gaussian", "polynomial") for B in (8, 18, 19)]
              + [(MUL_MAIN, 23, "expnorm", "cosine")]
              + [(mul, B, "bessel", "cosine") for mul in LAYOUTS for B in PER_INSTANTIATION])


def case_id(mul, B, rbf_kind, cutoff_kind):
    return f"{mul[0]}-{mul[1]}-{mul[2]}_{rbf_kind}{B}_{cutoff_kind}"


def bound(ref, ref32, tol):
    """max(tol max(1, max|ref|), 1.5 err32), err32 = |f32 restatement - f64 reference|"""
    return max(tol * max(1.0, float(ref.abs().max())), 1.5 * float((ref32.double() - ref).abs().max()))


# ---------------------------------------------------------------------------------------------------------------- edge lists
@functools.lru_cache(maxsize=None)
def _directed():
    base = pc.edge_list("directed").edge_index
    rng = np.random.default_rng(23)
    pool = np.array([j for j in range(pc.N_NODES) if j not in pc.ISOLATED and j not in pc.SOURCES])
    rows = [base]
    for k, deg in enumerate(SMALL_DEGREES):
        nbrs = rng.choice(pool, size=deg, replace=False)
        rows.append(np.stack([np.full(deg, pc.N_NODES + k), nbrs]))
    return np.concatenate(rows, axis=1).astype(np.int64)


@functools.lru_cache(maxsize=None)
def edge_list(kind):
    """As painn_kernel_cases.edge_list, over the 69 nodes: edge_index [2, E] int64 with the forward view (c_rowptr, c_perm) and the
    reverse view (n_rowptr, n_perm) in numpy, independent of the library's own sort."""
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
    ei = np.ascontiguousarray(ei, dtype=np.int64)
    c_rowptr, c_perm = pc.csr_view(ei[0], n)
    if kind == "symmetric":
        n_rowptr, n_perm = c_rowptr, pc.reverse_edge_map(ei, n)
    else:
        n_rowptr, n_perm = pc.csr_view(ei[1], n)
    return SimpleNamespace(kind=kind, n_nodes=n, n_edges=ei.shape[1], edge_index=ei, c_rowptr=c_rowptr, c_perm=c_perm, n_rowptr=n_rowptr,
                           n_perm=n_perm, symmetric=kind == "symmetric")


@functools.lru_cache(maxsize=None)
def _pair_vectors():
    """[n, n, 3] f32: the vector of edge (i, j), antisymmetric in (i, j)"""
    n, rng = N_NODES, np.random.default_rng(24)
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
    vec = _pair_vectors()[ei[0], ei[1]]
    d = np.linalg.norm(vec.astype(np.float64), axis=1)
    exact = (ei[0] == CUTOFF_NODE) | (ei[1] == CUTOFF_NODE)
    skin = ((ei[0] == SKIN_NODE) | (ei[1] == SKIN_NODE)) & ~exact
    beyond = d >= CUTOFF
    assert exact.any() and skin.any() and np.array_equal(beyond, exact | skin) and np.all(d[exact] == CUTOFF) and d.min() > 0.69
    assert np.all(np.linalg.norm(vec, axis=1)[~beyond] < np.float32(CUTOFF))          # ... in f32 arithmetic too
    return torch.tensor(vec.astype(np.float64)), torch.tensor(beyond)


# ---------------------------------------------------------------------------------------------------------------- references
def irreps_of(mul):
    return [(m, l, 1 if l % 2 == 0 else -1) for l, m in enumerate(mul) if m > 0]


def to_bt(x, mul):
    """e3nn rows [N, D] -> the BT layout (include/xeq.h: per l a row-major [N (2l + 1), mul_l] matrix), flat"""
    n, off, parts = x.shape[0], 0, []
    for l, m in enumerate(mul):
        d = 2 * l + 1
        parts.append(x[:, off:off + m * d].reshape(n, m, d).transpose(1, 2).reshape(-1))
        off += m * d
    return torch.cat(parts)


def from_bt(flat, mul, n):
    off, parts = 0, []
    for l, m in enumerate(mul):
        d = 2 * l + 1
        parts.append(flat[off:off + n * m * d].reshape(n, d, m).transpose(1, 2).reshape(n, m * d))
        off += n * m * d
    return torch.cat(parts, dim=1)


def message_ref(mul, h, xhat, vec, s, x, W, b, params, edge_index, rbf_kind, cutoff_kind, cutoff, y00=None):
    """(s_out, x_out) of one message block; ``params``: the basis parameters as the oracle's functions take them (p0[, p1]).  The scalar
    width is what h holds beyond its 2 C gate columns (the wq kernels: mul[0]).  ``y00``: the value of the l = 0 harmonic when it is not
    1 (tests/sb_message_cases.py: XEQ_SB_Y0_ZERO)."""
    irreps, C = irreps_of(mul), sum(mul)
    F = h.shape[1] - 2 * C
    center, nbr = edge_index[0].long(), edge_index[1].long()
    rbf, fcut, _ = pc.radial_ref(vec, rbf_kind, cutoff_kind, params, cutoff)
    rsh = orc.spherical_harmonics(irreps, vec[:, [1, 2, 0]])
    if y00 is not None:
        rsh = torch.cat([rsh[:, :mul[0]] * y00, rsh[:, mul[0]:]], dim=1)
    filt = torch.nn.functional.linear(rbf, W, b) * fcut
    g_state, g_edge, m_s = torch.split(h.index_select(0, nbr) * filt, [C, C, F], dim=-1)
    m_x = orc.elementwise_tp(irreps, xhat.index_select(0, nbr), g_state) + orc.elementwise_tp(irreps, rsh, g_edge)
    return s.index_add(0, center, m_s), x.index_add(0, center, m_x)


@functools.lru_cache(maxsize=None)
def radial_params(rbf_kind, cutoff_kind, B):
    """p0 / p1 [1, B] (f64 holding f32 values) from the project's own modules, each moved by about a percent so that no gradient is
    taken at a special point; the kind codes for the kernels"""
    sp = pc.radial_spec(rbf_kind, cutoff_kind, B, CUTOFF)
    rng = np.random.default_rng([B, pc.RBF_NAMES.index(rbf_kind)])
    jig = lambda p: None if p is None else pc._f32(p.double().numpy().reshape(1, -1) * (1 + 0.01 * rng.standard_normal((1, B))))
    assert rbf_kind in ("bessel", "gaussian", "expnorm")          # kinds whose (p0, p1) are the oracle's own arguments
    return jig(sp["p0"]), jig(sp["p1"])


@functools.lru_cache(maxsize=None)
def message_case(mul, B, rbf_kind="bessel", cutoff_kind="cosine", list_kind="directed", first_block=False):
    """``first_block``: xhat zero on every l > 0 column (what XEQ_XHAT_HIGHER_L_ZERO promises)"""
    mul = tuple(int(m) for m in mul)
    el = edge_list(list_kind)
    n, F, C, D = el.n_nodes, mul[0], sum(mul), mul[0] + 3 * mul[1] + 5 * mul[2]
    H = F + 2 * C
    rng = np.random.default_rng([*mul, B, pc.RBF_NAMES.index(rbf_kind), pc.CUTOFF_NAMES.index(cutoff_kind)])
    vec, beyond = edge_vectors(el)
    p0, p1 = radial_params(rbf_kind, cutoff_kind, B)
    r = lambda *shape: pc._f32(rng.standard_normal(shape))
    c = SimpleNamespace(mul=mul, B=B, F=F, C=C, D=D, H=H, n=n, rbf_kind=rbf_kind, cutoff_kind=cutoff_kind, cutoff=CUTOFF, edges=el,
                        first_block=first_block, vec=vec, beyond=beyond, p0=p0, p1=p1, h=r(n, H), xhat=r(n, D), s=r(n, F), x=r(n, D),
                        W=pc._f32(rng.standard_normal((H, B)) / math.sqrt(B)), b=r(H), g_s=r(n, F), g_x=r(n, D))
    if first_block:
        c.xhat[:, F:] = 0.0
    c.id = case_id(mul, B, rbf_kind, cutoff_kind) + f"_{list_kind}" + ("_first" if first_block else "")
    c.ref = message_eval(c, torch.float64)
    c.ref32 = message_eval(c, torch.float32)
    return c


def message_eval(c, dtype, W=None, b=None):
    """Forward outputs and autograd's gradients (OUTPUTS + PARAM_GRADS; grad_p1 None for a basis without p1) in ``dtype``.  ``W`` / ``b``
    restate the case with a changed filter (the power checks of the host test)."""
    t = lambda v: None if v is None else v.detach().to(dtype).clone().requires_grad_()
    h, xhat, vec, s, x = t(c.h), t(c.xhat), t(c.vec), t(c.s), t(c.x)
    W, b, p0, p1 = t(c.W if W is None else W), t(c.b if b is None else b), t(c.p0), t(c.p1)
    params = (p0,) if p1 is None else (p0, p1)
    out = message_ref(c.mul, h, xhat, vec, s, x, W, b, params, torch.tensor(c.edges.edge_index), c.rbf_kind, c.cutoff_kind, c.cutoff)
    leaves = [h, xhat, vec, s, x, W, b, p0] + ([] if p1 is None else [p1])
    g = list(torch.autograd.grad(out, leaves, [c.g_s.to(dtype), c.g_x.to(dtype)]))
    if p1 is None:
        g.append(None)
    g[7] = g[7].reshape(-1)
    g[8] = None if g[8] is None else g[8].reshape(-1)
    return dict(zip(OUTPUTS + PARAM_GRADS, [o.detach() for o in out] + g))
