"""Cases and f64 references for the C entry points of csrc/xeq_painn.hip, called one by one (tests/test_gpu_painn_kernels.py) at every
width, basis count, radial kind, envelope and list kind that ``xeq_painn_supported`` admits.  CPU only; no test functions here.

The scalar MLP's output ``h`` and the update MLP's output ``a`` are plain random inputs, so the PaiNN kernels stand alone and no width
depends on the 128-wide MLP kernels.  Every input is drawn in f64 and rounded to f32 once: the kernels, the f32 restatement and the f64
reference see the same numbers.

References (plain torch, dtype-generic, differentiable once):
  message_ref     tests/painn_oracle.py::message with ``h`` given; radial functions and envelopes of oracle/xpainn_oracle.py
  update_uv_ref   U, V, <U, V>, [s | |V|]      (|V| = torch.linalg.norm: a zero gradient at V = 0)
  update_out_ref  s + a_sv <U, V> + a_ss, x + a_vv U
Reverse quantities are torch.autograd.grad of these with given cotangents (message_eval / update_eval).

Edge lists and their CSR views are built in numpy (stable argsort by center for the forward walk, by neighbour for the reverse walk,
int32 row pointers, int32 perm or None when already sorted), so the library's own xeq_csr_by_key is not part of what is compared.

Node count.  The issue asks for "about 40 nodes" and for out-degrees {0, 1, 15, 16, 17, 31, 32, 33, 48} with distinct neighbours.  A node
of degree 48 needs 48 other listable nodes, two degree-0 nodes stay unlisted (isolated in every list: an interior one and the last one),
and six nodes of degrees 1, 15, 16, 17, 32, 33 are listed by nobody, so that the SYMMETRIC list (union with the transpose) has exactly
these degrees on them.  That gives 64 nodes = 7 turns through the nine degrees + the last degree-0 node, 1 351 directed edges.

Bound per output tensor: the project's rule (tests/test_gpu_painn.py::_bound), restated in ``bound``."""
import functools
import math
from types import SimpleNamespace

import numpy as np
import torch

from oracle import xpainn_oracle as orc

DEGREES = (0, 1, 15, 16, 17, 31, 32, 33, 48)
N_NODES = 64                      # 7 x 9 + 1: node 63 has degree 0
ISOLATED = (9, 63)                # degree 0 and listed by nobody: an interior position and the last node
SOURCES = (1, 2, 3, 4, 6, 7)      # out-degrees 1, 15, 16, 17, 32, 33, listed by nobody: the symmetric list keeps these degrees
CLAIMED = (15, 16, 17, 32, 33)    # segment lengths every list kind has on its walked row
CUTOFF_NODE = 1                   # every edge that touches this node has length exactly ``cutoff``
SKIN_NODE = 10                    # every edge centred on this node (out-degree 1) lies in the skin (1.0, 1.2) cutoff
LIST_KINDS = ("directed", "transpose", "shuffled", "symmetric")
RBF_NAMES = ("bessel", "gaussian", "expbern", "expnorm")
CUTOFF_NAMES = ("cosine", "polynomial")
KPAD = 32                         # padded basis width of the packed filter (num_basis + 1 <= 32)
FEW_ROWS = 2048                   # xeq_painn_few_rows_limit(), asserted by the GPU tests


def bound(ref, ref32):
    """max(1e-4 max(1, max|ref|), 1.5 err32), err32 = |f32 restatement - f64 reference|: tests/test_gpu_painn.py::_bound."""
    return max(1e-4 * max(1.0, float(ref.abs().max())), 1.5 * float((ref32.double() - ref).abs().max()))


# ---------------------------------------------------------------------------------------------------------------- references
def radial_ref(vec, rbf_kind, cutoff_kind, rbf_params, cutoff):
    """(rbf [E, B], fcut [E, 1], u [E, 3]) of one edge vector each; ``rbf_params`` as radial_spec()["rbf_params"]."""
    d = torch.linalg.norm(vec, dim=-1, keepdim=True)
    P = [p.to(vec.dtype) for p in rbf_params]
    if rbf_kind == "bessel":
        rbf = orc.bessel_rbf(d, P[0].reshape(1, -1), cutoff)
    elif rbf_kind == "gaussian":
        rbf = orc.gaussian_rbf(d, P[0].reshape(1, -1), P[1].reshape(1, -1))
    elif rbf_kind == "expbern":
        rbf = orc.exp_bernstein_rbf(d, P[0], P[1].reshape(1, -1), P[2].reshape(1, -1), P[3].reshape(1, -1))
    elif rbf_kind == "expnorm":
        rbf = orc.exp_norm_rbf(d, P[0].reshape(1, -1), P[1].reshape(1, -1))
    else:
        raise NotImplementedError(rbf_kind)
    if cutoff_kind == "cosine":
        fcut = orc.cosine_cutoff(d, cutoff)
    elif cutoff_kind == "polynomial":
        fcut = orc.polynomial_cutoff(d, cutoff)
    else:
        raise NotImplementedError(cutoff_kind)
    return rbf, fcut, vec / d


def message_from_basis(s, x, h, rbf, fcut, u, edge_index, w, b):
    """tests/painn_oracle.py::message behind the scalar MLP and the radial functions (w: rbf_lin.weight [3F, B], b: its bias)."""
    center, nbr = edge_index[0].long(), edge_index[1].long()
    F = s.shape[1]
    filt = (rbf @ w.T + b) * fcut
    m_s, g_edge, g_state = torch.split(h[nbr] * filt, F, dim=-1)
    m_v = x[nbr] * g_state.unsqueeze(1) + g_edge.unsqueeze(1) * u.unsqueeze(-1)
    return s.index_add(0, center, m_s), x.index_add(0, center, m_v)


def message_ref(s, x, h, vec, edge_index, w, b, rbf_kind, cutoff_kind, rbf_params, cutoff):
    return message_from_basis(s, x, h, *radial_ref(vec, rbf_kind, cutoff_kind, rbf_params, cutoff), edge_index, w, b)


def update_uv_ref(s, x, wu, wv):
    """U, V [N, 3, F], <U, V> [N, F], [s | |V|] [N, 2F]"""
    U, V = x @ wu.T, x @ wv.T
    return U, V, (U * V).sum(1), torch.cat([s, torch.linalg.norm(V, dim=1)], dim=-1)


def update_out_ref(s, x, a, U, ip):
    a_ss, a_vv, a_sv = torch.split(a, s.shape[1], dim=-1)
    return s + a_sv * ip + a_ss, x + a_vv.unsqueeze(1) * U


@functools.lru_cache(maxsize=None)
def radial_spec(rbf_kind, cutoff_kind, num_basis, cutoff):
    """The project's modules for this choice: their parameters for the reference (``rbf_params``), p0 / p1 and the kind codes for the
    kernel.  Built in f32, the form the kernels are handed; the f64 reference widens the same numbers."""
    from xequinet_amd import lib
    from xequinet_amd.nn.rbf import resolve_cutoff, resolve_rbf

    assert torch.get_default_dtype() == torch.float32
    rbf, env = resolve_rbf(rbf_kind, num_basis, cutoff), resolve_cutoff(cutoff_kind, cutoff)
    p0, p1 = rbf.params()
    params = {"bessel": lambda: (rbf.freq,), "gaussian": lambda: (rbf.mean, rbf.std),
              "expbern": lambda: (rbf._alpha, rbf.logc, rbf.n, rbf.v), "expnorm": lambda: (rbf.beta, rbf.mu)}[rbf_kind]()
    return {"rbf_kind": rbf_kind, "cutoff_kind": cutoff_kind, "num_basis": num_basis, "cutoff": float(env.cutoff),
            "rbf_params": tuple(p.detach().clone() for p in params),
            "p0": p0.detach().float().contiguous().clone(), "p1": None if p1 is None else p1.detach().float().contiguous().clone(),
            "rbf_code": lib.RBF_KINDS[rbf.kind], "cutoff_code": lib.CUTOFF_KINDS[env.kind]}


# ---------------------------------------------------------------------------------------------------------------- edge lists
def csr_view(keys, n):
    """(int32 rowptr [n + 1], int32 perm [E] or None) of the stable sort of ``keys``."""
    order = np.argsort(keys, kind="stable")
    rowptr = np.zeros(n + 1, dtype=np.int32)
    rowptr[1:] = np.cumsum(np.bincount(keys, minlength=n))
    perm = None if np.array_equal(order, np.arange(len(keys))) else order.astype(np.int32)
    return rowptr, perm


def reverse_edge_map(edge_index, n):
    """Position of (j, i) for every edge (i, j) of a center-sorted list with ascending unique neighbours."""
    key = edge_index[0] * n + edge_index[1]
    assert np.all(np.diff(key) > 0)
    rev = np.searchsorted(key, edge_index[1] * n + edge_index[0])
    assert np.array_equal(key[rev], edge_index[1] * n + edge_index[0]), "the list is not symmetric"
    return rev.astype(np.int32)


def _directed(rng):
    rows = []
    for k in range(N_NODES):
        pool = np.array([j for j in range(N_NODES) if j != k and j not in ISOLATED and j not in SOURCES])
        nbrs = rng.choice(pool, size=DEGREES[k % len(DEGREES)], replace=False)   # random order, distinct
        rows.append(np.stack([np.full(len(nbrs), k), nbrs]))
    return np.concatenate(rows, axis=1).astype(np.int64)


@functools.lru_cache(maxsize=None)
def edge_list(kind):
    """``directed`` | ``transpose`` (rows swapped, then shuffled) | ``shuffled`` | ``symmetric``: edge_index [2, E] int64 with the forward
    view (c_rowptr, c_perm) and the reverse view (n_rowptr, n_perm); the symmetric list walks the reverse-edge map over c_rowptr in
    reverse, as ops.EdgeGraph(symmetric=True) does."""
    n = N_NODES
    base = _directed(np.random.default_rng(20))
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
    c_rowptr, c_perm = csr_view(ei[0], n)
    if kind == "symmetric":
        n_rowptr, n_perm = c_rowptr, reverse_edge_map(ei, n)
    else:
        n_rowptr, n_perm = csr_view(ei[1], n)
    return SimpleNamespace(kind=kind, n_nodes=n, n_edges=ei.shape[1], edge_index=ei, c_rowptr=c_rowptr, c_perm=c_perm, n_rowptr=n_rowptr,
                           n_perm=n_perm, symmetric=kind == "symmetric")


def edge_vectors(el, cutoff, rng):
    """[E, 3] f32-representable vectors, inputs of their own: random directions, lengths uniform in (0.3, 0.95 cutoff); the edges
    centred on SKIN_NODE and six more in the skin (1.0, 1.2) cutoff; every edge that touches CUTOFF_NODE exactly ``cutoff`` long
    (along an axis, so that the f32 norm is the f32 cutoff itself).  Returns (vec f64, mask of the edges at or beyond the cutoff)."""
    E = el.n_edges
    u = rng.standard_normal((E, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    length = rng.uniform(0.3, 0.95 * cutoff, size=E)
    skin = el.edge_index[0] == SKIN_NODE
    skin[rng.choice(E, size=6, replace=False)] = True
    length[skin] = rng.uniform(1.0, 1.2, size=int(skin.sum())) * cutoff
    vec = (u * length[:, None]).astype(np.float32)
    exact = (el.edge_index[0] == CUTOFF_NODE) | (el.edge_index[1] == CUTOFF_NODE)
    assert exact.any()
    c32 = np.float32(cutoff)
    for q, e in enumerate(np.nonzero(exact)[0]):
        vec[e] = 0.0
        vec[e, q % 3] = c32 if q % 2 == 0 else -c32
    d = np.linalg.norm(vec.astype(np.float64), axis=1)
    assert d.min() > 0.29
    beyond = d >= float(c32)
    assert np.array_equal(beyond, skin | exact)
    return torch.tensor(vec.astype(np.float64)), torch.tensor(beyond)


# --------------------------------------------------------------------------------------------------------------------- cases
def _f32(a):
    """f64 tensor of values that f32 holds exactly"""
    return torch.tensor(np.asarray(a, dtype=np.float32).astype(np.float64))


@functools.lru_cache(maxsize=None)
def message_case(F, B, rbf_kind="bessel", cutoff_kind="cosine", cutoff=5.0, list_kind="directed"):
    el = edge_list(list_kind)
    spec = radial_spec(rbf_kind, cutoff_kind, B, cutoff)
    rng = np.random.default_rng([F, B, RBF_NAMES.index(rbf_kind), CUTOFF_NAMES.index(cutoff_kind), int(round(cutoff * 10)), LIST_KINDS.index(list_kind)])
    n = el.n_nodes
    vec, beyond = edge_vectors(el, cutoff, rng)
    c = SimpleNamespace(F=F, B=B, spec=spec, edges=el, n=n, vec=vec, beyond=beyond,
                        s=_f32(rng.standard_normal((n, F))), x=_f32(rng.standard_normal((n, 3, F))), h=_f32(rng.standard_normal((n, 3 * F))),
                        w=_f32(rng.standard_normal((3 * F, B)) / math.sqrt(B)), b=_f32(0.1 * rng.standard_normal(3 * F)),
                        g_s=_f32(rng.standard_normal((n, F))), g_x=_f32(rng.standard_normal((n, 3, F))))
    c.ref = message_eval(c, torch.float64)
    c.ref32 = message_eval(c, torch.float32)
    return c


MESSAGE_OUTPUTS = ("s_out", "x_out", "g_h", "g_x_in", "g_vec")


def message_eval(c, dtype, edge_index=None, vec=None, w=None, b=None, keep_envelope_gradient=True):
    """Forward outputs and autograd's dL/dh, dL/dx, dL/dvec for the cotangents (g_s, g_x) of the case.  The keywords restate the case
    with one thing changed (the power checks of tests/test_painn_kernel_cases_host.py); a changed ``edge_index`` [2, E'] comes with
    its own ``vec`` [E', 3]."""
    t = lambda v: v.detach().to(dtype).clone()
    ei = torch.tensor(c.edges.edge_index) if edge_index is None else edge_index
    h, x, vec = t(c.h).requires_grad_(), t(c.x).requires_grad_(), t(c.vec if vec is None else vec).requires_grad_()
    sp = c.spec
    rbf, fcut, u = radial_ref(vec, sp["rbf_kind"], sp["cutoff_kind"], sp["rbf_params"], sp["cutoff"])
    if not keep_envelope_gradient:
        fcut = fcut.detach()
    out = message_from_basis(t(c.s), x, h, rbf, fcut, u, ei, t(c.w if w is None else w), t(c.b if b is None else b))
    g = torch.autograd.grad(out, [h, x, vec], [t(c.g_s), t(c.g_x)])
    return dict(zip(MESSAGE_OUTPUTS, [o.detach() for o in out] + list(g)))


UPDATE_ROWS_MAX = FEW_ROWS + 1
ZERO_ROW_INSIDE = 5       # a row with x = 0 inside the first tile (when the case has more than 6 rows)


@functools.lru_cache(maxsize=None)
def _update_master(F):
    rng = np.random.default_rng([77, F])
    n = UPDATE_ROWS_MAX
    return SimpleNamespace(s=_f32(rng.standard_normal((n, F))), x=_f32(rng.standard_normal((n, 3, F))), a=_f32(rng.standard_normal((n, 3 * F))),
                           wu=_f32(rng.standard_normal((F, F)) / math.sqrt(F)), wv=_f32(rng.standard_normal((F, F)) / math.sqrt(F)),
                           g_s=_f32(rng.standard_normal((n, F))), g_x=_f32(rng.standard_normal((n, 3, F))), g_cat=_f32(rng.standard_normal((n, 2 * F))))


@functools.lru_cache(maxsize=None)
def update_case(F, n, zero_rows=True):
    """The first ``n`` rows of one master draw per width (a row means the same numbers in every case of that width); rows with x = 0 (an
    atom without neighbours in block 0) at ZERO_ROW_INSIDE and as the last row where the case has room for them."""
    m = _update_master(F)
    c = SimpleNamespace(F=F, n=n, wu=m.wu, wv=m.wv, **{k: getattr(m, k)[:n].clone() for k in ("s", "x", "a", "g_s", "g_x", "g_cat")})
    c.zero_rows = tuple(r for r in ((ZERO_ROW_INSIDE, n - 1) if zero_rows and n > ZERO_ROW_INSIDE + 1 else ()))
    for r in c.zero_rows:
        c.x[r] = 0.0
    c.ref = update_eval(c, torch.float64)
    c.ref32 = update_eval(c, torch.float32)
    return c


UPDATE_OUTPUTS = ("U", "V", "ip", "cat", "s_out", "x_out", "g_a", "g_s_in", "g_x_in")


def update_eval(c, dtype, swap_uv=False, a=None):
    """Forward outputs and autograd's dL/da, dL/ds, dL/dx of <g_s, s'> + <g_x, x'> + <g_cat, [s | |V|]> (``a`` an input)."""
    t = lambda v: v.detach().to(dtype).clone()
    s, x, a = t(c.s).requires_grad_(), t(c.x).requires_grad_(), t(c.a if a is None else a).requires_grad_()
    wu, wv = (t(c.wv), t(c.wu)) if swap_uv else (t(c.wu), t(c.wv))
    U, V, ip, cat = update_uv_ref(s, x, wu, wv)
    s_out, x_out = update_out_ref(s, x, a, U, ip)
    g = torch.autograd.grad([s_out, x_out, cat], [a, s, x], [t(c.g_s), t(c.g_x), t(c.g_cat)])
    return dict(zip(UPDATE_OUTPUTS, [o.detach() for o in (U, V, ip, cat, s_out, x_out)] + list(g)))


def packed_filter(w, b):
    """[KPAD, 3F] = [W^T; b; 0]: what xeq_painn_pack_filter writes."""
    out = torch.zeros((KPAD, w.shape[0]), dtype=w.dtype)
    out[:w.shape[1]] = w.T
    out[w.shape[1]] = b
    return out
