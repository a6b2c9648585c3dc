"""xeq_train_edge alone (csrc/xeq_train_edge.hip; training_ops.EdgeRecordFn / EdgeRecordGrad): values, the first reverse pass and the
second order against the tensor chain of nn/training.py (radial_basis, envelope, spherical_harmonics -> ops.training_records) in f64 and
torch's own double backward through it.

Tolerances.  f64: values to 1e-12 of the largest entry, first and second derivatives to 1e-9 of the largest entry of each output (the
kernel-form vs tensor-form figure of tests/test_gpu_training_ops.py).  f32: the kernel's error against the f64 chain is at most 4 x the
f32 tensor chain's own error against the f64 chain on the same inputs, per output -- both do the same few operations per entry in
another order -- with a floor of 4 ulp of the output's largest entry.
"""
import itertools

import pytest
import torch

from tests.guard_bands import guard_allocations
from xequinet_amd import lib, ops
from xequinet_amd.nn import training
from xequinet_amd.nn import training_ops as to
from xequinet_amd.nn.rbf import resolve_cutoff, resolve_rbf

pytestmark = pytest.mark.gpu
DEV = "cuda"
CUTOFF = 5.0
EDGES = (1, 63, 64, 65, 255, 257)      # wave and workgroup edges
BASES = (1, 3, 20, 21, 32)             # pad widths 3, 1, 0, 3, 0
# at the cutoff, beyond it, a short edge, the three axes (both signs among them)
SPECIAL = [(0.0, CUTOFF, 0.0), (0.0, 0.0, 7.0), (6e-4, -6e-4, 5.2915e-4), (2.0, 0.0, 0.0), (0.0, -3.0, 0.0), (0.0, 0.0, 1.5)]


def _vectors(E, seed, dtype):
    g = torch.Generator().manual_seed(seed)
    d = torch.randn((E, 3), generator=g, dtype=torch.float64)
    vec = d / d.norm(dim=1, keepdim=True) * (0.5 + 5.5 * torch.rand((E, 1), generator=g, dtype=torch.float64))      # a twelfth beyond the cutoff
    n = min(E, len(SPECIAL))
    vec[:n] = torch.tensor(SPECIAL[:n], dtype=torch.float64)
    return vec.to(dtype).to(DEV)


def _modules(rbf_kind, cutoff_kind, B, dtype):
    torch.manual_seed(3)
    rbf = resolve_rbf(rbf_kind, B, CUTOFF)
    if rbf_kind == "gaussian":          # not the initial values: widths of both signs
        with torch.no_grad():
            rbf.std.copy_(0.4 + torch.rand(1, B))
            rbf.std[0, ::2] *= -1
            rbf.mean.add_(0.05 * torch.randn(1, B))
    return rbf.to(dtype).to(DEV).requires_grad_(False), resolve_cutoff(cutoff_kind, CUTOFF)


def _chain(vec, rbf, cut):
    """The tensor form of the records: what nn/training.py::embedding hands to ops.training_records."""
    dist = torch.linalg.norm(vec, dim=-1).unsqueeze(-1)
    env = training.envelope(cut, dist)
    rsh = training.spherical_harmonics(vec, 2)
    return ops.training_records(training.radial_basis(rbf, dist) * env, env, rsh[1], rsh[2])


def _kernel(vec, rbf, cut):
    p0, p1 = (p if p is None else p.detach().reshape(-1).contiguous() for p in rbf.params())
    return to.EdgeRecordFn.apply(vec, p0, p1, (rbf.kind, cut.kind, rbf.num_basis, CUTOFF))[0]


def _three_orders(fn, vec, g, u, rbf, cut):
    """(record, dL/dvec for the cotangent g, d<u, dL/dvec>/dg, d<u, dL/dvec>/dvec)"""
    vec = vec.clone().requires_grad_()
    g = g.clone().requires_grad_()
    rec = fn(vec, rbf, cut)
    (dvec,) = torch.autograd.grad(rec, vec, g, create_graph=True)
    d_g, d_vec = torch.autograd.grad(dvec, [g, vec], u)
    return rec.detach(), dvec.detach(), d_g, d_vec


def _cotangents(E, W, seed, dtype):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn((E, W), generator=g, dtype=torch.float64).to(dtype).to(DEV),
            torch.randn((E, 3), generator=g, dtype=torch.float64).to(dtype).to(DEV))


def _pads(B):
    bp = (B + 3) & ~3
    return list(range(B, bp)) + [bp + 9, bp + 10, bp + 11], bp


NAMES = ("record", "dL/dvec", "d/dg", "d/dvec")


@pytest.mark.parametrize("rbf_kind,cutoff_kind,B", list(itertools.product(("bessel", "gaussian"), ("cosine", "polynomial"), BASES)))
def test_three_orders_match_the_tensor_chain_f64(rbf_kind, cutoff_kind, B):
    dtype = torch.float64
    rbf, cut = _modules(rbf_kind, cutoff_kind, B, dtype)
    W = lib.load().xeq_edge_basis_width(B)
    pads, bp = _pads(B)
    for E in EDGES:
        vec = _vectors(E, 100 + E, dtype)
        g, u = _cotangents(E, W, 200 + E, dtype)
        want = _three_orders(_chain, vec, g, u, rbf, cut)
        with guard_allocations():
            got = _three_orders(_kernel, vec, g, u, rbf, cut)
        for name, a, b, tol in zip(NAMES, got, want, (1e-12, 1e-9, 1e-9, 1e-9)):
            assert a.shape == b.shape and torch.isfinite(a).all(), (name, E)
            err, top = (a - b).abs().max().item(), b.abs().max().item()
            assert err <= tol * top, f"{name}, E={E}: {err:.2e} of {top:.2e}"
        assert (got[0][:, pads] == 0).all() and (got[2][:, pads] == 0).all()        # pad columns and the trailing three: exact zeros
        # at the cutoff and beyond it: the radial part and every derivative of it exactly zero, the harmonics filled
        out = torch.linalg.norm(vec, dim=-1) >= CUTOFF
        assert out[: min(E, 2)].all() and (E < 3 or not out[2:6].any())
        assert (got[0][out][:, : bp + 1] == 0).all() and (got[2][out][:, : bp + 1] == 0).all()
        assert (got[0][out][:, bp + 1 : bp + 9].abs().sum(1) > 1).all()
        g_head = g.clone()
        g_head[:, bp + 1 :] = 0                                                      # a cotangent of the record head alone
        with guard_allocations():
            head = _three_orders(_kernel, vec, g_head, u, rbf, cut)
        assert (head[1][out] == 0).all() and (head[3][out] == 0).all()


def test_reverse_form_with_both_tangents_and_with_either_one():
    """The entry itself: the reverse form at (vec + eps u, g + eps w) is (sum_k g_k Hess rec_k) u + J^T w; either tangent may be null."""
    dtype, B, E = torch.float64, 20, 65
    rbf, cut = _modules("bessel", "cosine", B, dtype)
    meta = (rbf.kind, cut.kind, B, CUTOFF)
    p0 = rbf.freq.detach().reshape(-1).contiguous()
    W = lib.load().xeq_edge_basis_width(B)
    vec = _vectors(E, 7, dtype)
    g, u = _cotangents(E, W, 8, dtype)
    w, _ = _cotangents(E, W, 9, dtype)
    _, _, _, hess_u = _three_orders(_chain, vec, g, u, rbf, cut)
    _, jt_w, _, _ = _three_orders(_chain, vec, w, u, rbf, cut)
    with guard_allocations():
        both = to._edge_call(1, vec, u, g, w, p0, None, meta)
        only_u = to._edge_call(1, vec, u, g, None, p0, None, meta)
        only_w = to._edge_call(1, vec, None, g, w, p0, None, meta)
    for got, want in ((both, hess_u + jt_w), (only_u, hess_u), (only_w, jt_w)):
        assert (got - want).abs().max().item() <= 1e-9 * want.abs().max().item()


@pytest.mark.parametrize("rbf_kind,cutoff_kind", [("bessel", "cosine"), ("gaussian", "polynomial"), ("bessel", "polynomial"), ("gaussian", "cosine")])
def test_gradcheck_and_gradgradcheck(rbf_kind, cutoff_kind):
    """fp64, defaults; edges at least 1e-2 away from the cutoff: the envelope's second derivative jumps there."""
    rbf, cut = _modules(rbf_kind, cutoff_kind, 3, torch.float64)
    lengths = torch.tensor([0.8, 2.3, 4.6, 4.99, 5.01, 6.0], dtype=torch.float64)
    d = torch.randn((6, 3), generator=torch.Generator().manual_seed(4), dtype=torch.float64)
    vec = (d / d.norm(dim=1, keepdim=True) * lengths.unsqueeze(1)).to(DEV).requires_grad_()
    fn = lambda v: _kernel(v, rbf, cut)
    assert torch.autograd.gradcheck(fn, (vec,))
    assert torch.autograd.gradgradcheck(fn, (vec,))


@pytest.mark.parametrize("rbf_kind,cutoff_kind,B", list(itertools.product(("bessel", "gaussian"), ("cosine", "polynomial"), BASES)))
def test_f32_error_stays_within_four_times_the_tensor_chains(rbf_kind, cutoff_kind, B):
    rbf32, cut = _modules(rbf_kind, cutoff_kind, B, torch.float32)
    rbf64 = _modules(rbf_kind, cutoff_kind, B, torch.float32)[0].to(torch.float64)      # the same (f32-representable) parameters
    W = lib.load().xeq_edge_basis_width(B)
    eps32 = torch.finfo(torch.float32).eps
    worst = {}
    for E in EDGES:
        vec = _vectors(E, 100 + E, torch.float32)
        g, u = _cotangents(E, W, 200 + E, torch.float32)
        ref = _three_orders(_chain, vec.double(), g.double(), u.double(), rbf64, cut)
        chain = _three_orders(_chain, vec, g, u, rbf32, cut)
        with guard_allocations():
            kern = _three_orders(_kernel, vec, g, u, rbf32, cut)
        for name, k, c, r in zip(NAMES, kern, chain, ref):
            e_k, e_c = (k.double() - r).abs().max().item(), (c.double() - r).abs().max().item()
            bound = max(4 * e_c, 4 * eps32 * r.abs().max().item())
            worst[name] = max(worst.get(name, 0.0), e_k / bound)
            print(f"f32 {rbf_kind}/{cutoff_kind} B={B} E={E} {name}: kernel {e_k:.3e} chain {e_c:.3e} largest {r.abs().max().item():.3e} "
                  f"kernel/chain {e_k / max(e_c, 1e-300):.2f} kernel/bound {e_k / bound:.2f}")
            assert e_k <= bound, f"{name}, E={E}: kernel {e_k:.3e}, chain {e_c:.3e}, bound {bound:.3e}"
    print(f"f32 {rbf_kind}/{cutoff_kind} B={B}: worst kernel/bound per output {worst}")
