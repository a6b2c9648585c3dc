"""Host side of the Hessian front (xequinet_amd/hessian.py) and of xeq_train_edge's entry: no GPU needed.

Bounds on the oracle's own Hessian: f64 rounding through a few hundred operations per entry, 1e-12 of the largest entry (measured:
H - H^T 2.5e-14 at max |H| 17, translation sum rule 4e-15); entries between different graphs, of a lone atom and of a pair beyond the
cutoff are exact zeros: no operation connects them."""
import copy

import pytest
import torch

from tests import hessian_cases as hc
from xequinet_amd import hessian as hz
from xequinet_amd import lib
from xequinet_amd.nn import resolve_model


@pytest.mark.parametrize("sizes", [[5, 1, 3], [1], [4, 4], [2, 9, 1, 1, 6]])
@pytest.mark.parametrize("replicas", [1, 2, 7, 1000])
def test_column_and_replica_plan(sizes, replicas):
    plan = hz.column_plan(sizes)
    assert len(plan) == 3 * max(sizes)
    seen = [gc for members in plan for gc in members]
    assert sorted(seen) == sorted((g, c) for g, n in enumerate(sizes) for c in range(3 * n))      # every (graph, column) exactly once
    assert len(set(seen)) == len(seen)
    for c, members in enumerate(plan):
        assert all(col == c and c < 3 * sizes[g] for g, col in members)
        assert len({g for g, _ in members}) == len(members)                                        # one unit entry per graph in a vector
    passes = hz.pass_plan(len(plan), replicas)
    assert [k for a, b in passes for k in range(a, b)] == list(range(len(plan)))
    assert all(0 < b - a <= replicas for a, b in passes)
    assert all(b - a == replicas for a, b in passes[:-1])
    if len(plan) % replicas:
        assert passes[-1][1] - passes[-1][0] == len(plan) % replicas                               # the ragged last pass
    if replicas >= len(plan):
        assert passes == [(0, len(plan))]


def test_pass_plan_refuses_no_replica():
    with pytest.raises(ValueError):
        hz.pass_plan(5, 0)


def test_default_replicas_follow_the_atom_budget():
    assert hz.default_replicas(hz.ATOM_BUDGET * 2, 63) == 1
    assert hz.default_replicas(21, 63) == min(63, hz.ATOM_BUDGET // 21)
    assert hz.default_replicas(1, 3) == 3


def test_replicate_offsets_every_index():
    host = hc.host_case("water box")
    rep = hz.replicate(host, 3)
    N, E = host["pos"].shape[0], host["edge_index"].shape[1]
    assert rep["pos"].shape == (3 * N, 3) and rep["edge_index"].shape == (2, 3 * E)
    for r in range(3):
        assert torch.equal(rep["edge_index"][:, r * E : (r + 1) * E], host["edge_index"] + r * N)
        assert torch.equal(rep["pos"][r * N : (r + 1) * N], host["pos"])
        assert torch.equal(rep["cell_offsets"][r * E : (r + 1) * E], host["cell_offsets"])
    assert rep["ptr"].tolist() == [0, N, 2 * N, 3 * N] and rep["batch"].tolist() == [r for r in range(3) for _ in range(N)]
    assert rep["cell"].shape == (3, 3, 3)
    ragged = hc.host_case("ragged")
    rep = hz.replicate(ragged, 2)
    ptr, n = ragged["ptr"], ragged["pos"].shape[0]
    assert rep["ptr"].tolist() == ptr.tolist() + (ptr[1:] + n).tolist()
    assert rep["batch"].tolist() == ragged["batch"].tolist() + (ragged["batch"] + 4).tolist()
    assert "pos" in ragged and ragged["pos"].shape[0] == n and not ragged["pos"].requires_grad


def test_the_oracle_hessian_is_symmetric_translation_invariant_and_block_diagonal():
    host = hc.host_case("ragged")
    full = hc.reference_hessian("well", "ragged")
    N = host["pos"].shape[0]
    top = full.abs().max().item()
    assert top > 1.0
    flat = full.reshape(3 * N, 3 * N)
    assert (flat - flat.t()).abs().max().item() <= 1e-12 * top
    assert full.sum(dim=2).abs().max().item() <= 1e-12 * top                # sum_k H[i, a, k, b] = 0
    batch = host["batch"]
    cross = batch.view(-1, 1) != batch.view(1, -1)
    assert (full.permute(0, 2, 1, 3)[cross] == 0).all()                      # between different graphs: exact zeros
    blocks = hc.blocks_of(full, host["ptr"])
    assert [tuple(b.shape) for b in blocks] == [(n, n, 3, 3) for n in (host["ptr"][1:] - host["ptr"][:-1]).tolist()]
    assert (blocks[1] == 0).all() and (blocks[2] == 0).all()                 # a lone atom, a pair beyond the cutoff
    assert blocks[3].abs().max().item() > 1e-3                               # the bonded pair
    i, k, a, b = 2, 5, 1, 2
    assert blocks[0][i, k, a, b].item() == full[i, a, k, b].item()


def _host_vectors(host, k=2):
    return torch.zeros((k, host["pos"].shape[0], 3), dtype=torch.float64)


def test_refusals():
    host = hc.host_case("ragged")
    model = copy.deepcopy(hc.model_case("well")[0]).double()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hz.hessian(model, dict(host))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hz.hessian_vector_products(model, dict(host), _host_vectors(host))
    for name in ("painn", "xpainn-ewald"):
        other = resolve_model(name, **(dict(use_pbc=False) if name == "xpainn-ewald" else {}))
        with pytest.raises(NotImplementedError, match=type(other).__name__):
            hz.hessian(other, dict(host))
        with pytest.raises(NotImplementedError, match=type(other).__name__):
            hz.hessian_vector_products(other, dict(host), _host_vectors(host))
    headless = resolve_model("xpainn", output_modes=["scalar"], **hc.SMALL)
    with pytest.raises(KeyError, match="energy"):
        hz.hessian(headless, dict(host))
    with pytest.raises(KeyError, match="energy"):
        hz.hessian_vector_products(headless, dict(host), _host_vectors(host))
    N = host["pos"].shape[0]
    for bad in (torch.zeros((2, N + 1, 3), dtype=torch.float64), torch.zeros((N, 3), dtype=torch.float64),
                torch.zeros((2, N, 2), dtype=torch.float64), torch.zeros((2, N, 3), dtype=torch.float32)):      # (the last: the wrong dtype)
        with pytest.raises(ValueError):
            hz.hessian_vector_products(model, dict(host), bad)


def test_the_package_exports_the_front():
    import xequinet_amd

    assert xequinet_amd.hessian_vector_products is hz.hessian_vector_products
    assert callable(xequinet_amd.hessian) and xequinet_amd.hessian.hessian is hz.hessian


def test_train_edge_argument_refusals():
    handle = lib.load()
    one = 1   # any non-null address: nothing is launched

    def call(dtype=0, reverse=0, n=10, vec=one, g=None, rbf=0, cut=0, B=20, cutoff=5.0, p0=one, p1=None, out=one):
        return handle.xeq_train_edge(dtype, reverse, n, vec, None, g, None, rbf, cut, B, cutoff, p0, p1, out, None)

    assert call(dtype=7) == 1 and b"dtype" in handle.xeq_last_error()
    assert call(B=0) == 1 and b"num_basis" in handle.xeq_last_error()
    assert call(B=33) == 1 and b"num_basis" in handle.xeq_last_error()
    assert call(rbf=5) == 1 and b"radial basis" in handle.xeq_last_error()
    assert call(rbf=2) == 1 and b"radial basis" in handle.xeq_last_error()          # the exponential bases have no kernel form
    assert call(cut=2) == 1 and b"cutoff function" in handle.xeq_last_error()
    assert call(vec=None) == 1 and b"vec" in handle.xeq_last_error()
    assert call(rbf=1) == 1 and b"std" in handle.xeq_last_error()                   # the Gaussian basis without p1
    assert call(reverse=1) == 1 and b"reverse form" in handle.xeq_last_error()
    assert call(g=one) == 1 and b"forward form" in handle.xeq_last_error()
    assert call(n=-1) == 1 and call(cutoff=0.0) == 1
    assert call(n=0) == 0 and call(n=0, reverse=1, g=one) == 0                      # no edges: success without a launch


def test_train_edge_supported_table():
    handle = lib.load()
    for dtype in (lib.XEQ_F32, lib.XEQ_F64, 2):
        for rbf, r in lib.RBF_KINDS.items():
            for cut in (0, 1, 2):
                for B in (0, 1, 3, 20, 32, 33):
                    want = dtype in (lib.XEQ_F32, lib.XEQ_F64) and rbf in ("bessel", "gaussian") and cut in (0, 1) and 1 <= B <= 32
                    assert handle.xeq_train_edge_supported(dtype, r, cut, B) == int(want), (dtype, rbf, cut, B)
