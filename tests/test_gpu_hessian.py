"""The Hessian front (xequinet_amd/hessian.py) on the GPU against the f64 oracle of tests/hessian_cases.py.

Tolerances.  f64 against the oracle: 1e-8 of the largest entry (two op orders of the same arithmetic: the f64 figure of
tests/test_gpu_training.py).  f64 between replica plans / batch compositions: 1e-10 of the largest entry (library GEMMs may change their
order with the row count).  f32 against the f64 oracle: 8 x the larger of two f32 CPU-oracle evaluations' max errors on the same inputs
(the second with the edge list permuted) -- the bound only has to separate rounding from a wrong term, which shows at 1e-2 max |H|, and
single-sample maxima of f32 evaluations in different orders lie a few x apart.  All three evaluations are compared with the f64 oracle
at the f64 positions, so the rounding of the positions to f32 is common to them.
"""
import copy

import pytest
import torch

from tests import hessian_cases as hc
from xequinet_amd import hessian as hz
from xequinet_amd import keys, lib
from xequinet_amd.nn import training

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _model(weights, dtype):
    return copy.deepcopy(hc.model_case(weights)[0]).to(dtype).to(DEV).eval().requires_grad_(False)


def _assert_blocks(got, full, ptr, tol):
    want = hc.blocks_of(full, ptr)
    top = full.abs().max().item()
    assert len(got) == len(want)
    worst = 0.0
    for g, w in zip(got, want):
        assert tuple(g.shape) == tuple(w.shape) and g.shape[0] == g.shape[1] and tuple(g.shape[2:]) == (3, 3)
        if w.numel():
            worst = max(worst, (g.double().cpu() - w).abs().max().item())
    assert worst <= tol * top, f"{worst:.3e} of {top:.3e}"
    return worst, top


@pytest.fixture
def edge_kernel(request):
    saved = training.NATIVE_EDGE
    training.NATIVE_EDGE = bool(request.param)
    yield bool(request.param)
    training.NATIVE_EDGE = saved


@pytest.mark.parametrize("edge_kernel", [True, False], indirect=True, ids=["edge kernel", "tensor chain"])
@pytest.mark.parametrize("weights,batch", [("well", "qm9 seed 5"), ("well", "qm9 seed 9"), ("plain", "qm9 seed 9")])
def test_f64_hessian_matches_the_oracle(weights, batch, edge_kernel):
    host = hc.host_case(batch)
    full = hc.reference_hessian(weights, batch)
    model = _model(weights, torch.float64)
    first = lib.launch_count()
    got = hz.hessian(model, hc.to_device(host, torch.float64))
    assert ("xeq_train_edge" in lib.launch_names(first)) == edge_kernel
    worst, top = _assert_blocks(got, full, host["ptr"], 1e-8)
    print(f"f64 {weights} / {batch}: max |dH| {worst:.3e} of max |H| {top:.3e}")
    # the reference's layout: H[i, k, a, b] = d2E / dpos[i, a] dpos[k, b] (an entry that its transposes do not equal)
    s, e = int(host["ptr"][1]), int(host["ptr"][2])
    block = full[s:e, :, s:e, :]
    skew = (block - block.transpose(1, 3)).abs()
    i, a, k, b = [int(t) for t in torch.unravel_index(skew.argmax(), skew.shape)]
    assert skew[i, a, k, b].item() > 1e-3 * top
    assert abs(got[1][i, k, a, b].item() - block[i, a, k, b].item()) <= 1e-8 * top


@pytest.mark.parametrize("batch", ["qm9 seed 5", "qm9 seed 9"])
def test_f32_hessian_error_stays_within_eight_times_the_f32_oracles(batch):
    host = hc.host_case(batch)
    sd = hc.model_case("well")[1]
    full = hc.reference_hessian("well", batch)
    top = full.abs().max().item()
    e_oracle = [(hc.oracle_hessian_full(sd, h, torch.float32).double() - full).abs().max().item() for h in (host, hc.permuted_edges(host, 1))]
    got = hz.hessian(_model("well", torch.float32), hc.to_device(host, torch.float32))
    N = host["pos"].shape[0]
    mine = torch.zeros((N, 3, N, 3), dtype=torch.float64)
    ptr = host["ptr"].tolist()
    for g, (a, b) in zip(got, zip(ptr[:-1], ptr[1:])):
        mine[a:b, :, a:b, :] = g.double().cpu().permute(0, 2, 1, 3)
    e_hip = (mine - full).abs().max().item()
    print(f"f32 well / {batch}: HIP error {e_hip:.3e}, f32 oracle errors {e_oracle[0]:.3e} {e_oracle[1]:.3e} (edges permuted), "
          f"ratio {e_hip / max(e_oracle):.2f}, max |H| {top:.3e}")
    assert e_hip <= 8 * max(e_oracle), (e_hip, e_oracle)


def test_the_replica_plan_and_the_batch_composition_do_not_change_the_result():
    host = hc.host_case("qm9 seed 5")
    dev = hc.to_device(host, torch.float64)
    model = _model("well", torch.float64)
    assert 3 * int((host["ptr"][1:] - host["ptr"][:-1]).max()) == 54
    base = hz.hessian(model, dev, replicas=54)
    top = max(b.abs().max().item() for b in base)
    for R in (1, 7):
        other = hz.hessian(model, dev, replicas=R)
        assert max((a - b).abs().max().item() for a, b in zip(base, other)) <= 1e-10 * top, R
    ptr = host["ptr"].tolist()
    for g, (a, b) in enumerate(zip(ptr[:-1], ptr[1:])):
        keep = (host["edge_index"][0] >= a) & (host["edge_index"][0] < b)
        alone = {"pos": host["pos"][a:b], "atomic_numbers": host["atomic_numbers"][a:b], "edge_index": host["edge_index"][:, keep] - a,
                 "batch": torch.zeros(b - a, dtype=torch.long), "ptr": torch.tensor([0, b - a])}
        (single,) = hz.hessian(model, hc.to_device(alone, torch.float64))
        assert (single - base[g]).abs().max().item() <= 1e-10 * top, g
    sym = hz.hessian(model, dev, symmetrize=True)
    for s, raw in zip(sym, base):
        assert torch.equal(s, s.permute(1, 0, 3, 2)) and (s - raw).abs().max().item() <= 1e-10 * top


@pytest.mark.parametrize("dtype", [torch.float64])
def test_ragged_batch(dtype):
    host = hc.host_case("ragged")
    full = hc.reference_hessian("well", "ragged")
    model = _model("well", dtype)
    got = hz.hessian(model, hc.to_device(host, dtype))
    sizes = (host["ptr"][1:] - host["ptr"][:-1]).tolist()
    assert [tuple(b.shape) for b in got] == [(n, n, 3, 3) for n in sizes]
    assert (got[1] == 0).all() and (got[2] == 0).all()          # the lone atom, the pair beyond the cutoff: exact zeros
    worst, top = _assert_blocks(got, full, host["ptr"], 1e-8)
    ptr = host["ptr"].tolist()
    for g, (a, b) in enumerate(zip(ptr[:-1], ptr[1:])):          # no column of one graph shows in another
        keep = (host["edge_index"][0] >= a) & (host["edge_index"][0] < b)
        alone = {"pos": host["pos"][a:b], "atomic_numbers": host["atomic_numbers"][a:b], "edge_index": host["edge_index"][:, keep] - a}
        (single,) = hz.hessian(model, hc.to_device(alone, dtype))
        assert (single - got[g]).abs().max().item() <= 1e-10 * top, g


def test_periodic_hessian_vector_products():
    host = hc.host_case("water box")
    sd = hc.model_case("well")[1]
    N = host["pos"].shape[0]
    vectors = torch.randn((4, N, 3), generator=torch.Generator().manual_seed(11), dtype=torch.float64)
    vectors[3] = 0
    vectors[3, 7, 1] = 1
    want = hc.cached(("hvp", "well", "water box"), lambda: hc.oracle_hvp(sd, host, vectors))
    model = _model("well", torch.float64)
    dev = hc.to_device(host, torch.float64)
    assert dev["edge_index"].shape[1] == 1286 and N == 24
    for R in (None, 3):
        got = hz.hessian_vector_products(model, dev, vectors.to(DEV), replicas=R).cpu()
        assert tuple(got.shape) == (4, N, 3)
        assert (got - want).abs().max().item() <= 1e-8 * want.abs().max().item()
    a, b = (vectors[0] * got[1]).sum().item(), (vectors[1] * got[0]).sum().item()
    assert abs(a - b) <= 1e-9 * max(abs(a), abs(b))


def test_what_ran_for_a_training_model_and_for_a_frozen_one():
    host = hc.host_case("qm9 seed 5")
    dev = hc.to_device(host, torch.float64)
    results = []
    for frozen in (False, True):
        model = _model("well", torch.float64)
        if not frozen:
            model.train().requires_grad_(True)
        first = lib.launch_count()
        H = hz.hessian(model, dev, replicas=7)
        names = lib.launch_names(first)
        passes = len(hz.pass_plan(54, 7))
        assert passes == 8
        assert names.count("xeq_train_edge") == 2 + 2 * passes      # one forward, one reverse, two per second-order pass
        assert not [n for n in names if "wgrad" in n]
        assert all(p.grad is None for p in model.parameters())
        results.append(H)
    top = max(b.abs().max().item() for b in results[0])
    for a, b in zip(*results):      # the same launches; the tensor form's index_add sums in no fixed order, hence not bit for bit
        assert (a - b).abs().max().item() <= 1e-10 * top


@pytest.mark.parametrize("mode", ["train", "eval"])
def test_nothing_is_left_behind(mode):
    host = hc.host_case("qm9 seed 9")
    dev = hc.to_device(host, torch.float32)
    model = _model("well", torch.float32)
    if mode == "train":
        model.train().requires_grad_(True)
        for i, p in enumerate(model.parameters()):      # a mixed set of flags and one gradient that must survive
            p.requires_grad_(i % 3 != 0)
        marked = next(p for p in model.parameters() if p.requires_grad)
        marked.grad = torch.full_like(marked, 0.25)
    flags = [(p.requires_grad, None if p.grad is None else p.grad.clone()) for p in model.parameters()]

    def forces():     # (on tensors of its own: an ordinary evaluation marks the positions it is handed)
        return model({k: v.clone() for k, v in dev.items()}, True, False)[keys.FORCES].detach().clone()

    before = forces()
    snapshot = {k: v.clone() for k, v in dev.items()}
    data = dict(dev)
    hz.hessian(model, data)
    hz.hessian_vector_products(model, data, torch.ones((1, host["pos"].shape[0], 3), dtype=torch.float32, device=DEV))
    assert model.training == (mode == "train")
    for p, (flag, grad) in zip(model.parameters(), flags):
        assert p.requires_grad == flag
        assert (p.grad is None) == (grad is None) and (grad is None or torch.equal(p.grad, grad))
    assert set(data) == set(snapshot) and all(data[k] is dev[k] and torch.equal(data[k], snapshot[k]) for k in snapshot)
    assert not data["pos"].requires_grad and data["pos"].grad is None
    after = forces()
    if mode == "eval":
        assert torch.equal(before, after)
    else:   # the training form scatters dE/dvec to the atoms with index_add, whose order of summation is not fixed: a few f32 ulp
        assert (before - after).abs().max().item() <= 16 * torch.finfo(torch.float32).eps * before.abs().max().item()
