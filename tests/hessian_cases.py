"""Cases and f64 oracle of the Hessian tests (tests/test_hessian_host.py, tests/test_gpu_hessian.py).

The oracle side is oracle/xpainn_oracle.py's public pieces as a function of the positions -- compute_edge_data, embedding, message,
update, energy_out -- differentiated by torch: the Hessian by ``torch.autograd.functional.hessian``, Hessian-vector products by one
``create_graph`` gradient and one more gradient per vector.  Oracle results are cached per process: they are the slow part (6 s for
the 34-atom batch on the CPU).

Models follow the recipe of tests/test_gpu_training.py::_model (SMALL, two blocks, randomised norm weights and biases) with two sets of
weights: "plain", and "well" -- the construction of tests/test_gpu_fullsize.py::test_qm9_1024_well_conditioned_model_meets_the_plain_
tolerance (the 0e block of every update_V.weight scaled by 0.02, update_V.bias = +-(1 .. 1.5)), which keeps ``Invariant``'s
sqrt(V^2 + eps^2) away from its curvature spike of 1 / eps at V = 0.  The plain weights on synth_qm9_batch(2, seed=5) sit ON that spike
(max |H| 397, f32 error 12 %): that pair is used in no f32 comparison.
"""
import numpy as np
import torch

from oracle import xpainn_oracle as orc
from xequinet_amd.data import synthetic as syn
from xequinet_amd.nn import resolve_model

SMALL = dict(node_dim=128, node_irreps="128x0e + 64x1o + 32x2e", action_blocks=2, hidden_dim=64)
CUTOFF = 5.0


def build_model(weights="well", seed=0, **kw):
    """The f32 host model (the caller casts and moves it); ``weights``: "plain" / "well"."""
    cfg = dict(SMALL, **kw)
    torch.manual_seed(seed)
    model = resolve_model("xpainn", **cfg)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name.endswith(("norm.weight", "affine_weight")):
                p.copy_(1.0 + 0.2 * torch.randn(p.shape, generator=g))
            elif name.endswith(("bias", "affine_bias")):
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
    if weights == "well":
        g = torch.Generator().manual_seed(5)
        sd = model.state_dict()
        for name in sd:
            if name.endswith("update_V.weight"):
                sd[name][: 128 * 128] *= 0.02
            elif name.endswith("update_V.bias"):
                sign = torch.where(torch.rand(128, generator=g) < 0.5, -1.0, 1.0)
                sd[name].copy_((sign * (1.0 + 0.5 * torch.rand(128, generator=g))).to(sd[name]))
        model.load_state_dict(sd)
    else:
        assert weights == "plain"
    return model


def state_dict_f64(model):
    return {k: v.detach().double().cpu().clone() for k, v in model.state_dict().items()}


def host_batch(pos, z, ptr, cell=None, cell_offsets=None, edge_index=None):
    ptr = np.asarray(ptr)
    if edge_index is None:
        edge_index = orc.radius_graph_canonical(pos, ptr, CUTOFF)
    batch = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
    host = {"pos": torch.tensor(pos, dtype=torch.float64), "atomic_numbers": torch.tensor(np.asarray(z).astype(np.int64)),
            "edge_index": torch.tensor(edge_index), "batch": torch.tensor(batch), "ptr": torch.tensor(ptr)}
    if cell is not None:
        host["cell"] = torch.tensor(cell, dtype=torch.float64)
        host["cell_offsets"] = torch.tensor(cell_offsets, dtype=torch.float64)
    return host


def qm9_batch(n_mol, seed):
    return host_batch(*syn.synth_qm9_batch(n_mol, seed=seed))


def ragged_batch():
    """One molecule, a lone atom, a pair beyond the cutoff and a bonded pair: 1 + 1 + 2 + 2 atoms behind the molecule's."""
    pos0, z0, ptr0 = syn.synth_qm9_batch(1, seed=21)
    n = len(pos0)
    pos = np.concatenate([pos0, [[30.0, 0.0, 0.0]], [[60.0, 0.0, 0.0], [60.0, 8.0, 0.0]], [[90.0, 0.0, 0.0], [90.0, 1.1, 0.2]]])
    z = np.concatenate([z0, [8], [1, 6], [6, 8]])
    return host_batch(pos, z, [0, n, n + 1, n + 3, n + 5])


def water_box():
    """24 atoms, 1 286 edges, a box shorter than twice the cutoff: atoms see their own images."""
    pos, z, ptr, cell = syn.synth_water_box(2, seed=3)
    ei, off = orc.radius_graph_pbc_oracle(pos, np.array([len(pos)]), [True, True, True], cell, CUTOFF)
    return host_batch(pos, z, ptr, cell=cell, cell_offsets=off, edge_index=ei)


def to_device(host, dtype, device="cuda"):
    return {k: (v.to(dtype) if v.is_floating_point() else v).to(device) for k, v in host.items()}


def permuted_edges(host, seed=0):
    """The same batch with its edge list in another order."""
    perm = torch.randperm(host["edge_index"].shape[1], generator=torch.Generator().manual_seed(seed))
    out = dict(host)
    out["edge_index"] = host["edge_index"][:, perm].contiguous()
    if "cell_offsets" in host:
        out["cell_offsets"] = host["cell_offsets"][perm].contiguous()
    return out


def oracle_energy_fn(sd, host, dtype=torch.float64, **kw):
    """pos [N, 3] -> the sum of the graphs' energies, on the oracle's pieces in ``dtype``."""
    cfg = dict(SMALL, **kw)
    sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}
    oracle = orc.XPaiNNOracle(sd, **cfg)
    fixed = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in host.items() if k != "pos"}

    def energy(pos):
        data = dict(fixed)
        data["pos"] = pos
        data = orc.compute_edge_data(data, compute_forces=False, compute_virial=False)
        data = oracle.embedding(data)
        for i in range(oracle.blocks):
            data = oracle.message(i, data)
            data = oracle.update(i, data)
        return oracle.energy_out(data)["energy"].sum()

    return energy


def oracle_hessian_full(sd, host, dtype=torch.float64, **kw):
    """[N, 3, N, 3]: H[i, a, k, b] = d2E / dpos[i, a] dpos[k, b]."""
    f = oracle_energy_fn(sd, host, dtype, **kw)
    return torch.autograd.functional.hessian(f, host["pos"].to(dtype).clone()).detach()


def blocks_of(full, ptr):
    """The reference's layout (run/geometry.py:84-92), one [n_g, n_g, 3, 3] per graph: H[i, k, a, b]."""
    ptr = [int(p) for p in ptr]
    return [full[a:b, :, a:b, :].permute(0, 2, 1, 3).contiguous() for a, b in zip(ptr[:-1], ptr[1:])]


def oracle_hvp(sd, host, vectors, **kw):
    """out[k] = d<dE/dpos, vectors[k]>/dpos in f64."""
    f = oracle_energy_fn(sd, host, torch.float64, **kw)
    pos = host["pos"].double().clone().requires_grad_()
    (grad,) = torch.autograd.grad(f(pos), pos, create_graph=True)
    return torch.stack([torch.autograd.grad(grad, pos, grad_outputs=v.double(), retain_graph=True)[0] for v in vectors]).detach()


_CACHE = {}


def cached(key, make):
    """Oracle results by key, once per process; returned tensors are shared and must not be changed."""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


_HOSTS = {"qm9 seed 5": lambda: qm9_batch(2, 5), "qm9 seed 9": lambda: qm9_batch(2, 9), "ragged": ragged_batch, "water box": water_box}


def host_case(name):
    return cached(("host", name), _HOSTS[name])


def model_case(weights):
    """(f32 host model, its f64 state dict) of a set of weights, built once."""
    def make():
        model = build_model(weights)
        return model, state_dict_f64(model)

    return cached(("model", weights), make)


def reference_hessian(weights, batch_name):
    """The f64 oracle Hessian [N, 3, N, 3] of (weights, batch), cached."""
    return cached(("hessian", weights, batch_name), lambda: oracle_hessian_full(model_case(weights)[1], host_case(batch_name)))
