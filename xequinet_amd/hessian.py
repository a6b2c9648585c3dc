"""Analytic second derivatives of the XPaiNN energy with respect to the positions: Hessian-vector products and full Hessians.

The reference forms a Hessian with one reverse pass per force component on a model put into training mode (run/geometry.py:59-99,
``calc_analytical_hessian``).  Here the evaluation takes the differentiable form of nn/training.py whatever the model's mode, with the
parameters frozen for its duration (no parameter gradient is formed in any pass), and the passes are batched:

* the Hessian of a batch is block-diagonal over its graphs, so ONE second-order pass whose cotangent has one unit entry per graph gives
  one column of every graph (``column_plan``: ``max_g 3 n_g`` vectors for the whole batch);
* R replicas of the batch (``replicate``) take R vectors per pass: energy and dE/dpos of the replicated batch are formed once with
  ``create_graph=True`` and every pass is one ``autograd.grad`` on the kept graph (``pass_plan``; the last pass may be ragged).

The edge geometry of such an evaluation is one dual-number kernel launch per order (training_ops.EdgeRecordFn, csrc/xeq_train_edge.hip)
when every message block of the model takes ops.DiffMessage; ``training.NATIVE_EDGE = False`` keeps it on the tensor chain.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import torch

from . import keys, lib, ops
from .nn import training

# Atoms of the replicated batch that ``replicas=None`` aims at: R = ATOM_BUDGET // n_atoms, at least 1 and at most the number of vectors.
# A pass on a small batch is bound by its launches, so its time hardly grows with R until the batch fills the GPU; the kept graph grows by
# one batch per replica.  Value: the fastest of the budgets timed by profiles/hessian_timing.py (profiles/hessian_timing.txt).
ATOM_BUDGET = 16384


def column_plan(sizes) -> List[List[Tuple[int, int]]]:
    """Graph sizes n_g -> for every column c < max_g 3 n_g the list of (graph, c) whose graph has that column: column c of graph g is the
    unit displacement of atom c // 3 of the graph along axis c % 3.  Every (graph, column) appears exactly once."""
    n_cols = 3 * max((int(n) for n in sizes), default=0)
    return [[(g, c) for g, n in enumerate(sizes) if c < 3 * int(n)] for c in range(n_cols)]


def pass_plan(n_vectors: int, replicas: int) -> List[Tuple[int, int]]:
    """[first, last) of the vectors each second-order pass takes, ``replicas`` at a time; the last pass may be ragged."""
    if replicas < 1:
        raise ValueError(f"replicas must be at least 1, got {replicas}")
    return [(k, min(k + replicas, n_vectors)) for k in range(0, n_vectors, replicas)]


def default_replicas(n_atoms: int, n_vectors: int) -> int:
    return max(1, min(int(n_vectors), ATOM_BUDGET // max(int(n_atoms), 1)))


def _refuse(model, data) -> None:
    from .nn.model import PaiNN, XPaiNNEwald
    from .nn.output import EnergyOut

    if isinstance(model, (PaiNN, XPaiNNEwald)):
        raise NotImplementedError(f"hessian: {type(model).__name__} is not supported: the reverse kernels of its blocks are "
                                  "once_differentiable, so its force evaluation cannot be differentiated again")
    if not any(isinstance(m, EnergyOut) for m in model.mods.values()):
        raise KeyError(f"a Hessian is the second derivative of {keys.TOTAL_ENERGY!r}: this model has no \"energy\" output head "
                       f"(heads: {[k for k in model.mods if k.startswith('output_')]})")


def _ptr_of(data) -> torch.Tensor:
    n = data[keys.POSITIONS].shape[0]
    if keys.BATCH_PTR in data:
        return data[keys.BATCH_PTR].long()
    if keys.BATCH in data:
        counts = torch.bincount(data[keys.BATCH].long())
        return torch.cat([counts.new_zeros(1), counts.cumsum(0)])
    return torch.tensor([0, n], dtype=torch.long, device=data[keys.POSITIONS].device)


def replicate(data: Dict[str, torch.Tensor], replicas: int) -> Dict[str, torch.Tensor]:
    """R copies of the batch as one batch of R G graphs, built once: positions (a fresh leaf), atomic numbers, ``batch`` / ``ptr``,
    ``edge_index`` offset by r N, ``cell``, ``cell_offsets``, total charge / spin.  The caller's dict and tensors are not touched."""
    R = int(replicas)
    pos = data[keys.POSITIONS]
    N, dev = pos.shape[0], pos.device
    ptr = _ptr_of(data)
    G = ptr.numel() - 1
    out = {keys.POSITIONS: pos.detach().repeat(R, 1), keys.ATOMIC_NUMBERS: data[keys.ATOMIC_NUMBERS].repeat(R)}
    batch = data[keys.BATCH].long() if keys.BATCH in data else torch.repeat_interleave(torch.arange(G, device=dev), ptr[1:] - ptr[:-1])
    rep = torch.arange(R, device=dev)
    out[keys.BATCH] = (batch.unsqueeze(0) + G * rep.unsqueeze(1)).reshape(-1)
    out[keys.BATCH_PTR] = torch.cat([(ptr[:-1].unsqueeze(0) + N * rep.unsqueeze(1)).reshape(-1), ptr.new_tensor([R * N])])
    ei = data[keys.EDGE_INDEX]
    out[keys.EDGE_INDEX] = (ei.unsqueeze(1) + (N * rep).view(1, R, 1).to(ei.dtype)).reshape(2, -1).contiguous()
    if keys.CELL in data:
        out[keys.CELL] = data[keys.CELL].detach().reshape(-1, 3, 3).repeat(R, 1, 1)
        out[keys.CELL_OFFSETS] = data[keys.CELL_OFFSETS].repeat(R, 1)
    for k in (keys.TOTAL_CHARGE, keys.TOTAL_SPIN):
        if k in data:
            out[k] = data[k].reshape(-1).repeat(R)
    return out


def _edge_kernel_applies(model, data) -> bool:
    """Every message block takes ops.DiffMessage and the embedding's basis has the kernel form: then nobody reads the [E, B] tensors."""
    from .nn.basic import edge_graph
    from .nn.training_ops import edge_record_supported
    from .nn.xpainn import XEmbedding, XPainnMessage

    emb = [m for m in model.mods.values() if isinstance(m, XEmbedding)]
    msgs = [m for m in model.mods.values() if isinstance(m, XPainnMessage)]
    if len(emb) != 1 or emb[0].node_irreps.lmax != 2 or not training.NATIVE_MESSAGE:
        return False
    pos = data[keys.POSITIONS]
    if not edge_record_supported(pos, emb[0].rbf.kind, emb[0].cutoff_fn.kind, emb[0].rbf.num_basis):
        return False
    graph = edge_graph(data)
    for m in msgs:
        try:
            cfg = (int(m.rbf_lin.weight.shape[1]), int(m.node_dim), tuple(m.node_irreps.mul3()))
        except NotImplementedError:
            return False
        if not ops.diff_message_supported(pos, graph, cfg):
            return False
    return True


class _Frozen:
    """Every parameter's ``requires_grad`` off for the duration: no pass forms a parameter gradient, whatever the flags say."""

    def __init__(self, model) -> None:
        self.flags = [(p, p.requires_grad) for p in model.parameters()]

    def __enter__(self):
        for p, _ in self.flags:
            p.requires_grad_(False)
        return self

    def __exit__(self, *exc):
        for p, flag in self.flags:
            p.requires_grad_(flag)
        return False


def _gradient(model, data):
    """(dE/dpos with its graph, pos) of the batch in the differentiable form of nn/training.py; E = the sum of the graphs' energies."""
    from .nn.output import EnergyOut, OutputModule

    data[training.TRAIN_PASS] = True
    data[training.PARAM_GRADS] = False
    data[training.EDGE_KERNEL] = _edge_kernel_applies(model, data)
    data = training.edge_data(data, compute_forces=True, compute_virial=False)
    pos = data[keys.POSITIONS]
    for mod in model.mods.values():
        if isinstance(mod, OutputModule) and not isinstance(mod, EnergyOut):
            continue
        data = mod(data)
    energy = data[keys.TOTAL_ENERGY]
    with ops.geometry_only_backward(energy):
        (grad,) = torch.autograd.grad([energy], [pos], grad_outputs=[torch.ones_like(energy)], create_graph=True, allow_unused=True)
    if grad is None or grad.grad_fn is None:     # no edge at all: the energy does not depend on the positions
        return None, pos
    return grad, pos


def hessian_vector_products(model, data: Dict[str, torch.Tensor], vectors: torch.Tensor, *, replicas: Optional[int] = None) -> torch.Tensor:
    """``out[k] = d<dE/dpos, vectors[k]>/dpos`` [K, N, 3] for displacement fields ``vectors`` [K, N, 3] over all atoms of the batch, E the
    sum of the graphs' energies, in the model's units (energy / length^2).  ``data`` is the dict the model takes (after
    ``NeighborTransform``): one graph or a batch, periodic or not, f32 or f64.  ``replicas``: vectors per second-order pass (None: from
    ``ATOM_BUDGET``).  The model's mode, flags and ``.grad`` and the caller's ``data`` are as before afterwards."""
    _refuse(model, data)
    pos = data[keys.POSITIONS]
    N = pos.shape[0]
    if not torch.is_tensor(vectors) or vectors.dim() != 3 or tuple(vectors.shape[1:]) != (N, 3):
        raise ValueError(f"vectors must be a tensor of shape [K, {N}, 3], got {tuple(vectors.shape) if torch.is_tensor(vectors) else type(vectors)}")
    if vectors.dtype != pos.dtype:
        raise ValueError(f"vectors must have the dtype of the positions ({pos.dtype}), got {vectors.dtype}")
    lib.require_hip(pos, data[keys.EDGE_INDEX], vectors)
    K = vectors.shape[0]
    R = default_replicas(N, K) if replicas is None else min(int(replicas), max(K, 1))
    plan = pass_plan(K, R)
    out = torch.zeros((K, N, 3), dtype=pos.dtype, device=pos.device)
    if K == 0 or N == 0 or data[keys.EDGE_INDEX].shape[1] == 0:     # (no edge: the energy does not depend on the positions)
        return out
    with _Frozen(model), torch.enable_grad():
        grad, rpos = _gradient(model, replicate(data, R))
        if grad is None:
            return out
        cot = torch.zeros((R, N, 3), dtype=pos.dtype, device=pos.device)
        for i, (k0, k1) in enumerate(plan):
            if k1 - k0 < R:
                cot.zero_()
            cot[: k1 - k0] = vectors[k0:k1]
            (hv,) = torch.autograd.grad([grad], [rpos], grad_outputs=[cot.view(R * N, 3)], retain_graph=i + 1 < len(plan))
            out[k0:k1] = hv.view(R, N, 3)[: k1 - k0]
    return out


def hessian(model, data: Dict[str, torch.Tensor], *, replicas: Optional[int] = None, symmetrize: bool = False) -> List[torch.Tensor]:
    """One tensor [n_g, n_g, 3, 3] per graph in the reference's layout (run/geometry.py:84-92): ``H[i, k, a, b] = d2E / dpos[i, a] dpos[k, b]``,
    row (i, a) from the pass whose cotangent is the unit displacement of atom i along a -- the raw result, as in the reference;
    ``symmetrize``: (H + H^T) / 2 over the (i, a), (k, b) pairs.  ``hessian_vector_products`` with the unit vectors of ``column_plan``."""
    _refuse(model, data)
    pos = data[keys.POSITIONS]
    lib.require_hip(pos, data[keys.EDGE_INDEX])
    ptr = _ptr_of(data).tolist()
    sizes = [b - a for a, b in zip(ptr[:-1], ptr[1:])]
    plan = column_plan(sizes)
    vectors = torch.zeros((len(plan), pos.shape[0], 3), dtype=pos.dtype, device=pos.device)
    idx = torch.tensor([(c, ptr[g] + c // 3, c % 3) for c, members in enumerate(plan) for g, _ in members], dtype=torch.long).reshape(-1, 3)
    if idx.numel():
        idx = idx.to(pos.device)
        vectors[idx[:, 0], idx[:, 1], idx[:, 2]] = 1
    cols = hessian_vector_products(model, data, vectors, replicas=replicas)
    blocks = []
    for g, n in enumerate(sizes):
        H = cols[: 3 * n, ptr[g] : ptr[g] + n].reshape(n, 3, n, 3).permute(0, 2, 1, 3).contiguous()
        if symmetrize:
            H = 0.5 * (H + H.permute(1, 0, 3, 2))
        blocks.append(H)
    return blocks


class _CallableModule(type(lib)):
    """``xequinet_amd.hessian`` names this module and the function alike: calling the module is calling ``hessian``."""

    def __call__(self, *args, **kwargs):
        return hessian(*args, **kwargs)


import sys as _sys  # noqa: E402

_sys.modules[__name__].__class__ = _CallableModule
