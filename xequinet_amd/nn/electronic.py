"""Charge and spin embeddings -- mirror of ``xequinet/nn/electronic.py:13-90`` (same class names, constructor arguments and
sub-module names, so reference checkpoints load strictly).

Per graph g with total charge / spin t_g and node scalars s (F = node_dim):
  charge: a_g = relu([t_g, -t_g])      spin: a_g = [t_g]      key_in = a_g / max(a_g, 1)
  attn_n = softplus(<linear_q(s_n), linear_k(key_in_g)> / sqrt(F)),  c_n = attn_n linear_v(a_g) / sum_{m in g} attn_m
  s_n <- s_n + residual(c_n)
A module is the identity when its key is absent from the data.  Inference in f32 runs two launches per module
(csrc/xeq_electronic.hip: attention pass, mix pass); a training pass, f64 and widths / activations the kernels do not take run the
reference's op sequence on device tensor operations (differentiable in both orders).  Positions are not read: forces and the virial
do not flow through these modules.
"""
from __future__ import annotations

import math
from typing import Dict

import torch
import torch.nn as nn

from .. import keys, lib
from . import training
from .basic import ResidualLayer

_KINDS = {keys.TOTAL_CHARGE: 0, keys.TOTAL_SPIN: 1}


class _ElectronicEmbedding(nn.Module):
    key: str = ""
    n_in: int = 1

    def __init__(self, node_dim: int = 128, activation: str = "silu") -> None:
        super().__init__()
        self.node_dim = node_dim
        self.scale_factor = 1 / math.sqrt(node_dim)
        self.linear_q = nn.Linear(node_dim, node_dim)
        self.linear_k = nn.Linear(self.n_in, node_dim, bias=False)
        self.linear_v = nn.Linear(self.n_in, node_dim, bias=False)
        self.residual = ResidualLayer(node_dim=node_dim, n_layers=2, activation=activation)

    def inputs(self, total: torch.Tensor) -> torch.Tensor:
        """a_g [G, n_in] of the per-graph totals."""
        raise NotImplementedError

    def reference_form(self, s: torch.Tensor, total: torch.Tensor, batch: torch.Tensor) -> torch.Tensor:
        """The reference's op sequence (nn/electronic.py:30-48 / :71-88) on device tensor operations."""
        a = self.inputs(total.reshape(-1).to(s.dtype))
        key_in = a / torch.maximum(a, torch.ones_like(a))
        batch = batch.long()
        query = self.linear_q(s)
        key = self.linear_k(key_in).index_select(0, batch)
        value = self.linear_v(a).index_select(0, batch)
        attn = nn.functional.softplus(torch.sum(query * key, dim=-1, keepdim=True) * self.scale_factor)
        attn_sum = torch.zeros((a.shape[0], 1), dtype=attn.dtype, device=attn.device).index_add(0, batch, attn).index_select(0, batch)
        return s + self.residual((attn * value) / attn_sum)

    def _kernel_ok(self, s: torch.Tensor, data: Dict[str, torch.Tensor]) -> bool:
        mlp = self.residual.mlp
        return (s.is_cuda and s.dtype == torch.float32 and s.dim() == 2 and s.stride(1) == 1 and s.stride(0) % 4 == 0
                and len(mlp) == 4 and isinstance(mlp[1], nn.SiLU) and isinstance(mlp[3], nn.SiLU)
                and not data.get(training.PARAM_GRADS, False) and bool(lib.load().xeq_electronic_supported(lib.XEQ_F32, self.node_dim)))

    def _kernel_form(self, s: torch.Tensor, total: torch.Tensor, ptr: torch.Tensor) -> torch.Tensor:
        from .fused import _linear_pack

        mlp = self.residual.mlp
        wq = _linear_pack(self.linear_q, self.linear_q.weight, self.linear_q.bias, False)
        w1 = _linear_pack(mlp[0], mlp[0].weight, None, False)
        w2 = _linear_pack(mlp[2], mlp[2].weight, None, False)
        n, F = s.shape
        ptr = ptr if ptr.dtype == torch.int64 and ptr.is_contiguous() else ptr.to(torch.int64).contiguous()
        total = total.reshape(-1)
        total = total if total.dtype == torch.float32 and total.is_contiguous() else total.to(torch.float32).contiguous()
        attn = torch.empty(n, dtype=torch.float32, device=s.device)
        out = torch.empty((n, F), dtype=torch.float32, device=s.device)
        wk, wv = self.linear_k.weight.detach().contiguous(), self.linear_v.weight.detach().contiguous()
        lib.call("xeq_electronic_fwd", _KINDS[self.key], lib.ptr(s), s.stride(0), n, F, lib.ptr(ptr), ptr.numel() - 1, lib.ptr(total),
                 lib.ptr(wq), lib.ptr(wk), lib.ptr(wv), lib.ptr(w1), lib.ptr(w2), lib.ptr(attn), lib.ptr(out), lib.stream())
        return out

    def forward(self, data: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        if self.key not in data:
            return data
        s = data[keys.NODE_INVARIANT]
        total = data[self.key]
        lib.require_hip(s, total)
        ptr = data.get(keys.BATCH_PTR)
        n_graphs = ptr.numel() - 1 if ptr is not None else total.numel()
        if total.numel() != n_graphs:
            raise ValueError(f"{self.key}: {total.numel()} values for {n_graphs} graphs")
        if not training.active(self, data) and self._kernel_ok(s, data):
            if ptr is None:   # graph index without its CSR form: ptr from the per-graph atom counts (sorted batch, as collated)
                counts = torch.bincount(data[keys.BATCH].long(), minlength=n_graphs)
                ptr = torch.cat([counts.new_zeros(1), torch.cumsum(counts, 0)])
            data[keys.NODE_INVARIANT] = self._kernel_form(s, total, ptr)
        else:
            data[keys.NODE_INVARIANT] = self.reference_form(s, total, data[keys.BATCH])
        return data


class ChargeEmbedding(_ElectronicEmbedding):
    """nn/electronic.py:13-50 (positive and negative charges enter through two key / value columns)."""

    key = keys.TOTAL_CHARGE
    n_in = 2

    def inputs(self, total: torch.Tensor) -> torch.Tensor:
        return nn.functional.relu(torch.stack([total, -total], dim=-1))


class SpinEmbedding(_ElectronicEmbedding):
    """nn/electronic.py:53-90 (the spin is non-negative: one column)."""

    key = keys.TOTAL_SPIN
    n_in = 1

    def inputs(self, total: torch.Tensor) -> torch.Tensor:
        return total.unsqueeze(-1)
