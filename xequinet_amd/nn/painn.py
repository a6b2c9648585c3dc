"""PaiNN embedding / message / update blocks -- host-side mirror of ``xequinet/nn/painn.py`` (same class names, constructor
arguments, sub-module and parameter names and initial values, so the reference's state dicts load; ``forward(data) -> data``).

``data[keys.NODE_EQUIVARIANT]`` is Cartesian ``[N, 3, F]`` in x, y, z order, as in the reference.

Two forms of every block:

* native (f32 on the GPU, SiLU, widths the kernels take, no parameter gradients wanted): the HIP kernels of ``csrc/xeq_painn.hip``
  with explicit reverse passes -- message 2 launches per direction (+ one add in reverse), update 3 per direction; the radial
  basis, envelope, unit vectors, filter and per-edge messages never exist in memory;
* tensor form (f64, CPU tensors, other activations or widths, and every training pass): the block on differentiable tensor
  operations written here, differentiable twice (a force loss differentiates the force evaluation).
"""
from __future__ import annotations

import math
from typing import Dict

import torch
import torch.nn as nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .. import keys, lib
from ..lib import call, ptr, stream
from . import training
from .basic import Int2c1eEmbedding, edge_graph, resolve_activation
from .rbf import resolve_cutoff, resolve_rbf

RADIAL_SPEC = "_xeq_painn_radial_spec"   # (rbf module, cutoff module) of the embedding, read by the message blocks
EDGE_GRAD = "_xeq_painn_edge_grad"       # the evaluation's shared dL/dvec collector (_EdgeGrad)
TENSOR_FORM = "_xeq_painn_tensor_form"   # set by the model: every block of this evaluation takes the tensor form


# ---- tensor form -----------------------------------------------------------------------------------------------------------------
def tensor_radial(rbf: nn.Module, cutoff_fn: nn.Module, vec: torch.Tensor):
    """(rbf [E, B], fcut [E, 1], u [E, 3]) of nn/painn.py:48-53 on differentiable tensor operations."""
    d = torch.linalg.norm(vec, dim=-1, keepdim=True)
    return training.radial_basis(rbf, d), training.envelope(cutoff_fn, d), vec / d


def tensor_message(mod: "PainnMessage", s, x, rbf, fcut, u, edge_index):
    center, nbr = edge_index[keys.CENTER_IDX].long(), edge_index[keys.NEIGHBOR_IDX].long()
    h = mod.scalar_mlp(s)
    filt = mod.rbf_lin(rbf) * fcut
    m_s, g_edge, g_state = torch.split(h.index_select(0, nbr) * filt, mod.node_dim, dim=-1)
    m_v = x.index_select(0, nbr) * g_state.unsqueeze(1) + g_edge.unsqueeze(1) * u.unsqueeze(-1)
    return s.index_add(0, center, m_s), x.index_add(0, center, m_v)


def _norm3(v: torch.Tensor) -> torch.Tensor:
    """|v| over the three components with a zero gradient at v = 0 in EVERY order: torch.linalg.norm's first derivative is 0 there
    too, its second is 0 / 0, which a force loss would meet on every atom without a neighbour."""
    sq = (v * v).sum(1)
    pos = sq > 0
    return torch.where(pos, torch.sqrt(torch.where(pos, sq, torch.ones_like(sq))), torch.zeros_like(sq))


def tensor_update(mod: "PainnUpdate", s, x, want_x: bool = True):
    U, V = mod.update_U(x), mod.update_V(x)
    a = mod.update_mlp(torch.cat([s, _norm3(V)], dim=-1))
    a_ss, a_vv, a_sv = torch.split(a, mod.node_dim, dim=-1)
    return s + a_sv * (U * V).sum(1) + a_ss, (x + a_vv.unsqueeze(1) * U) if want_x else None


def tensor_edge_data(data: Dict[str, torch.Tensor], compute_forces: bool, compute_virial: bool) -> Dict[str, torch.Tensor]:
    """nn/basic.py:60-140 on differentiable tensor operations, on whatever device the positions live."""
    pos = data[keys.POSITIONS]
    ei = data[keys.EDGE_INDEX]
    if keys.BATCH not in data:
        data[keys.BATCH] = torch.zeros(pos.shape[0], dtype=torch.long, device=pos.device)
        data[keys.BATCH_PTR] = torch.tensor([0, pos.shape[0]], dtype=torch.long, device=pos.device)
    batch = data[keys.BATCH].long()
    n_graphs = data[keys.BATCH_PTR].numel() - 1 if keys.BATCH_PTR in data else int(batch.max()) + 1
    cell = data.get(keys.CELL)
    if compute_forces:
        pos.requires_grad_()
    strain = torch.zeros((n_graphs, 3, 3), dtype=pos.dtype, device=pos.device)
    if compute_virial:
        strain.requires_grad_()
        sym = 0.5 * (strain + strain.transpose(1, 2))
        pos = pos + torch.bmm(pos.unsqueeze(1), sym.index_select(0, batch)).squeeze(1)
        if cell is not None:
            cell = cell + torch.bmm(cell, sym)
    center, nbr = ei[keys.CENTER_IDX].long(), ei[keys.NEIGHBOR_IDX].long()
    vec = pos.index_select(0, center) - pos.index_select(0, nbr)
    if cell is not None:
        cell_e = cell.index_select(0, batch.index_select(0, nbr))
        vec = vec - torch.einsum("ni,nij->nj", data[keys.CELL_OFFSETS].to(pos.dtype), cell_e)
    data.update({keys.EDGE_LENGTH: torch.linalg.norm(vec, dim=-1), keys.EDGE_VECTOR: vec, keys.STRAIN: strain})
    return data


def tensor_energy_out(head: nn.Module, data: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """EnergyOut (nn/output.py:114-128) on tensor operations."""
    atom = head.out_mlp(data[keys.NODE_INVARIANT]).reshape(-1)
    if keys.ATOMIC_ENERGIES in data:
        atom = data[keys.ATOMIC_ENERGIES] + atom
    n_graphs = data[keys.BATCH_PTR].numel() - 1
    data[keys.ATOMIC_ENERGIES] = atom
    data[keys.TOTAL_ENERGY] = torch.zeros(n_graphs, dtype=atom.dtype, device=atom.device).index_add(0, data[keys.BATCH].long(), atom)
    return data


def _use_tensor_form(mod: nn.Module, data: Dict[str, torch.Tensor]) -> bool:
    flag = data.get(TENSOR_FORM)
    return training.wants_training_pass(mod) if flag is None else bool(flag)


def native_supported(model_or_block: nn.Module, dtype=torch.float32) -> bool:
    """Every PaiNN block under ``model_or_block`` has the kernel form: f32, SiLU, widths of xeq_painn_supported and of the MLP kernels."""
    L = lib.load()
    for m in model_or_block.modules():
        if isinstance(m, (PainnMessage, PainnUpdate)):
            seq = m.scalar_mlp if isinstance(m, PainnMessage) else m.update_mlp
            nb = m.num_basis if isinstance(m, PainnMessage) else 1
            if not (dtype == torch.float32 and isinstance(seq[1], nn.SiLU) and L.xeq_painn_supported(lib.XEQ_F32, m.node_dim, nb)
                    and L.xeq_mlp2h_supported(lib.XEQ_F32, seq[0].weight.shape[1], seq[0].weight.shape[0], seq[2].weight.shape[0])):
                return False
    return True


# ---- native form -------------------------------------------------------------------------------------------------------------------
class _EdgeGrad:
    """dL/dvec of one evaluation: the message blocks' reverse kernels add into one [E, 3] buffer (every edge has one writer per
    launch) and the block that runs last in the reverse pass hands it to autograd, so the edge-vector op sees one gradient and no
    tensor sums are launched between the blocks.

    Invariant: one reverse pass runs ``registered`` MessageFn.backward calls and the one that runs last is the first block's, whose
    dL/dvec output then carries the whole sum.  PaiNN.run_blocks makes a new collector per evaluation and registers its block
    count; a PainnMessage used outside PaiNN finds no collector in ``data`` and returns its own dL/dvec to autograd."""

    def __init__(self) -> None:
        self.registered = 0
        self.seen = 0
        self.buf = None

    def next(self, vec: torch.Tensor):
        """(buffer, accumulate flag, this is the last block of the reverse pass)"""
        if self.buf is None:
            self.buf = torch.empty_like(vec)
        self.seen += 1
        last = self.seen == self.registered
        out = (self.buf, self.seen > 1, last)
        if last:
            self.buf, self.seen = None, 0
        return out


def _filter_pack(mod: "PainnMessage") -> torch.Tensor:
    w, b = mod.rbf_lin.weight, mod.rbf_lin.bias

    def build():
        out = torch.empty(int(lib.load().xeq_painn_filter_packed_floats(mod.node_dim)), dtype=torch.float32, device=w.device)
        call("xeq_painn_pack_filter", ptr(w.detach().contiguous()), ptr(b.detach().contiguous()), mod.node_dim, mod.num_basis, ptr(out), stream())
        return out

    return lib.cached(mod, "_xeq_filter_pack", (w, b), build)


def _uv_pack(mod: "PainnUpdate") -> torch.Tensor:
    wu, wv = mod.update_U.weight, mod.update_V.weight

    def build():
        out = torch.empty(int(lib.load().xeq_painn_uv_packed_floats(mod.node_dim)), dtype=torch.float32, device=wu.device)
        call("xeq_painn_pack_uv", ptr(wu.detach().contiguous()), ptr(wv.detach().contiguous()), mod.node_dim, ptr(out), stream())
        return out

    return lib.cached(mod, "_xeq_uv_pack", (wu, wv), build)


class MessageFn(Function):
    """nn/painn.py:99-117 with its explicit reverse pass (dL/ds, dL/dx, dL/dvec)."""

    @staticmethod
    def forward(ctx, s, x, vec, mod, graph, rbf, cutoff_fn, collector, x_is_zero):
        from .fused import _mlp_fwd

        s, x, vec = s.contiguous(), x.contiguous(), vec.contiguous()
        n, F = s.shape
        pre, h = _mlp_fwd(mod.scalar_mlp, s)
        wp = _filter_pack(mod)
        p0, p1 = rbf.params()
        cfg = (lib.RBF_KINDS[rbf.kind], lib.CUTOFF_KINDS[cutoff_fn.kind], mod.num_basis, float(cutoff_fn.cutoff), F)
        s_out, x_out = torch.empty_like(s), torch.empty_like(x)
        call("xeq_painn_message_fwd", n, graph.n_edges, ptr(graph.c_rowptr), ptr(graph.c_perm), ptr(graph.edge_index), ptr(vec), ptr(h), ptr(s),
             ptr(x), ptr(wp), ptr(p0.detach()), ptr(None if p1 is None else p1.detach()), *cfg, ptr(s_out), ptr(x_out), stream())
        ctx.save_for_backward(vec, h, x, pre, wp, p0.detach(), None if p1 is None else p1.detach())
        ctx.mod, ctx.graph, ctx.cfg, ctx.collector, ctx.x_is_zero = mod, graph, cfg, collector, x_is_zero
        ctx.set_materialize_grads(False)
        return s_out, x_out

    @staticmethod
    @once_differentiable
    def backward(ctx, g_s, g_x):
        from .fused import _mlp_bwd

        vec, h, x, pre, wp, p0, p1 = ctx.saved_tensors
        graph, n, F = ctx.graph, h.shape[0], ctx.cfg[4]
        if g_s is None:
            g_s = torch.zeros((n, F), dtype=h.dtype, device=h.device)
        g_s = g_s.contiguous()
        g_x = None if g_x is None else g_x.contiguous()
        g_h = torch.empty_like(h)
        want_gx = ctx.needs_input_grad[1] and not ctx.x_is_zero
        g_x_in = torch.empty_like(x) if want_gx else None
        g_vec, accumulate, last = ctx.collector.next(vec) if ctx.collector is not None else (torch.empty_like(vec), False, True)
        call("xeq_painn_message_bwd", n, graph.n_edges, ptr(graph.n_rowptr), ptr(graph.n_perm), ptr(graph.edge_index), ptr(vec), ptr(h), ptr(x),
             ptr(wp), ptr(p0), ptr(p1), *ctx.cfg, ptr(g_s), ptr(g_x), ptr(g_h), ptr(g_x_in), ptr(g_vec), int(accumulate), stream())
        g_s_in = None
        if ctx.needs_input_grad[0]:
            g_mlp = _mlp_bwd(ctx.mod.scalar_mlp, g_h, pre)
            g_s_in = torch.empty_like(g_s)
            call("xeq_painn_add", ptr(g_s), ptr(g_mlp), g_s.numel(), ptr(g_s_in), stream())
        return g_s_in, g_x_in, (g_vec if last and ctx.needs_input_grad[2] else None), None, None, None, None, None, None


class UpdateFn(Function):
    """nn/painn.py:146-164 with its explicit reverse pass.  ``want_x`` False: the vector output is not formed (returned as None)."""

    @staticmethod
    def forward(ctx, s, x, mod, want_x):
        from .fused import _mlp_fwd

        s, x = s.contiguous(), x.contiguous()
        n, F = s.shape
        wp = _uv_pack(mod)
        U, V = torch.empty_like(x), torch.empty_like(x)
        ip = torch.empty_like(s)
        cat = torch.empty((n, 2 * F), dtype=s.dtype, device=s.device)
        call("xeq_painn_update_uv_fwd", n, F, ptr(s), ptr(x), ptr(wp), ptr(U), ptr(V), ptr(ip), ptr(cat), stream())
        pre, a = _mlp_fwd(mod.update_mlp, cat)
        s_out = torch.empty_like(s)
        x_out = torch.empty_like(x) if want_x else None
        call("xeq_painn_update_out_fwd", n, F, ptr(s), ptr(x), ptr(a), ptr(U), ptr(ip), ptr(s_out), ptr(x_out), stream())
        ctx.save_for_backward(a, U, V, ip, cat, pre, wp)
        ctx.mod = mod
        ctx.set_materialize_grads(False)
        return s_out, x_out

    @staticmethod
    @once_differentiable
    def backward(ctx, g_s, g_x):
        from .fused import _mlp_bwd

        a, U, V, ip, cat, pre, wp = ctx.saved_tensors
        n, F = ip.shape
        if g_s is None:
            g_s = torch.zeros_like(ip)
        g_s = g_s.contiguous()
        g_x = None if g_x is None else g_x.contiguous()
        g_a = torch.empty_like(a)
        call("xeq_painn_update_out_bwd", n, F, ptr(g_s), ptr(g_x), ptr(U), ptr(ip), ptr(g_a), stream())
        g_cat = _mlp_bwd(ctx.mod.update_mlp, g_a, pre)
        g_s_in, g_x_in = torch.empty_like(g_s), torch.empty_like(U)
        call("xeq_painn_update_uv_bwd", n, F, ptr(g_s), ptr(g_x), ptr(a), ptr(U), ptr(V), ptr(cat), ptr(g_cat), ptr(wp), ptr(g_s_in), ptr(g_x_in),
             stream())
        return g_s_in, g_x_in, None, None


# ---- modules -----------------------------------------------------------------------------------------------------------------------
class Embedding(nn.Module):
    """nn/painn.py:13-63.  The radial basis, envelope and unit vectors are not written to ``data`` (the message blocks form them per
    edge)."""

    def __init__(
        self,
        node_dim: int = 128,
        num_basis: int = 20,
        embed_basis: str = "one-hot",
        aux_basis: str = "aux56",
        rbf_kernel: str = "bessel",
        cutoff: float = 5.0,
        cutoff_fn: str = "cosine",
    ) -> None:
        super().__init__()
        self.node_dim = node_dim
        if embed_basis == "one-hot":
            self.embedding = nn.Embedding(100, self.node_dim, padding_idx=0)
        else:
            int2c1e = Int2c1eEmbedding(embed_basis, aux_basis)
            self.embedding = nn.Sequential(int2c1e, nn.Linear(int2c1e.embed_dim, self.node_dim))
        self.rbf = resolve_rbf(rbf_kernel, num_basis, cutoff)
        self.cutoff_fn = resolve_cutoff(cutoff_fn, cutoff)

    def _embed_native(self, z: torch.Tensor) -> torch.Tensor:
        from .fused import _linear, _linear_pack

        if isinstance(self.embedding, nn.Embedding):   # a table lookup: no product to run
            return self.embedding.weight.detach().index_select(0, z.long())
        table, lin = self.embedding[0].embed_ten, self.embedding[1]
        pack = _linear_pack(lin, lin.weight, lin.bias, False) if table.dtype == torch.float32 and table.stride(0) % 4 == 0 else None
        if pack is None:
            raise NotImplementedError(f"PaiNN embedding: no kernel for Linear({lin.weight.shape[1]}, {lin.weight.shape[0]})")
        return _linear(table, pack, lin.weight.shape[1], lin.weight.shape[0], lin.bias is not None, row_index=z.to(torch.int32).contiguous())[0]

    def forward(self, data: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        z = data[keys.ATOMIC_NUMBERS]
        vec = data[keys.EDGE_VECTOR]
        data[RADIAL_SPEC] = (self.rbf, self.cutoff_fn)
        if _use_tensor_form(self, data):
            s = self.embedding(z.long())
        else:
            lib.require_hip(vec)
            s = self._embed_native(z)
        data[keys.NODE_INVARIANT] = s
        data[keys.NODE_EQUIVARIANT] = torch.zeros((s.shape[0], 3, self.node_dim), dtype=s.dtype, device=s.device)
        return data


class PainnMessage(nn.Module):
    """Message function for PaiNN (nn/painn.py:66-119)."""

    def __init__(self, node_dim: int = 128, num_basis: int = 20, activation: str = "silu") -> None:
        super().__init__()
        self.node_dim = node_dim
        self.num_basis = num_basis
        self.hidden_dim = self.node_dim * 3
        self.scalar_mlp = nn.Sequential(
            nn.Linear(self.node_dim, self.node_dim),
            resolve_activation(activation),
            nn.Linear(self.node_dim, self.hidden_dim),
        )
        self.rbf_lin = nn.Linear(self.num_basis, self.hidden_dim)

    def forward(self, data: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        s, x = data[keys.NODE_INVARIANT], data[keys.NODE_EQUIVARIANT]
        if RADIAL_SPEC not in data:
            raise KeyError("PainnMessage needs the Embedding of xequinet_amd.nn.painn to run first (radial spec missing)")
        rbf, cutoff_fn = data[RADIAL_SPEC]
        if rbf.num_basis != self.num_basis:
            raise ValueError(f"num_basis mismatch: embedding {rbf.num_basis} vs message {self.num_basis}")
        if _use_tensor_form(self, data):
            basis = data.get("_xeq_painn_basis")
            if basis is None or basis[0] is not data[keys.EDGE_VECTOR]:
                basis = (data[keys.EDGE_VECTOR], *tensor_radial(rbf, cutoff_fn, data[keys.EDGE_VECTOR]))
                data["_xeq_painn_basis"] = basis
            s, x = tensor_message(self, s, x, basis[1], basis[2], basis[3], data[keys.EDGE_INDEX])
        else:
            lib.require_hip(s)
            if not native_supported(self, s.dtype):
                raise NotImplementedError("PainnMessage: no kernel for this width / activation / dtype (the model selects the tensor form)")
            x_is_zero = bool(data.pop("_xeq_painn_x_is_zero", False))
            s, x = MessageFn.apply(s, x, data[keys.EDGE_VECTOR], self, edge_graph(data), rbf, cutoff_fn, data.get(EDGE_GRAD), x_is_zero)
        data[keys.NODE_INVARIANT], data[keys.NODE_EQUIVARIANT] = s, x
        return data


class PainnUpdate(nn.Module):
    """Update function for PaiNN (nn/painn.py:122-166)."""

    def __init__(self, node_dim: int = 128, activation: str = "silu") -> None:
        super().__init__()
        self.node_dim = node_dim
        self.hidden_dim = self.node_dim * 3
        self.update_U = nn.Linear(self.node_dim, self.node_dim, bias=False)
        self.update_V = nn.Linear(self.node_dim, self.node_dim, bias=False)
        self.update_mlp = nn.Sequential(
            nn.Linear(self.node_dim * 2, self.node_dim),
            resolve_activation(activation),
            nn.Linear(self.node_dim, self.hidden_dim),
        )
        # set by the model on its last update block when no head reads the vectors: data[NODE_EQUIVARIANT] is None behind the block
        self.equivariant_output_unused = False

    def forward(self, data: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        s, x = data[keys.NODE_INVARIANT], data[keys.NODE_EQUIVARIANT]
        want_x = not self.equivariant_output_unused
        if _use_tensor_form(self, data):
            s, x = tensor_update(self, s, x, want_x)
        else:
            lib.require_hip(s)
            if not native_supported(self, s.dtype):
                raise NotImplementedError("PainnUpdate: no kernel for this width / activation / dtype (the model selects the tensor form)")
            s, x = UpdateFn.apply(s, x, self, want_x)
        data[keys.NODE_INVARIANT], data[keys.NODE_EQUIVARIANT] = s, x
        return data
