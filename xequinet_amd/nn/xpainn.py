"""XPaiNN embedding / message / update blocks -- host-side mirror of
``xequinet/nn/xpainn.py`` (same class names, constructor signatures, sub-module
and parameter names, ``forward(data) -> data`` contract).

The message block is ONE fused HIP kernel per direction (ops.FusedMessage); the
reference's rbf[E,20], fcut[E,1], rsh[E,480], filter[E,576] and msg[E,480] tensors
never exist.
"""
from __future__ import annotations

from typing import Dict, Iterable, Optional

import torch
import torch.nn as nn

from .. import keys, o3, ops
from .basic import Int2c1eEmbedding, edge_graph, resolve_activation
from . import training
from . import nodeblock
from .fused import EmbeddingLinear, MessageBlock, NodeBlock, UpdateBlock, message_params, update_params
from .o3layer import EquivariantDot, EquivariantLayerNorm, Invariant
from .rbf import resolve_cutoff, resolve_rbf

# private data-dict entry: (rbf module, cutoff module) of the embedding, read by the fused message blocks
RADIAL_SPEC = "_xeq_radial_spec"
# private data-dict entry written by XEmbedding next to its all-zero equivariant features and consumed by the FIRST message block
# behind it: the block then knows xhat is zero on the l > 0 columns and the kernels skip every term with that factor
# (include/xeq.h, XEQ_XHAT_HIGHER_L_ZERO).  A tag on the data, not on a module: whatever else produces the features does not set it
EQUIVARIANT_IS_ZERO = "_xeq_equivariant_is_zero"
# private data-dict entry a caller with static buffers (runtime.GraphedStep*) may set: an all-zero [n_atoms, irreps.dim] tensor nobody
# writes to, used as the start value of the equivariant features instead of a fresh zero fill per evaluation
ZERO_EQUIVARIANT = "_xeq_zero_equivariant"
# private data-dict entry written by an XPainnUpdate that ran the fused node-block launch (csrc/xeq_nodeblock.hip) together with the
# front half of the message block behind it: (s, x, h, xhat) -- the block's outputs and the next block's scalar_mlp output and
# normalised equivariant features (BT layout).  The message block consumes it when (s, x) are the tensors it is handed.
PRESTAGE = "_xeq_message_prestage"
FIRST_FRONT = "_xeq_first_front"     # (s, h, xhat) of the first message block gathered by XEmbedding.forward in one launch
ELEMENT_ROWS = "_xeq_element_rows"   # (atomic numbers, embedding of every table row, the gathered node features): see XEmbedding.forward


class XEmbedding(nn.Module):
    """nn/xpainn.py:14-83.  ``materialize_edge_basis=True`` additionally writes the
    reference's ``radial_basis_function`` / ``envelope_function`` /
    ``spherical_harmonics`` entries (detached); the fused path does not need them."""

    def __init__(
        self,
        node_dim: int = 128,
        node_irreps: Iterable = "128x0e + 64x1o + 32x2e",
        embed_basis: str = "gfn2-xtb",
        aux_basis: str = "aux56",
        num_basis: int = 20,
        rbf_kernel: str = "bessel",
        cutoff: float = 5.0,
        cutoff_fn: str = "cosine",
        materialize_edge_basis: bool = False,
    ) -> None:
        super().__init__()
        self.node_dim = node_dim
        self.node_irreps = o3.Irreps(node_irreps)
        self.node_num_irreps = self.node_irreps.num_irreps
        if embed_basis == "one-hot":
            self.embedding = nn.Embedding(100, self.node_dim, padding_idx=0)
        else:
            int2c1e = Int2c1eEmbedding(embed_basis, aux_basis)
            self.embedding = nn.Sequential(int2c1e, nn.Linear(int2c1e.embed_dim, self.node_dim))
            nn.init.zeros_(self.embedding[1].bias)
        self.sph_harm = o3.SphericalHarmonics(self.node_irreps, normalize=True, normalization="component")
        self.rbf = resolve_rbf(rbf_kernel, num_basis, cutoff)
        self.cutoff_fn = resolve_cutoff(cutoff_fn, cutoff)
        self.materialize_edge_basis = materialize_edge_basis
        # set by the model: [the message block behind the embedding] (a plain list: not a registered sub-module); its norms and scalar_mlp
        # are then gathered from the element table together with the node scalars (nn/fused.py::first_block_front)
        self._next_message = []

    def _embed(self, atomic_numbers: torch.Tensor, param_grads: bool = False) -> torch.Tensor:
        """nn/xpainn.py:62: table rows of the atomic numbers through Linear(embed_dim, node_dim) -- one matrix-core launch that
        gathers the rows itself (csrc/xeq_linear.hip) where the kernel takes the layer, else lookup + library GEMM."""
        if isinstance(self.embedding, nn.Embedding):
            return self.embedding(atomic_numbers.long())
        from .fused import _linear, _linear_pack

        table, lin = self.embedding[0].embed_ten, self.embedding[1]
        if (atomic_numbers.is_cuda and table.dtype == torch.float32 and table.stride(0) % 4 == 0
                and (pack := _linear_pack(lin, lin.weight, lin.bias, False)) is not None):
            z = atomic_numbers.to(torch.int32).contiguous()
            if param_grads:   # training pass: the same launch with the Linear's parameter gradients behind it
                return EmbeddingLinear.apply(z, table, lin, lin.weight, lin.bias)
            return _linear(table, pack, lin.weight.shape[1], lin.weight.shape[0], lin.bias is not None, row_index=z)[0]
        return self.embedding(atomic_numbers)

    def _embedded_rows(self, atomic_numbers: torch.Tensor) -> Optional[torch.Tensor]:
        """Linear(table) for EVERY row of the element table [Z_max + 1, node_dim], cached per weight version, or None where the
        per-node launch is the only form (training pass, nn.Embedding tables, CPU tensors)."""
        if isinstance(self.embedding, nn.Embedding) or not atomic_numbers.is_cuda:
            return None
        from .fused import _linear, _linear_pack

        table, lin = self.embedding[0].embed_ten, self.embedding[1]
        if table.dtype != torch.float32 or table.stride(0) % 4 != 0:
            return None

        def build():   # (None where the kernel does not take the layer: a property of the weight, cached like the rows)
            pack = _linear_pack(lin, lin.weight, lin.bias, False)
            return None if pack is None else _linear(table, pack, lin.weight.shape[1], lin.weight.shape[0], lin.bias is not None)[0]

        return ops.lib.cached(self, "_rows_cache", (lin.weight, lin.bias, table), build)

    def forward(self, data: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        if training.active(self, data):   # parameter gradients / double backward: the differentiable form
            return training.embedding(self, data)
        atomic_numbers = data[keys.ATOMIC_NUMBERS]
        vectors = data[keys.EDGE_VECTOR]
        ops.lib.require_hip(vectors)

        rows = None if data.get(training.PARAM_GRADS, False) else self._embedded_rows(atomic_numbers)
        if rows is not None:
            # Behind the embedding a node's features are a function of its ELEMENT alone (nn/xpainn.py:62, 76-81: s = Linear(table[Z]),
            # x = 0), and so are the norms and scalar_mlp of the first message block: they are evaluated once per table row (cached per
            # weight version) and gathered by atomic number, here and in the first XPainnMessage (nn/fused.py::first_block_front).
            # The kernels give a row the same bits in any batch, so the results are those of the per-node launches.
            z = atomic_numbers if atomic_numbers.dtype in (torch.int32, torch.int64) else atomic_numbers.long()   # (index_select takes either)
            nxt = self._next_message[0] if self._next_message else None
            front = None
            if nxt is not None and nxt.fused and rows.shape[1] == nxt.node_dim and nxt._mul == tuple(self.node_irreps.mul3()):
                from .fused import first_block_front

                # s, h, xhat of the first block in ONE gather launch; the wq kernels never read xhat's l > 0 blocks behind the embedding
                g = data.get(keys.EDGE_GRAPH)
                # ... but the PARAMETER-gradient kernels do (xeq_message_param_grad reads the whole xhat): an eval-mode model whose
                # rbf_lin / radial parameters still require grad gets the zero-filled tail (round-5 advisor, medium: uninitialised
                # memory reached d_w / d_b of message_0.rbf_lin on loss.backward())
                params_want_grad = torch.is_grad_enabled() and (any(p.requires_grad for p in nxt.rbf_lin.parameters())
                                                                or any(p.requires_grad for p in self.rbf.parameters()))
                wq = g is not None and ops.select_message_impl(rows.dtype, g.n_nodes, g.n_edges, nxt.num_basis, nxt.node_dim, nxt._mul) == "wq"
                wants_grad = rows.requires_grad or params_want_grad
                unread = wq and not wants_grad
                # the wq kernels' table form reads the table rows themselves (fused.first_block_table): then only s is gathered per node
                from .fused import first_block_table

                table = first_block_table(nxt, z, rows, wq=wq, training=wants_grad) if nxt.node_dim == nxt._mul[0] else None
                front = first_block_front(nxt, z, rows, z.shape[0], higher_l_unread=unread, table_form=table is not None)
                if front is not None:
                    front = (*front, table)
            if front is not None:
                node_invariant = front[0]
                data[FIRST_FRONT] = front
            else:
                node_invariant = rows.index_select(0, z)
                data[ELEMENT_ROWS] = (z, rows, node_invariant)
        else:
            node_invariant = self._embed(atomic_numbers, bool(data.get(training.PARAM_GRADS, False)))
        data[keys.NODE_INVARIANT] = node_invariant
        data[RADIAL_SPEC] = (self.rbf, self.cutoff_fn)

        if self.materialize_edge_basis:
            distances = data[keys.EDGE_LENGTH].unsqueeze(-1)
            data[keys.RADIAL_BASIS_FUNCTION] = self.rbf(distances)
            data[keys.ENVELOPE_FUNCTION] = self.cutoff_fn(distances)
            with torch.no_grad():  # [x, y, z] -> [y, z, x]  (nn/xpainn.py:71-74)
                data[keys.SPHERICAL_HARMONICS] = self.sph_harm(vectors.detach()[:, [1, 2, 0]])

        node_equivariant = data.pop(ZERO_EQUIVARIANT, None)
        if (node_equivariant is None or node_equivariant.shape != (node_invariant.shape[0], self.node_irreps.dim)
                or node_equivariant.dtype != node_invariant.dtype or node_equivariant.device != node_invariant.device):
            node_equivariant = torch.zeros(
                (node_invariant.shape[0], self.node_irreps.dim), dtype=node_invariant.dtype, device=node_invariant.device
            )
        data[keys.NODE_EQUIVARIANT] = node_equivariant
        data[EQUIVARIANT_IS_ZERO] = True
        front = data.pop(FIRST_FRONT, None)
        if front is not None:   # the first message block finds its norms and scalar_mlp done (the hand-over an update block uses)
            data[PRESTAGE] = (node_invariant, node_equivariant, front[1], front[2], ops.lib.XHAT_HIGHER_L_ZERO, front[3])
        return data


class XPainnMessage(nn.Module):
    """Message function for XPaiNN (nn/xpainn.py:86-161)."""

    def __init__(
        self,
        node_dim: int = 128,
        node_irreps: Iterable = "128x0e + 64x1o + 32x2e",
        num_basis: int = 20,
        activation: str = "silu",
        layer_norm: bool = True,
    ) -> None:
        super().__init__()
        self.node_dim = node_dim
        self.node_irreps = o3.Irreps(node_irreps)
        self.node_num_irreps = self.node_irreps.num_irreps
        self.hidden_dim = self.node_dim + self.node_num_irreps * 2
        self.num_basis = num_basis
        # scalar feature
        self.scalar_mlp = nn.Sequential(
            nn.Linear(self.node_dim, self.node_dim),
            resolve_activation(activation),
            nn.Linear(self.node_dim, self.hidden_dim),
        )
        # spherical feature
        self.rbf_lin = nn.Linear(self.num_basis, self.hidden_dim, bias=True)
        # elementwise tensor product (kept for API parity; fused into the kernel)
        self.rsh_conv = o3.ElementwiseTensorProduct(self.node_irreps, f"{self.node_num_irreps}x0e")
        # normalization
        self.norm = nn.LayerNorm(self.node_dim) if layer_norm else nn.Identity()
        self.o3norm = EquivariantLayerNorm(self.node_irreps) if layer_norm else nn.Identity()
        self._mul = self.node_irreps.mul3()
        self.fused = True  # False: run the reference's op sequence on the operator-level drop-ins

    def forward(self, data: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        x_is_zero = bool(data.pop(EQUIVARIANT_IS_ZERO, False))     # consumed by the first block behind the embedding, whatever its path
        if training.active(self, data):
            return training.message(self, data)
        ori_scalar = data[keys.NODE_INVARIANT]
        ori_equi = data[keys.NODE_EQUIVARIANT]
        if RADIAL_SPEC not in data:
            raise KeyError("XPainnMessage needs the XEmbedding of xequinet_amd to run first (radial spec missing)")
        rbf, cutoff_fn = data[RADIAL_SPEC]
        if rbf.num_basis != self.num_basis:
            raise ValueError(f"num_basis mismatch: embedding {rbf.num_basis} vs message {self.num_basis}")
        pre = data.pop(PRESTAGE, None)
        elem = data.pop(ELEMENT_ROWS, None)
        if (self.fused and pre is None and elem is not None and x_is_zero and elem[2] is ori_scalar and not data.get(training.PARAM_GRADS, False)
                and not ori_scalar.requires_grad and not ori_equi.requires_grad):
            from .fused import first_block_front

            front = first_block_front(self, elem[0], elem[1], ori_scalar.shape[0])
            if front is not None:   # norms and scalar_mlp of the first block from the element table: the message kernel alone is left
                pre = (ori_scalar, ori_equi, front[1], front[2], ops.lib.XHAT_HIGHER_L_ZERO)   # front = (s, h, xhat)
        if self.fused and pre is not None and pre[0] is ori_scalar and pre[1] is ori_equi and not data.get(training.PARAM_GRADS, False):
            # norms and scalar_mlp came out of the update block's launch: the message kernel alone is left (nn/fused.py::NodeBlock)
            p0, p1 = rbf.params()
            cfg = (rbf.kind, cutoff_fn.kind, self.num_basis, float(cutoff_fn.cutoff), self.node_dim, self._mul, 1 | (pre[4] if len(pre) > 4 else 0),
                   *((pre[5],) if len(pre) > 5 and pre[5] is not None else ()))
            new_scalar, new_equi = ops.FusedMessage.apply(pre[2], pre[3], data[keys.EDGE_VECTOR], ori_scalar, ori_equi,
                                                          self.rbf_lin.weight, self.rbf_lin.bias, p0, p1, edge_graph(data), cfg)
        elif self.fused:  # block-level path: explicit forward/reverse, see nn/fused.py
            params = message_params(self, rbf) if data.get(training.PARAM_GRADS, False) else ()
            new_scalar, new_equi = MessageBlock.apply(ori_scalar, ori_equi, data[keys.EDGE_VECTOR], self, edge_graph(data), rbf, cutoff_fn,
                                                      x_is_zero, *params)
        else:           # operator-level path (the reference's own op sequence on the drop-in ops)
            node_scalar = self.norm(ori_scalar)
            node_equi = self.o3norm(ori_equi)
            scalar_out = self.scalar_mlp(node_scalar)
            p0, p1 = rbf.params()
            cfg = (rbf.kind, cutoff_fn.kind, self.num_basis, float(cutoff_fn.cutoff), self.node_dim, self._mul)
            new_scalar, new_equi = ops.FusedMessage.apply(
                scalar_out, node_equi, data[keys.EDGE_VECTOR], ori_scalar, ori_equi,
                self.rbf_lin.weight, self.rbf_lin.bias, p0, p1, edge_graph(data), cfg,
            )
        data[keys.NODE_INVARIANT] = new_scalar
        data[keys.NODE_EQUIVARIANT] = new_equi
        return data


class XPainnUpdate(nn.Module):
    """Update function for XPaiNN (nn/xpainn.py:164-231)."""

    def __init__(
        self,
        node_dim: int = 128,
        node_irreps: Iterable = "128x0e + 64x1o + 32x2e",
        activation: str = "silu",
        layer_norm: bool = True,
    ) -> None:
        super().__init__()
        self.node_dim = node_dim
        self.node_irreps = o3.Irreps(node_irreps)
        self.node_num_irreps = self.node_irreps.num_irreps
        self.hidden_dim = self.node_dim * 2 + self.node_num_irreps
        # spherical feature
        self.update_U = o3.Linear(self.node_irreps, self.node_irreps, biases=True)
        self.update_V = o3.Linear(self.node_irreps, self.node_irreps, biases=True)
        self.invariant = Invariant(self.node_irreps)
        self.equidot = EquivariantDot(self.node_irreps)
        self.dot_lin = nn.Linear(self.node_num_irreps, self.node_dim, bias=False)
        self.rsh_conv = o3.ElementwiseTensorProduct(self.node_irreps, f"{self.node_num_irreps}x0e")
        # scalar feature
        self.update_mlp = nn.Sequential(
            nn.Linear(self.node_dim + self.node_num_irreps, self.node_dim),
            resolve_activation(activation),
            nn.Linear(self.node_dim, self.hidden_dim),
        )
        # normalization
        self.norm = nn.LayerNorm(self.node_dim) if layer_norm else nn.Identity()
        self.o3norm = EquivariantLayerNorm(self.node_irreps) if layer_norm else nn.Identity()
        self.fused = True  # False: run the reference's op sequence on the operator-level drop-ins
        # set by the model on its last update block when no head reads the equivariant features: they are then not computed
        # (data[NODE_EQUIVARIANT] is None behind the block)
        self.equivariant_output_unused = False
        # set by the model: [the message block that follows this update block] (a plain list: not a registered sub-module); its norms
        # and scalar_mlp then run inside this block's launch
        self._next_message = []

    def _node_block_ok(self, data) -> bool:
        """One fused launch per direction for the whole block (nn/fused.py::NodeBlock): f32 on the GPU, the default layout, no
        parameter gradients wanted (the native training pass keeps the kernels that save what the weight gradients read)."""
        s = data[keys.NODE_INVARIANT]
        return (s.is_cuda and s.dtype == torch.float32 and not data.get(training.PARAM_GRADS, False) and nodeblock.supported(self)
                and bool(ops.lib.load().xeq_node_block_auto(s.shape[0])))   # the size rule is the C ABI's (both fronts ask it)

    def forward(self, data: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        if training.active(self, data):
            return training.update(self, data)
        if self.fused and self._node_block_ok(data):
            nxt = self._next_message[0] if self._next_message else None
            if nxt is not None and not (nxt.fused and nodeblock.supported(self, nxt)):
                nxt = None
            out = NodeBlock.apply(data[keys.NODE_INVARIANT], data[keys.NODE_EQUIVARIANT], self, nxt)
            data[keys.NODE_INVARIANT], data[keys.NODE_EQUIVARIANT] = out[0], out[1]
            if nxt is not None:
                data[PRESTAGE] = out
            return data
        if self.fused:
            params = update_params(self) if data.get(training.PARAM_GRADS, False) else ()
            s_new, x_new = UpdateBlock.apply(data[keys.NODE_INVARIANT], data[keys.NODE_EQUIVARIANT], self, *params)
            data[keys.NODE_INVARIANT] = s_new
            data[keys.NODE_EQUIVARIANT] = x_new
            return data
        node_scalar = self.norm(data[keys.NODE_INVARIANT])
        node_equi = self.o3norm(data[keys.NODE_EQUIVARIANT])

        U_equi = self.update_U(node_equi)
        V_equi = self.update_V(node_equi)

        V_scalar = self.invariant(V_equi)
        mlp_in = torch.cat([node_scalar, V_scalar], dim=-1)
        mlp_out = self.update_mlp(mlp_in)

        a_vv, a_sv, a_ss = torch.split(mlp_out, [self.node_num_irreps, self.node_dim, self.node_dim], dim=-1)
        d_equi = self.rsh_conv(U_equi, a_vv)
        inner_prod = self.equidot(U_equi, V_equi)
        inner_prod = self.dot_lin(inner_prod)
        d_scalar = a_sv * inner_prod + a_ss

        ori_scalar = data[keys.NODE_INVARIANT]
        ori_equi = data[keys.NODE_EQUIVARIANT]
        data[keys.NODE_INVARIANT] = ori_scalar + d_scalar
        data[keys.NODE_EQUIVARIANT] = ori_equi + d_equi
        return data
