"""Ewald message passing -- mirror of ``xequinet/nn/ewald.py``: ``EwaldInitialPBC`` (:60-95), ``EwaldInitialNonPBC`` (:98-138) and
``EwaldBlock`` (:141-212), with the reference's constructor arguments, defaults, sub-module, parameter and buffer names and
initialisation (reference checkpoints load through ``load_reference_state_dict``).

Per graph g with k-vectors kvec[g, k, :], atom n of g at pos_n, theta_nk = <kvec[g, k], pos_n>, damping d_n (1 with periodic
boundaries, prod_i sinc(0.5 delta_k pos_ni + eps) without), h = LayerNorm(pre_residual(s)), kf = down_projection up.weight^T:
  S_R[g, k, f] = sum_{n in g} d_n cos(theta_nk) h[n, f]        S_I the same with sin
  m[n, f] = d_n sum_k kf[k, f] (cos(theta_nk) S_R[g, k, f] + sin(theta_nk) S_I[g, k, f])
  s_n <- s_n + update_layer(m_n)
The modules read data[POSITIONS] and data[CELL], which the edge geometry leaves unstrained (nn/basic.py:99-107 of the reference
strains local copies): their own position and cell dependence enters the forces and not the virial; the strain reaches them through
the trunk's node scalars alone, so the virial of the whole model is not that of the trunk.

Dispatch, as nn/electronic.py and nn/output.py: an f32 inference evaluation on the GPU with SiLU and node_dim a multiple of 32 up to
256 runs the kernel form (csrc/xeq_ewald.hip: structure factor, apply and phase gradient on the exact-f32 matrix instruction, the
eight dense layers on xeq_linear_fwd, row kernels for LayerNorm and the glue; one autograd.Function with an explicit reverse pass
for the node scalars and the positions, no float atomics, a graph's result bit-identical alone and in any batch).  A training pass,
f64, CPU tensors and other widths / activations run the tensor form: the reference's op sequence on differentiable torch
operations, which autograd differentiates twice and which materialises the reference's [n_atoms, K, node_dim] intermediates.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn as nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .. import keys, lib
from . import training
from .basic import ResidualLayer, resolve_activation

# data-dict entry the initial module leaves for the kernel form of the blocks: (kvec, graph stride of kvec, damping [n] or None,
# d damping / d pos [n, 3] or None, ptr [G + 1]); the K_DOT_R / SINC_DAMPING tensors of the tensor form are then not formed
GEOMETRY = "_xeq_ewald_geometry"
KERNEL_MAX_K = 192    # the kernels' cap on the number of k-points (EW_KMAX of csrc/xeq_ewald.hip; xeq_ewald_supported is the authority)


@torch.no_grad()
def get_k_index_product_set(num_k_x: int, num_k_y: int, num_k_z: int) -> torch.Tensor:
    """ewald.py:13-24: the box of k-lattice indices around the origin, cut in half (k and -k carry the same term)."""
    sets = (torch.arange(-num_k_x, num_k_x + 1), torch.arange(-num_k_y, num_k_y + 1), torch.arange(-num_k_z, num_k_z + 1))
    prod = torch.cartesian_prod(*sets)
    prod = prod[prod.shape[0] // 2 + 1 :]
    return prod.to(torch.get_default_dtype())


@torch.no_grad()
def get_k_voxel_grid(k_cutoff: float, delta_k: float, num_k_basis: int, k_offset: Optional[float] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """ewald.py:27-57: the k-lattice sites inside the cutoff sphere and their radial values, a Gaussian basis (nn/rbf.py:113-131 at
    its initial mean / std) times the order-5 polynomial envelope (nn/rbf.py:60-73), evaluated once on the host."""
    num_k = int(k_cutoff / delta_k)
    index_set = get_k_index_product_set(num_k, num_k, num_k)
    k_grid = torch.matmul(index_set, torch.eye(3) * delta_k)
    k_grid = k_grid[torch.square(k_grid).sum(dim=-1) < k_cutoff**2]
    if k_offset is None:
        k_offset = 0.1 if num_k_basis <= 48 else 0.25
    cutoff = k_cutoff + k_offset
    length = torch.linalg.norm(k_grid, dim=-1, keepdim=True)
    mean = torch.linspace(0, cutoff, num_k_basis).view(1, -1)
    std = torch.ones(num_k_basis).view(1, -1).abs() + 1e-5
    rbf = 1 / (std * math.sqrt(2 * math.pi)) * torch.exp(-0.5 * ((length - mean) / std) ** 2)
    p, x = 5, length / cutoff
    poly = 1 - 0.5 * (p + 1) * (p + 2) * torch.pow(x, p) + p * (p + 2) * torch.pow(x, p + 1) - 0.5 * p * (p + 1) * torch.pow(x, p + 2)
    envelope = torch.where(length < cutoff, poly, torch.zeros_like(length))
    return k_grid, rbf * envelope


def _graph_ptr(data: Dict[str, torch.Tensor]) -> torch.Tensor:
    from .output import _graph_ptr as graph_ptr

    return graph_ptr(data)


def _kernel_evaluation(module: nn.Module, data: Dict[str, torch.Tensor]) -> bool:
    """An f32 inference evaluation on the GPU: the only one the kernel form takes."""
    pos = data[keys.POSITIONS]
    return bool(pos.is_cuda and pos.dtype == torch.float32 and not data.get(training.PARAM_GRADS, False) and not training.active(module, data))


class _EwaldInitial(nn.Module):
    # False: the blocks behind this module cannot run the kernel form (width, activation, number of k-points), so the tensors of the
    # tensor form are always written (set by the model; a module used on its own writes the kernel geometry when it can)
    kernel_consumers: bool = True


class EwaldInitialPBC(_EwaldInitial):
    k_index_product_set: torch.Tensor

    def __init__(self, num_k_points: List[int], projection_dim: int = 8) -> None:
        super().__init__()
        assert len(num_k_points) == 3 and any(num_k_points)
        k_index_product_set = get_k_index_product_set(*num_k_points)
        self.register_buffer("k_index_product_set", k_index_product_set)
        self.down_projection = nn.Parameter(torch.empty(k_index_product_set.shape[0], projection_dim))
        nn.init.xavier_uniform_(self.down_projection)

    def forward(self, data: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        pos, cell = data[keys.POSITIONS], data[keys.CELL]
        data[keys.DOWN_PROJECTION] = self.down_projection
        if self.kernel_consumers and _kernel_evaluation(self, data) and bool(
                lib.load().xeq_ewald_supported(lib.XEQ_F32, 32, self.k_index_product_set.shape[0])):
            # 2 pi cell^-1 by the adjugate (rows a, b, c: columns b x c, c x a, a x b over the volume): O(G) tensor operations
            cell = cell.detach().reshape(-1, 3, 3).to(torch.float32)
            a, b, c = cell[:, 0], cell[:, 1], cell[:, 2]
            bc = torch.linalg.cross(b, c)
            inv = torch.stack([bc, torch.linalg.cross(c, a), torch.linalg.cross(a, b)], dim=-1) / (a * bc).sum(-1)[:, None, None]
            kvec = torch.matmul(self.k_index_product_set.to(torch.float32), 2 * math.pi * inv).contiguous()    # [G, K, 3]
            ptr = _graph_ptr(data)
            if kvec.shape[0] != ptr.numel() - 1:
                raise ValueError(f"{keys.CELL}: {kvec.shape[0]} cells for {ptr.numel() - 1} graphs")
            data[GEOMETRY] = (kvec, kvec.shape[1] * 3, None, None, ptr)
            return data
        k_cell = 2 * torch.pi * torch.inverse(cell)
        k_grid = torch.matmul(self.k_index_product_set, k_cell)      # [n_graphs, K, 3] (row convention, ewald.py:80-82)
        k_grid = k_grid.reshape(-1, k_grid.shape[-2], 3).index_select(0, data[keys.BATCH].long())
        data[keys.K_DOT_R] = torch.einsum("aki, ai -> ak", k_grid, pos)
        data[keys.SINC_DAMPING] = torch.tensor(1.0, device=pos.device, dtype=pos.dtype)
        return data


class EwaldInitialNonPBC(_EwaldInitial):
    k_grid: torch.Tensor
    k_rbf_values: torch.Tensor

    def __init__(self, k_cutoff: float, delta_k: float, num_k_basis: int, k_offset: Optional[float] = None, projection_dim: int = 8,
                 eps: float = 1e-5) -> None:
        super().__init__()
        k_grid, k_rbf_values = get_k_voxel_grid(k_cutoff=k_cutoff, delta_k=delta_k, num_k_basis=num_k_basis, k_offset=k_offset)
        self.register_buffer("k_grid", k_grid)
        self.register_buffer("k_rbf_values", k_rbf_values)
        self.delta_k = delta_k
        self.down = nn.Linear(k_rbf_values.shape[-1], projection_dim, bias=False)
        self.eps = eps

    def forward(self, data: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        pos = data[keys.POSITIONS]
        if self.kernel_consumers and _kernel_evaluation(self, data) and bool(lib.load().xeq_ewald_supported(lib.XEQ_F32, 32, self.k_grid.shape[0])):
            # the projection is a function of the parameters alone: one tensor per weight version, so the blocks' filter cache hits
            data[keys.DOWN_PROJECTION] = lib.cached(self, "_xeq_ewald_down", (self.down.weight, self.k_rbf_values),
                                                    lambda: self.down(self.k_rbf_values))
            p = pos.detach().contiguous()
            n = p.shape[0]
            damp = torch.empty(n, dtype=torch.float32, device=p.device)
            ddamp = torch.empty((n, 3), dtype=torch.float32, device=p.device)
            lib.call("xeq_ewald_damping", lib.ptr(p), n, 0.5 * self.delta_k, float(self.eps), lib.ptr(damp), lib.ptr(ddamp), lib.stream())
            data[GEOMETRY] = (self.k_grid.to(torch.float32).contiguous(), 0, damp, ddamp, _graph_ptr(data))
            return data
        data[keys.K_DOT_R] = torch.einsum("ki, ai -> ak", self.k_grid, pos)
        data[keys.SINC_DAMPING] = torch.sinc(0.5 * self.delta_k * pos + self.eps).prod(dim=-1, keepdim=True)
        data[keys.DOWN_PROJECTION] = self.down(self.k_rbf_values)
        return data


# ---- kernel form ---------------------------------------------------------------------------------------------------------------
_INV_SQRT2 = 1 / math.sqrt(2)


def _combine(a: torch.Tensor, sa: float, b: Optional[torch.Tensor], sb: float, pre: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(sa a + sb b) [* silu'(pre)] over contiguous rows, one launch."""
    out = torch.empty_like(a)
    lib.call("xeq_ewald_combine", lib.ptr(a), float(sa), lib.ptr(b), float(sb), lib.ptr(pre), a.numel(), lib.ptr(out), lib.stream())
    return out


def structure_factor(x: torch.Tensor, pos: torch.Tensor, geometry) -> Tuple[torch.Tensor, torch.Tensor]:
    """S_R, S_I [G, K, F] of the rows x [n, F] (xeq_ewald_structure_factor)."""
    kvec, gstride, damp, _, ptr = geometry
    n, F = x.shape
    K, G = kvec.shape[-2], ptr.numel() - 1
    L = lib.load()
    s_r = torch.empty((G, K, F), dtype=torch.float32, device=x.device)
    s_i = torch.empty((G, K, F), dtype=torch.float32, device=x.device)
    parts = torch.empty(int(L.xeq_ewald_parts_floats(n, G, K, F)), dtype=torch.float32, device=x.device)
    lib.call("xeq_ewald_structure_factor", lib.ptr(x), x.stride(0), n, F, lib.ptr(pos), lib.ptr(kvec), gstride, K, lib.ptr(damp), lib.ptr(ptr), G,
             lib.ptr(parts), lib.ptr(s_r), lib.ptr(s_i), lib.stream())
    return s_r, s_i


def apply_filter(s_r: torch.Tensor, s_i: torch.Tensor, kf: torch.Tensor, pos: torch.Tensor, geometry) -> torch.Tensor:
    """m [n, F] from the structure factors and the filter (xeq_ewald_apply)."""
    kvec, gstride, damp, _, ptr = geometry
    G, K, F = s_r.shape
    n = pos.shape[0]
    out = torch.empty((n, F), dtype=torch.float32, device=pos.device)
    lib.call("xeq_ewald_apply", lib.ptr(s_r), lib.ptr(s_i), lib.ptr(kf), n, F, lib.ptr(pos), lib.ptr(kvec), gstride, K, lib.ptr(damp), lib.ptr(ptr), G,
             lib.ptr(out), F, lib.stream())
    return out


def phase_grad(gm, h, s_r, s_i, p_r, p_i, kf, pos, geometry, want_theta: bool = False):
    """(dL/dpos [n, 3], dL/dd [n], dL/dtheta [n, K] or None) (xeq_ewald_phase_grad)."""
    kvec, gstride, damp, ddamp, ptr = geometry
    G, K, F = s_r.shape
    n = pos.shape[0]
    g_pos = torch.empty((n, 3), dtype=torch.float32, device=pos.device)
    g_damp = torch.empty(n, dtype=torch.float32, device=pos.device)
    g_theta = torch.empty((n, K), dtype=torch.float32, device=pos.device) if want_theta else None
    lib.call("xeq_ewald_phase_grad", lib.ptr(gm), gm.stride(0), lib.ptr(h), h.stride(0), lib.ptr(s_r), lib.ptr(s_i), lib.ptr(p_r), lib.ptr(p_i),
             lib.ptr(kf), n, F, lib.ptr(pos), lib.ptr(kvec), gstride, K, lib.ptr(damp), lib.ptr(ddamp), lib.ptr(ptr), G, lib.ptr(g_theta),
             lib.ptr(g_damp), lib.ptr(g_pos), lib.stream())
    return g_pos, g_damp, g_theta


class _EwaldBlockFn(Function):
    """EwaldBlock.forward on the kernels with its explicit reverse pass (gradients for the node scalars and the positions)."""

    @staticmethod
    def forward(ctx, s, pos, block, geometry, kf):
        from .fused import _linear, _linear_pack

        F = block.node_dim
        s = s.contiguous()
        p = pos.detach().contiguous()

        def dense(lin, x):
            return _linear(x, _linear_pack(lin, lin.weight, None, False), F, F, False, act=1, want_pre=True)

        pre_mlp = block.pre_residual.mlp
        u1, p1 = dense(pre_mlp[0], s)
        u2, p2 = dense(pre_mlp[2], u1)
        r = _combine(s, _INV_SQRT2, u2, _INV_SQRT2)
        if isinstance(block.norm, nn.LayerNorm):
            h = torch.empty_like(r)
            stats = torch.empty((r.shape[0], 2), dtype=torch.float32, device=r.device)
            lib.call("xeq_ewald_layernorm_fwd", lib.ptr(r), r.shape[0], F, lib.ptr(block.norm.weight), lib.ptr(block.norm.bias), float(block.norm.eps),
                     lib.ptr(h), lib.ptr(stats), lib.stream())
        else:
            h, stats = r, None
        s_r, s_i = structure_factor(h, p, geometry)
        m = apply_filter(s_r, s_i, kf, p, geometry)
        v, p0 = dense(block.update_layer[0], m)
        pres = []
        for layer in list(block.update_layer)[2:]:
            a, pa = dense(layer.mlp[0], v)
            b, pb = dense(layer.mlp[2], a)
            v = _combine(v, _INV_SQRT2, b, _INV_SQRT2)
            pres += [pa, pb]
        out = _combine(s, 1.0, v, 1.0)
        ctx.block, ctx.geometry, ctx.has_norm = block, geometry, stats is not None
        ctx.save_for_backward(p, kf, p1, p2, r, h, s_r, s_i, p0, *pres, *((stats,) if stats is not None else ()))
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g_out):
        from .fused import _linear, _linear_pack

        block, geometry = ctx.block, ctx.geometry
        F = block.node_dim
        saved = ctx.saved_tensors
        p, kf, p1, p2, r, h, s_r, s_i, p0 = saved[:9]
        stats = saved[-1] if ctx.has_norm else None
        pres = saved[9 : len(saved) - (1 if ctx.has_norm else 0)]
        g_out = g_out.contiguous()

        def dense_t(lin, g):    # g W: the input gradient through the transposed pack of the same weight
            return _linear(g, _linear_pack(lin, lin.weight, None, True), F, F, False)[0]

        gv = g_out
        layers = list(block.update_layer)[2:]
        for j in range(len(layers) - 1, -1, -1):
            pa, pb = pres[2 * j], pres[2 * j + 1]
            g_pb = _combine(gv, _INV_SQRT2, None, 0.0, pb)
            g_pa = _combine(dense_t(layers[j].mlp[2], g_pb), 1.0, None, 0.0, pa)
            gv = _combine(gv, _INV_SQRT2, dense_t(layers[j].mlp[0], g_pa), 1.0)
        gm = dense_t(block.update_layer[0], _combine(gv, 1.0, None, 0.0, p0))
        p_r, p_i = structure_factor(gm, p, geometry)
        g_h = apply_filter(p_r, p_i, kf, p, geometry)          # the operator h -> m is symmetric
        g_pos = None
        if ctx.needs_input_grad[1]:
            g_pos = phase_grad(gm, h, s_r, s_i, p_r, p_i, kf, p, geometry)[0]
        if stats is not None:
            g_r = torch.empty_like(g_h)
            lib.call("xeq_ewald_layernorm_bwd", lib.ptr(g_h), lib.ptr(r), lib.ptr(stats), lib.ptr(block.norm.weight), r.shape[0], F, lib.ptr(g_r),
                     lib.stream())
        else:
            g_r = g_h
        pre_mlp = block.pre_residual.mlp
        g_p2 = _combine(g_r, _INV_SQRT2, None, 0.0, p2)
        g_p1 = _combine(dense_t(pre_mlp[2], g_p2), 1.0, None, 0.0, p1)
        g_s = _combine(_combine(g_out, 1.0, g_r, _INV_SQRT2), 1.0, dense_t(pre_mlp[0], g_p1), 1.0)
        return g_s, g_pos, None, None, None


class EwaldBlock(nn.Module):
    def __init__(self, node_dim: int = 128, projection_dim: int = 8, activation: str = "silu", layer_norm: bool = True,
                 num_residuals: int = 3) -> None:
        super().__init__()
        self.node_dim = node_dim
        self.norm = nn.LayerNorm(node_dim) if layer_norm else nn.Identity()
        act_fn = resolve_activation(activation)
        self.pre_residual = ResidualLayer(node_dim=node_dim, n_layers=2, activation=activation)
        self.up = nn.Linear(projection_dim, node_dim, bias=False)
        with torch.no_grad():    # ewald.py:158-160
            self.up.weight *= 0.01
        self.update_layer = nn.Sequential(nn.Linear(node_dim, node_dim, bias=False), act_fn)
        for _ in range(num_residuals):
            self.update_layer.append(ResidualLayer(node_dim=node_dim, n_layers=2, activation=activation))

    def kernel_shape_ok(self, n_k: Optional[int] = None) -> bool:
        """What the kernel form needs of the module itself: SiLU, node_dim a multiple of 32 up to 256 (and, when given, K)."""
        F = self.node_dim
        return bool(isinstance(self.update_layer[1], nn.SiLU) and F % 32 == 0 and 32 <= F <= 256
                    and (n_k is None or lib.load().xeq_ewald_supported(lib.XEQ_F32, F, n_k)))

    def tensor_form(self, s: torch.Tensor, k_dot_r: torch.Tensor, damping: torch.Tensor, down_projection: torch.Tensor, batch: torch.Tensor,
                    n_graphs: int) -> torch.Tensor:
        """ewald.py:171-212 on differentiable torch operations (CPU tensors too)."""
        batch = batch.long()
        node_res = self.norm(self.pre_residual(s))
        real_part = (torch.cos(k_dot_r) * damping).unsqueeze(-1)
        imag_part = (torch.sin(k_dot_r) * damping).unsqueeze(-1)
        zeros = torch.zeros((n_graphs, k_dot_r.shape[1], s.shape[1]), dtype=s.dtype, device=s.device)
        sf_real = zeros.index_add(0, batch, real_part * node_res.unsqueeze(1))
        sf_imag = zeros.index_add(0, batch, imag_part * node_res.unsqueeze(1))
        kfilter = self.up(down_projection).unsqueeze(0)
        filter_real = torch.index_select(kfilter * sf_real, 0, batch)
        filter_imag = torch.index_select(kfilter * sf_imag, 0, batch)
        message = torch.sum(filter_real * real_part + filter_imag * imag_part, dim=1)
        return s + self.update_layer(message)

    def forward(self, data: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        s = data[keys.NODE_INVARIANT]
        geometry = data.get(GEOMETRY)
        if geometry is not None:
            if not (s.is_cuda and s.dtype == torch.float32 and s.dim() == 2 and self.kernel_shape_ok(geometry[0].shape[-2])):
                raise RuntimeError("EwaldBlock: the initial module left the kernel geometry but this block cannot run the kernel form "
                                   f"(node_dim {self.node_dim}, dtype {s.dtype}); set kernel_consumers = False on the initial module")
            down = data[keys.DOWN_PROJECTION]
            kf = lib.cached(self, "_xeq_ewald_kf", (self.up.weight, down), lambda: torch.mm(down, self.up.weight.t()).contiguous())
            data[keys.NODE_INVARIANT] = _EwaldBlockFn.apply(s, data[keys.POSITIONS], self, geometry, kf)
            return data
        ptr = data.get(keys.BATCH_PTR)
        batch = data[keys.BATCH]
        n_graphs = ptr.numel() - 1 if ptr is not None else (int(batch.max()) + 1 if batch.numel() else 0)
        data[keys.NODE_INVARIANT] = self.tensor_form(s, data[keys.K_DOT_R], data[keys.SINC_DAMPING], data[keys.DOWN_PROJECTION], batch, n_graphs)
        return data
