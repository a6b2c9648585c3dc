"""Output heads -- mirror of ``xequinet/nn/output.py``: ``EnergyOut`` (:79-128, the head on the energy+force path),
``ScalarOut`` (:28-76), ``AtomicChargesOut`` (:131-179) and ``PolarOut`` (:245-326), with the reference's class names, constructor
arguments, defaults and sub-module names (reference checkpoints load through ``load_reference_state_dict``).

The three property heads follow the dispatch of nn/electronic.py: inference in f32 runs kernels (the energy head's MLP kernels for
the scalar and charge MLPs, csrc/xeq_heads.hip for PolarOut's node pass and for every per-graph reduction: no atomics, a graph's
result is bit-identical alone, in a batch and in a shard); a training pass, f64 and widths / activations without a kernel run the
reference's op sequence on differentiable device tensor operations.  The kernel form has no reverse pass: in inference only the
energy is differentiated and these heads do not feed it.  ``dipole``, ``spatial`` and ``cartesian`` are not built.
The second set of heads of XPaiNNEwald (``ewald_output_<mode>``, nn/model.py) is built by the same factory."""
from __future__ import annotations

import math
from typing import Dict, Iterable, List, Optional

import torch
import torch.nn as nn

from .. import keys, lib, o3
from ..scatter import scatter_sum
from . import training
from .basic import resolve_activation
from .o3layer import Gate


class OutputModule(nn.Module):
    extra_properties: List[str]

    def __init__(self) -> None:
        super().__init__()

    def forward(self, data: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        raise NotImplementedError


class EnergyOut(OutputModule):
    def __init__(
        self,
        node_dim: int = 128,
        hidden_dim: int = 64,
        activation: str = "silu",
        node_shift: float = 0.0,
        node_scale: float = 1.0,
        **kwargs,
    ) -> None:
        super().__init__()
        self.node_dim = node_dim
        self.hidden_dim = hidden_dim
        final_linear = nn.Linear(self.hidden_dim, 1)
        final_linear.weight.data *= node_scale
        nn.init.constant_(final_linear.bias, node_shift)
        self.out_mlp = nn.Sequential(
            nn.Linear(self.node_dim, self.hidden_dim),
            resolve_activation(activation),
            final_linear,
        )
        self.extra_properties = [keys.TOTAL_ENERGY, keys.ATOMIC_ENERGIES]

    def forward(self, data: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        if training.active(self, data):
            return training.energy_out(self, data)
        batch = data[keys.BATCH]
        node_scalar = data[keys.NODE_INVARIANT]
        from .fused import EnergyHead, EnergyReadout

        ptr_ = data.get(keys.BATCH_PTR)
        if (ptr_ is not None and keys.ATOMIC_ENERGIES not in data and not data.get(training.PARAM_GRADS, False)
                and EnergyReadout.supported(self.out_mlp, node_scalar)):
            # the head, the per-graph sum and (saved as one row per node) the head's whole reverse pass: two launches (nn/fused.py)
            atomic_energies, total_energy = EnergyReadout.apply(node_scalar, self.out_mlp, batch.to(torch.int64).contiguous(), ptr_)
            data[keys.ATOMIC_ENERGIES] = atomic_energies
            data[keys.TOTAL_ENERGY] = total_energy
            return data
        if EnergyHead.supported(self.out_mlp, node_scalar):    # matrix-core kernels, explicit reverse pass (nn/fused.py)
            params = EnergyHead.params(self.out_mlp) if data.get(training.PARAM_GRADS, False) else ()
            atom_eng_out = EnergyHead.apply(node_scalar, self.out_mlp, *params)
        else:                                                  # f64, other activations / widths: library GEMMs
            atom_eng_out = self.out_mlp(node_scalar).reshape(-1)
        if keys.ATOMIC_ENERGIES in data:
            atomic_energies = data[keys.ATOMIC_ENERGIES] + atom_eng_out
        else:
            atomic_energies = atom_eng_out
        total_energy = scatter_sum(atomic_energies, batch, dim=0, ptr=data.get(keys.BATCH_PTR))
        data[keys.ATOMIC_ENERGIES] = atomic_energies
        data[keys.TOTAL_ENERGY] = total_energy
        return data


def _graph_ptr(data: Dict[str, torch.Tensor]) -> torch.Tensor:
    """ptr [G + 1] (int64, contiguous) of the batch; from the sorted graph index when the batch came without its CSR form."""
    ptr = data.get(keys.BATCH_PTR)
    if ptr is None:
        batch = data[keys.BATCH].long()
        counts = torch.bincount(batch, minlength=int(batch.max()) + 1 if batch.numel() else 0)
        ptr = torch.cat([counts.new_zeros(1), torch.cumsum(counts, 0)])
    return ptr if ptr.dtype == torch.int64 and ptr.is_contiguous() else ptr.to(torch.int64).contiguous()


def _graph_sum(src: torch.Tensor, data: Dict[str, torch.Tensor]) -> torch.Tensor:
    """Per-graph sum of node rows in the tensor form (differentiable)."""
    return scatter_sum(src, data[keys.BATCH], dim=0, ptr=_graph_ptr(data))


def _head_rows_ok(seq: nn.Sequential, s: torch.Tensor, data: Dict[str, torch.Tensor]) -> bool:
    from .fused import EnergyHead, EnergyReadout

    return (s.dim() == 2 and s.is_cuda and s.dtype == torch.float32 and not data.get(training.PARAM_GRADS, False)
            and (EnergyReadout.supported(seq, s) or EnergyHead.supported(seq, s)))


def _head_rows(seq: nn.Sequential, s: torch.Tensor) -> torch.Tensor:
    """Linear - SiLU - Linear(., 1) per node on the energy head's kernels, [n]; no reverse pass is kept."""
    from .fused import EnergyHead, EnergyReadout, _linear_pack

    s = s.detach()
    if EnergyReadout.supported(seq, s) and s.stride(1) == 1 and s.stride(0) % 4 == 0:    # xeq_head_fwd: one launch
        lin1, lin2 = seq[0], seq[2]
        n, F = s.shape
        out = torch.empty(n, dtype=torch.float32, device=s.device)
        w2 = lin2.weight.detach().reshape(-1).contiguous()
        lib.call("xeq_head_fwd", lib.ptr(s), s.stride(0), n, F, lin1.weight.shape[0], lib.ptr(_linear_pack(lin1, lin1.weight, lin1.bias, False)),
                 None, lib.ptr(w2), lib.ptr(lin2.bias), lib.ptr(out), None, lib.stream())
        return out
    with torch.no_grad():
        return EnergyHead.apply(s, seq)                                                  # xeq_linear_fwd + xeq_head_dot


def _reduce(mode: int, src: torch.Tensor, width: int, ptr: torch.Tensor, total=None, out=None, iso=None) -> None:
    lib.call("xeq_head_graph_reduce", mode, lib.ptr(src), src.stride(0), width, lib.ptr(ptr), ptr.numel() - 1, lib.ptr(total), lib.ptr(out),
             lib.ptr(iso), lib.stream())


class ScalarOut(OutputModule):
    """nn/output.py:28-76: r_n = out_mlp(s_n), reduced per graph by ``reduce_op`` ("sum", "mean" or None)."""

    def __init__(
        self,
        node_dim: int = 128,
        hidden_dim: int = 64,
        activation: str = "silu",
        node_shift: float = 0.0,
        node_scale: float = 1.0,
        reduce_op: Optional[str] = "sum",
        output_field: str = keys.SCALAR_OUTPUT,
        **kwargs,
    ) -> None:
        super().__init__()
        if reduce_op not in ("sum", "mean", None):
            raise NotImplementedError(f"ScalarOut: reduce_op {reduce_op!r} (sum, mean or None)")
        self.node_dim = node_dim
        self.hidden_dim = hidden_dim
        final_linear = nn.Linear(self.hidden_dim, 1)
        final_linear.weight.data *= node_scale
        nn.init.constant_(final_linear.bias, node_shift)
        self.out_mlp = nn.Sequential(
            nn.Linear(self.node_dim, self.hidden_dim),
            resolve_activation(activation),
            final_linear,
        )
        self.reduce_op = reduce_op
        self.output_field = output_field
        self.extra_properties = [output_field]

    def forward(self, data: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        s = data[keys.NODE_INVARIANT]
        lib.require_hip(s)
        if not training.active(self, data) and _head_rows_ok(self.out_mlp, s, data):
            res = _head_rows(self.out_mlp, s)
            if self.reduce_op is not None:
                ptr = _graph_ptr(data)
                rows, res = res, torch.empty(ptr.numel() - 1, dtype=torch.float32, device=s.device)
                _reduce(0 if self.reduce_op == "sum" else 1, rows, 1, ptr, out=res)
        else:
            res = training._mlp(self.out_mlp, s).reshape(-1)
            if self.reduce_op is not None:
                res = _graph_sum(res, data)
                if self.reduce_op == "mean":
                    ptr = _graph_ptr(data)
                    res = res / (ptr[1:] - ptr[:-1]).clamp_min(1).to(res.dtype)
        data[self.output_field] = res
        return data


class AtomicChargesOut(OutputModule):
    """nn/output.py:131-179: q_n = out_mlp(s_n); with ``conservation`` every graph's charges are shifted by the same amount so that
    they add up to data["charge"] (zero when absent)."""

    def __init__(
        self,
        node_dim: int = 128,
        hidden_dim: int = 64,
        activation: str = "silu",
        conservation: bool = True,
        **kwargs,
    ) -> None:
        super().__init__()
        self.node_dim = node_dim
        self.hidden_dim = hidden_dim
        self.out_mlp = nn.Sequential(
            nn.Linear(self.node_dim, self.hidden_dim),
            resolve_activation(activation),
            nn.Linear(self.hidden_dim, 1),
        )
        nn.init.zeros_(self.out_mlp[0].bias)
        nn.init.zeros_(self.out_mlp[2].bias)
        self.conservation = conservation
        self.extra_properties = [keys.ATOMIC_CHARGES]

    def forward(self, data: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        s = data[keys.NODE_INVARIANT]
        total = data.get(keys.TOTAL_CHARGE)
        lib.require_hip(s, total)
        if not training.active(self, data) and _head_rows_ok(self.out_mlp, s, data):
            q = _head_rows(self.out_mlp, s)
            if self.conservation:
                ptr = _graph_ptr(data)
                if total is not None:
                    total = total.reshape(-1)
                    if total.numel() != ptr.numel() - 1:
                        raise ValueError(f"{keys.TOTAL_CHARGE}: {total.numel()} values for {ptr.numel() - 1} graphs")
                    total = total if total.dtype == torch.float32 and total.is_contiguous() else total.to(torch.float32).contiguous()
                _reduce(3, q, 1, ptr, total=total)
        else:
            q = training._mlp(self.out_mlp, s).reshape(-1)
            if self.conservation:
                ptr = _graph_ptr(data)
                raw = _graph_sum(q, data)
                target = total.reshape(-1).to(q.dtype) if total is not None else torch.zeros_like(raw)
                delta = (target - raw) / (ptr[1:] - ptr[:-1]).clamp_min(1).to(q.dtype)
                q = q + delta.index_select(0, data[keys.BATCH].long())
        data[keys.ATOMIC_CHARGES] = q
        return data


class PolarOut(OutputModule):
    """nn/output.py:245-326: the polarizability tensor from the node scalars and the 0e / 2e blocks of the equivariant features."""

    reads_equivariant = True

    def __init__(
        self,
        node_dim: int = 128,
        node_irreps: Iterable = "128x0e + 64x1o + 32x2e",
        hidden_dim: int = 64,
        hidden_irreps: Iterable = "64x0e + 16x2e",
        activation: str = "silu",
        isotropic: bool = False,
        **kwargs,
    ) -> None:
        super().__init__()
        self.node_dim = node_dim
        self.node_irreps = o3.Irreps(node_irreps)
        self.hidden_dim = hidden_dim
        self.hidden_irreps = o3.Irreps(hidden_irreps)
        self.scalar_out_mlp = nn.Sequential(
            nn.Linear(self.node_dim, self.hidden_dim),
            resolve_activation(activation),
            nn.Linear(self.hidden_dim, 2),
        )
        nn.init.zeros_(self.scalar_out_mlp[0].bias)
        nn.init.zeros_(self.scalar_out_mlp[2].bias)
        self.equi_out_mlp = nn.Sequential(
            o3.Linear(self.node_irreps, self.hidden_irreps, biases=True),
            Gate(self.hidden_irreps, activation=activation),
            o3.Linear(self.hidden_irreps, "1x0e + 1x2e", biases=True),
        )
        self.isotropic = isotropic
        self.extra_properties = [keys.POLARIZABILITY if not isotropic else keys.ISO_POLARIZABILITY]

    def _widths(self):
        """(mul0, mul2, offset of the 2e block, hid0, hid2) when both irreps are (0e, ..., 2e) with the kernel's block order, else None."""
        def pick(irreps):
            found = {}
            for mul, l, off, _ in irreps.blocks():
                found[l] = (mul, off)
            return found

        if any(ir.p != (1 if ir.l % 2 == 0 else -1) for irreps in (self.node_irreps, self.hidden_irreps) for _, ir in irreps):
            return None
        ni, hi = pick(self.node_irreps), pick(self.hidden_irreps)
        if len(ni) != len(self.node_irreps) or set(hi) != {0, 2} or len(self.hidden_irreps) != 2 or 0 not in ni or 2 not in ni:
            return None
        if ni[0][1] != 0 or hi[0][1] != 0:
            return None
        return ni[0][0], ni[2][0], ni[2][1], hi[0][0], hi[2][0]

    def _kernel_ok(self, s: torch.Tensor, x: torch.Tensor, data: Dict[str, torch.Tensor]) -> bool:
        w = self._widths()
        return (w is not None and s.is_cuda and s.dtype == torch.float32 and x.dtype == torch.float32 and s.dim() == 2 and x.dim() == 2
                and s.stride(1) == 1 and s.stride(0) % 4 == 0 and x.stride(1) == 1 and x.stride(0) % 4 == 0 and w[2] % 4 == 0
                and s.data_ptr() % 16 == 0 and x.data_ptr() % 16 == 0
                and isinstance(self.scalar_out_mlp[1], nn.SiLU) and isinstance(self.equi_out_mlp[1].activation, nn.Sigmoid)
                and not data.get(training.PARAM_GRADS, False)
                and bool(lib.load().xeq_head_polar_supported(lib.XEQ_F32, self.node_dim, w[0], w[1], self.hidden_dim, w[3], w[4])))

    def _packs(self):
        """The three packed hidden weights (output columns padded to a multiple of 32 by zero rows, 1 / sqrt(mul_in) folded into the
        o3 blocks), through the per-front pack cache."""
        lin_s, lin_e = self.scalar_out_mlp[0], self.equi_out_mlp[0]
        mul0, mul2, _, hid0, hid2 = self._widths()

        def pack(w, bias):
            n_out, k_in = w.shape
            n_pad = (n_out + 31) // 32 * 32
            wp = torch.zeros((n_pad, k_in), dtype=torch.float32, device=w.device)
            wp[:n_out] = w
            bp = None
            if bias is not None:
                bp = torch.zeros(n_pad, dtype=torch.float32, device=w.device)
                bp[:n_out] = bias
            out = torch.empty(lib.load().xeq_mlp_packed_floats(n_pad, k_in), dtype=torch.float32, device=w.device)
            lib.call("xeq_mlp_pack", lib.ptr(wp), lib.ptr(bp), n_pad, k_in, 0, lib.ptr(out), lib.stream())
            return out

        def build():
            w = lin_e.weight.detach()
            w0 = w[: mul0 * hid0].view(mul0, hid0).t() * (1.0 / math.sqrt(mul0))
            w2 = w[mul0 * hid0 : mul0 * hid0 + mul2 * hid2].view(mul2, hid2).t() * (1.0 / math.sqrt(mul2))
            b0 = lin_e.bias.detach() if lin_e.bias.numel() > 0 else None
            return pack(lin_s.weight.detach(), lin_s.bias.detach()), pack(w0, b0), pack(w2, None)

        return lib.cached(self, "_xeq_polar_pack", (lin_s.weight, lin_s.bias, lin_e.weight, lin_e.bias), build)

    def _kernel_form(self, s: torch.Tensor, x: torch.Tensor, data: Dict[str, torch.Tensor]):
        mul0, mul2, off2, hid0, hid2 = self._widths()
        s, x = s.detach(), x.detach()
        ws1, w0, w2 = self._packs()
        lin_s2, lin_e2 = self.scalar_out_mlp[2], self.equi_out_mlp[2]
        n = s.shape[0]
        ptr = _graph_ptr(data)
        G = ptr.numel() - 1
        f32 = dict(dtype=torch.float32, device=s.device)
        t = torch.empty((n, 8), **f32)
        ws2 = lin_s2.weight.detach().contiguous()
        wb = lin_e2.weight.detach().contiguous()
        lib.call("xeq_head_polar_nodes", lib.ptr(s), s.stride(0), lib.ptr(x), x.stride(0), n, self.node_dim, mul0, mul2, off2, self.hidden_dim,
                 hid0, hid2, lib.ptr(ws1), lib.ptr(w0), lib.ptr(w2), lib.ptr(ws2), lib.ptr(lin_s2.bias), lib.ptr(wb), lib.ptr(lin_e2.bias),
                 float(self.equi_out_mlp[1].invariant.eps), lib.ptr(t), lib.stream())
        alpha = torch.empty((G, 3, 3), **f32)
        iso = torch.empty(G, **f32) if self.isotropic else None
        _reduce(2, t, 6, ptr, out=alpha, iso=iso)
        return alpha, iso

    def tensor_form(self, s: torch.Tensor, x: torch.Tensor, data: Dict[str, torch.Tensor]):
        """The reference's op sequence (nn/output.py:288-326) on differentiable device tensor operations."""
        equi = self.equi_out_mlp(x)                                  # [n, 6]: 1x0e + 1x2e
        a = training._mlp(self.scalar_out_mlp, s)                    # [n, 2]
        p = _graph_sum(torch.cat([equi[:, :1] * a[:, :1], equi[:, 1:6] * a[:, 1:2]], dim=-1), data)
        z, d = p[:, 0], p[:, 1:6]
        dn = torch.linalg.norm(d, dim=-1)
        dxy, dyz, dz2, dzx, dx2 = d.unbind(-1)
        is3 = 1.0 / math.sqrt(3.0)
        xx, yy, zz = is3 * (dn - dz2) + dx2 + z, is3 * (dn - dz2) - dx2 + z, is3 * (dn + 2 * dz2) + z
        alpha = torch.stack([xx, dxy, dzx, dxy, yy, dyz, dzx, dyz, zz], dim=-1).reshape(-1, 3, 3)
        iso = torch.diagonal(alpha, dim1=-2, dim2=-1).mean(dim=-1) if self.isotropic else None
        return alpha, iso

    def forward(self, data: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        s, x = data[keys.NODE_INVARIANT], data[keys.NODE_EQUIVARIANT]
        if x is None:
            raise KeyError("PolarOut reads the equivariant node features, which the last update block did not form")
        lib.require_hip(s, x)
        if not training.active(self, data) and self._kernel_ok(s, x, data):
            alpha, iso = self._kernel_form(s, x, data)
        else:
            alpha, iso = self.tensor_form(s, x, data)
        data[keys.POLARIZABILITY] = alpha
        if iso is not None:
            data[keys.ISO_POLARIZABILITY] = iso
        return data


def refuse_extra_heads(model, who: str) -> None:
    """The capture classes, the native operator and the MD fronts return the energy and its derivatives only: a model with any
    other output head is refused there (runtime.GraphedModel and the eager model evaluate every head)."""
    m = model
    while not isinstance(m, nn.Module) and hasattr(m, "model"):    # a plain callable around a module (md_model._Core)
        m = m.model
    if isinstance(m, nn.Module):
        extra = sorted({type(x).__name__ for x in m.modules() if isinstance(x, OutputModule) and not isinstance(x, EnergyOut)})
        if extra:
            raise ValueError(f"{who} evaluates the energy output head alone: a model with another output head ({', '.join(extra)}) is "
                             "refused (use GraphedModel or the eager model)")
    refuse_ewald(model, who)


def refuse_ewald(model, who: str) -> None:
    """The same fronts walk the energy chain embedding - message / update blocks - energy head themselves: they would skip the
    Ewald modules of an XPaiNNEwald and return the short-range energy alone, so that model is refused there (the eager model
    evaluates it)."""
    m = model
    while not isinstance(m, nn.Module) and hasattr(m, "model"):
        m = m.model
    if isinstance(m, nn.Module):
        from .ewald import EwaldBlock, _EwaldInitial

        if any(isinstance(x, (EwaldBlock, _EwaldInitial)) for x in m.modules()):
            raise ValueError(f"{who} evaluates the energy chain of XPaiNN alone: an XPaiNNEwald model (\"xpainn-ewald\", "
                             f"{type(m).__name__} with Ewald modules) is refused; evaluate it with the eager model")


_NOT_BUILT = {
    "dipole": "the DipoleOut head stays outside this package's scope (DESIGN.md: its refusal is part of the pinned factory contract)",
    "spatial": "SpatialOut needs the reference's atomic mass table, which this package does not carry",
    "cartesian": "CartTensorOut needs SelfMixTP and Sph2Cart, which this package does not build",
}


def resolve_output(mode: str, **kwargs) -> OutputModule:
    """nn/output.py output factory: energy, scalar, charges / atomic_charges, polar."""
    if mode == "energy":
        return EnergyOut(**{k: v for k, v in kwargs.items() if k in ("node_dim", "hidden_dim", "activation", "node_shift", "node_scale")})
    factory = {"scalar": ScalarOut, "charges": AtomicChargesOut, "atomic_charges": AtomicChargesOut, "polar": PolarOut}
    if mode in factory:
        return factory[mode](**kwargs)
    if mode in _NOT_BUILT:
        raise NotImplementedError(f"output mode {mode!r} is not built: {_NOT_BUILT[mode]}")
    raise NotImplementedError(f"output mode {mode!r} is outside the energy+force hot path")
