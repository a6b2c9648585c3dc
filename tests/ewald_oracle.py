"""Restatement of the reference's Ewald message passing (nn/ewald.py:60-95 EwaldInitialPBC, :98-138 EwaldInitialNonPBC, :141-212
EwaldBlock with the bias-free ResidualLayer of nn/basic.py:11-31) on plain torch operations, in the dtype of its inputs (f64 for the
reference values, f32 for the error the number format alone makes), and ``EwaldOracle``: ``XPaiNNOracle`` with the Ewald modules and
the second energy head behind it (nn/model.py:125-176).

``p`` maps a module's state-dict names to tensors; autograd runs through them.  The pieces the kernels compute on their own
(structure factor, apply, phase gradient) are restated separately so that each C entry point has its own reference."""
import math

import torch
import torch.nn.functional as F

from oracle import xpainn_oracle as orc
from tests.heads_oracle import graph_sum, sub_params


def _silu(x):
    return x * torch.sigmoid(x)


def residual(x, p, prefix):
    """nn/basic.py:11-31 with n_layers = 2: (x + SiLU(W_2 SiLU(W_1 x))) / sqrt(2)."""
    y = _silu(F.linear(_silu(F.linear(x, p[f"{prefix}.mlp.0.weight"])), p[f"{prefix}.mlp.2.weight"]))
    return (x + y) / math.sqrt(2)


def initial_pbc(pos, cell, batch, p):
    """(k_dot_r [n, K], damping, down_projection [K, P]); k_grid = index_set @ (2 pi cell^-1), row convention (ewald.py:80-82)."""
    k_grid = torch.matmul(p["k_index_product_set"], 2 * math.pi * torch.inverse(cell))
    k_dot_r = torch.einsum("aki,ai->ak", k_grid.index_select(0, batch.long()), pos)
    return k_dot_r, torch.ones((), dtype=pos.dtype), p["down_projection"]


def initial_nonpbc(pos, p, delta_k=0.2, eps=1e-5):
    k_dot_r = torch.einsum("ki,ai->ak", p["k_grid"], pos)
    damping = torch.sinc(0.5 * delta_k * pos + eps).prod(dim=-1, keepdim=True)
    return k_dot_r, damping, F.linear(p["k_rbf_values"], p["down.weight"])


def structure_factor(h, k_dot_r, damping, batch, n_graphs):
    """S_R, S_I [G, K, F] (ewald.py:184-196)."""
    real = (torch.cos(k_dot_r) * damping).unsqueeze(-1)
    imag = (torch.sin(k_dot_r) * damping).unsqueeze(-1)
    return graph_sum(real * h.unsqueeze(1), batch, n_graphs), graph_sum(imag * h.unsqueeze(1), batch, n_graphs)


def apply_filter(s_r, s_i, kf, k_dot_r, damping, batch):
    """m [n, F] (ewald.py:199-207)."""
    real = (torch.cos(k_dot_r) * damping).unsqueeze(-1)
    imag = (torch.sin(k_dot_r) * damping).unsqueeze(-1)
    b = batch.long()
    return torch.sum((kf.unsqueeze(0) * s_r).index_select(0, b) * real + (kf.unsqueeze(0) * s_i).index_select(0, b) * imag, dim=1)


def message(h, k_dot_r, damping, kf, batch, n_graphs):
    s_r, s_i = structure_factor(h, k_dot_r, damping, batch, n_graphs)
    return apply_filter(s_r, s_i, kf, k_dot_r, damping, batch)


def ewald_block(s, k_dot_r, damping, down_projection, batch, n_graphs, p, layer_norm=True):
    """EwaldBlock.forward (ewald.py:171-212)."""
    h = residual(s, p, "pre_residual")
    if layer_norm:
        h = F.layer_norm(h, (h.shape[-1],), p["norm.weight"], p["norm.bias"], 1e-5)
    m = message(h, k_dot_r, damping, F.linear(down_projection, p["up.weight"]), batch, n_graphs)
    v = _silu(F.linear(m, p["update_layer.0.weight"]))
    i = 2
    while f"update_layer.{i}.mlp.0.weight" in p:
        v = residual(v, p, f"update_layer.{i}")
        i += 1
    return s + v


class EwaldOracle(orc.XPaiNNOracle):
    """XPaiNNOracle with ``ewald_initial``, ``ewald_i`` and ``ewald_output_energy`` behind the first energy head; the second head adds
    to the atomic energies.  The Ewald modules read the unstrained positions and cell (data["pos"] / data["cell"], which
    oracle.compute_edge_data leaves as they came), so the strain reaches them through the trunk's node scalars alone.
    kwargs beyond the oracle's: ``use_pbc``, ``delta_k``, ``ewald_blocks``."""

    def __init__(self, sd, **kwargs):
        super().__init__(sd, **kwargs)
        self.use_pbc = kwargs.get("use_pbc", True)
        self.delta_k = kwargs.get("delta_k", 0.2)
        self.ewald_blocks = kwargs.get("ewald_blocks", 1)

    def energy_out(self, data):
        data = super().energy_out(data)
        sd, batch, pos = self.sd, data["batch"], data["pos"]
        n_graphs = int(data["ptr"].numel()) - 1
        pi = sub_params(sd, "mods.ewald_initial.")
        if self.use_pbc:
            k_dot_r, damping, down = initial_pbc(pos, data["cell"].reshape(-1, 3, 3), batch, pi)
        else:
            k_dot_r, damping, down = initial_nonpbc(pos, pi, self.delta_k)
        s = data["node_invariant"]
        for i in range(self.ewald_blocks):
            s = ewald_block(s, k_dot_r, damping, down, batch, n_graphs, sub_params(sd, f"mods.ewald_{i}."), self.layer_norm)
        data["node_invariant"] = s
        ph = sub_params(sd, "mods.ewald_output_energy.")
        e_atom = F.linear(self.act(F.linear(s, ph["out_mlp.0.weight"], ph["out_mlp.0.bias"])), ph["out_mlp.2.weight"], ph["out_mlp.2.bias"]).reshape(-1)
        data["atomic_energies"] = data["atomic_energies"] + e_atom
        data["energy"] = graph_sum(data["atomic_energies"], batch, n_graphs)
        return data
