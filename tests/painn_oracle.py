"""CPU restatement of the reference's PaiNN blocks (nn/painn.py:13-166) and of the model built from them (nn/model.py:261-307) on
plain torch operations, for the fixture checks (tests/test_painn_host.py) and as the f64 / f32 oracle of tests/test_gpu_painn.py.

Functional on a reference-layout state dict ``p``: ``embedding.embedding.1.weight`` (or ``embedding.embedding.weight`` for the
one-hot table), ``embedding.rbf.freq``, ``message_i.scalar_mlp.{0,2}.*``, ``message_i.rbf_lin.*``, ``update_i.update_{U,V}.weight``,
``update_i.update_mlp.{0,2}.*``; autograd runs through all of them.  Node vectors are Cartesian [N, 3, F] in x, y, z order.
Bessel basis and cosine envelope only (the defaults of the model); the other radial kinds and the polynomial envelope, with ``h``
and ``a`` as inputs, are restated in tests/painn_kernel_cases.py (pinned to ``message`` / ``update`` here for Bessel + cosine)."""
import math

import numpy as np
import torch


def _silu(x):
    return x * torch.sigmoid(x)


def _lin(x, p, name):
    y = x @ p[name + ".weight"].T
    return y + p[name + ".bias"] if name + ".bias" in p else y


def _mlp(x, p, name):
    return _lin(_silu(_lin(x, p, name + ".0")), p, name + ".2")


def edge_vectors(pos, edge_index, cell=None, cell_offsets=None, batch=None, strain=None):
    """vec = pos[center] - pos[neighbor] - offsets @ cell (nn/basic.py:110-131), positions and cell scaled by 1 + sym(strain)."""
    center, nbr = edge_index[0].long(), edge_index[1].long()
    if strain is not None:
        sym = 0.5 * (strain + strain.transpose(1, 2))
        pos = pos + torch.bmm(pos.unsqueeze(1), sym[batch]).squeeze(1)
        if cell is not None:
            cell = cell + torch.bmm(cell, sym)
    vec = pos[center] - pos[nbr]
    if cell is not None:
        vec = vec - torch.einsum("ni,nij->nj", cell_offsets.to(pos.dtype), cell[batch[nbr]])
    return vec


def radial(vec, freq, cutoff, eps=1e-5):
    """(rbf [E, B], fcut [E, 1], u [E, 3]) of nn/painn.py:48-53."""
    d = torch.linalg.norm(vec, dim=-1, keepdim=True)
    rbf = math.sqrt(2.0 / cutoff) * torch.sin(freq.reshape(1, -1) * d) / (d + eps)
    fcut = torch.where(d < cutoff, 0.5 * (torch.cos(math.pi * d / cutoff) + 1.0), torch.zeros_like(d))
    return rbf, fcut, vec / d


def embedding(z, p, table=None, prefix="embedding."):
    if prefix + "embedding.weight" in p:
        return p[prefix + "embedding.weight"][z.long()]
    t = p[prefix + "embedding.0.embed_ten"] if table is None else table
    return _lin(t[z.long()].to(p[prefix + "embedding.1.weight"].dtype), p, prefix + "embedding.1")


def message(s, x, rbf, fcut, u, edge_index, p, prefix):
    """nn/painn.py:99-117"""
    center, nbr = edge_index[0].long(), edge_index[1].long()
    F = s.shape[1]
    h = _mlp(s, p, prefix + "scalar_mlp")
    filt = _lin(rbf, p, prefix + "rbf_lin") * fcut
    m_s, g_edge, g_state = torch.split(h[nbr] * filt, F, dim=-1)
    m_v = x[nbr] * g_state.unsqueeze(1) + g_edge.unsqueeze(1) * u.unsqueeze(-1)
    return s.index_add(0, center, m_s), x.index_add(0, center, m_v)


def update(s, x, p, prefix):
    """nn/painn.py:146-164"""
    F = s.shape[1]
    U, V = _lin(x, p, prefix + "update_U"), _lin(x, p, prefix + "update_V")
    a = _mlp(torch.cat([s, torch.linalg.norm(V, dim=1)], dim=-1), p, prefix + "update_mlp")
    a_ss, a_vv, a_sv = torch.split(a, F, dim=-1)
    return s + a_sv * (U * V).sum(1) + a_ss, x + a_vv.unsqueeze(1) * U


def blocks(z, vec, edge_index, p, n_blocks, cutoff, prefix="", table=None, collect=None):
    """Embedding and ``n_blocks`` x (message, update); returns (s, x).  ``collect``: a list that receives s after every block."""
    s = embedding(z, p, table, prefix + "embedding.")
    x = torch.zeros((s.shape[0], 3, s.shape[1]), dtype=s.dtype)
    rbf, fcut, u = radial(vec, p[prefix + "embedding.rbf.freq"], cutoff)
    for i in range(n_blocks):
        s, x = message(s, x, rbf, fcut, u, edge_index, p, f"{prefix}message_{i}.")
        s, x = update(s, x, p, f"{prefix}update_{i}.")
        if collect is not None:
            collect.append(s)
    return s, x


def energy_out(s, batch, n_graphs, p, prefix="output_energy."):
    """EnergyOut (nn/output.py:114-128): Linear-SiLU-Linear per atom, summed per graph."""
    atom = _mlp(s, p, prefix + "out_mlp").reshape(-1)
    return torch.zeros(n_graphs, dtype=s.dtype).index_add(0, batch.long(), atom)


def model(p, z, pos, edge_index, batch, n_graphs, n_blocks, cutoff, cell=None, cell_offsets=None, virial=False, w_out=None,
          create_graph=False):
    """Energies, forces (and the virial) of the PaiNN model on a ``mods.``-prefixed state dict; ``w_out`` replaces the energy head
    by a linear readout s @ w_out (what the fixtures store)."""
    pos = pos.clone().requires_grad_()
    strain = torch.zeros((n_graphs, 3, 3), dtype=pos.dtype, requires_grad=True) if virial else None
    vec = edge_vectors(pos, edge_index, cell, cell_offsets, batch.long(), strain)
    pre = "mods." if any(k.startswith("mods.") for k in p) else ""
    s, _ = blocks(z, vec, edge_index, p, n_blocks, cutoff, pre)
    if w_out is not None:
        energy = torch.zeros(n_graphs, dtype=s.dtype).index_add(0, batch.long(), s @ w_out)
    else:
        energy = energy_out(s, batch, n_graphs, p, pre + "output_energy.")
    wrt = [pos] + ([strain] if virial else [])
    g = torch.autograd.grad([energy], wrt, [torch.ones_like(energy)], create_graph=create_graph)
    out = {"energy": energy, "forces": -g[0]}
    if virial:
        out["virial"] = -g[1]
    return out


# ---- seeded weights shared by the fixture generator and the tests ------------------------------------------------------------------
def seeded_weights(shapes, seed, dtype=torch.float64):
    """Values for every ``*.weight`` / ``*.bias`` entry of ``shapes`` (name -> shape, walked in sorted order) from one numpy
    generator: weights ~ N(0, 1 / fan_in) (unit variance for an embedding table, row 0 kept zero), biases ~ N(0, 0.1^2)."""
    rng = np.random.default_rng(int(seed))
    out = {}
    for k in sorted(shapes):
        shape = tuple(int(n) for n in shapes[k])
        if k.endswith(".bias"):
            v = 0.1 * rng.standard_normal(shape)
        elif k.endswith("embedding.weight"):
            v = rng.standard_normal(shape)
            v[0] = 0.0
        elif k.endswith(".weight"):
            v = rng.standard_normal(shape) / math.sqrt(shape[-1])
        else:
            continue
        out[k] = torch.tensor(v, dtype=dtype)
    return out


def cast(p, dtype):
    return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in p.items()}
