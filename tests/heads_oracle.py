"""Restatement of the reference's property heads (nn/output.py:28-76 ScalarOut, :131-179 AtomicChargesOut, :245-326 PolarOut with the
Gate of nn/o3layer.py:47-75) on plain torch operations, in the dtype of its inputs (f64 for the reference values, f32 for the error
the number format alone makes), and ``HeadsOracle``: ``XPaiNNOracle`` with the heads applied behind the trunk.

``p`` maps a head's state-dict names to tensors; autograd runs through them.  The rectangular ``o3.Linear`` is restated here (the
oracle's ``o3_linear`` takes equal irreps on both sides): one path per irrep both sides hold, out[w, m] = mul_in^-1/2 sum_u W[u, w]
x[u, m], weight blocks row-major [mul_in, mul_out] in the order of the input irreps, a bias on the 0e output only -- the e3nn
definitions are the [3P-recalled] ones of SURVEY 8c."""
import math

import torch
import torch.nn.functional as F

from oracle import xpainn_oracle as orc


def _silu(x):
    return x * torch.sigmoid(x)


def mlp(s, p, prefix="out_mlp"):
    return F.linear(_silu(F.linear(s, p[f"{prefix}.0.weight"], p[f"{prefix}.0.bias"])), p[f"{prefix}.2.weight"], p[f"{prefix}.2.bias"])


def graph_sum(src, batch, n_graphs):
    return torch.zeros((n_graphs,) + tuple(src.shape[1:]), dtype=src.dtype).index_add(0, batch.long(), src)


def scalar_out(s, batch, n_graphs, p, reduce_op="sum"):
    r = mlp(s, p).reshape(-1)
    if reduce_op is None:
        return r
    out = graph_sum(r, batch, n_graphs)
    if reduce_op == "mean":
        out = out / torch.bincount(batch.long(), minlength=n_graphs).clamp(min=1).to(out.dtype)
    elif reduce_op != "sum":
        raise NotImplementedError(reduce_op)
    return out


def charges_out(s, batch, n_graphs, p, total=None, conservation=True):
    q = mlp(s, p).reshape(-1)
    if conservation:
        raw = graph_sum(q, batch, n_graphs)
        n = torch.bincount(batch.long(), minlength=n_graphs).clamp(min=1).to(q.dtype)
        target = torch.zeros_like(raw) if total is None else total.reshape(-1).to(q.dtype)
        q = q + ((target - raw) / n)[batch.long()]
    return q


def o3_linear_rect(irreps_in, irreps_out, x, weight, bias):
    """``o3.Linear(irreps_in, irreps_out, biases=True)`` for irreps that differ."""
    blocks_in = {(l, par): (mul, off) for (mul, l, par), (_, _, off, _) in zip(orc.parse_irreps(irreps_in), orc._blocks(irreps_in))}
    w_of, woff = {}, 0
    for mul_in, l, par in orc.parse_irreps(irreps_in):
        for mul_out, l2, par2 in orc.parse_irreps(irreps_out):
            if (l, par) == (l2, par2):
                w_of[(l, par)] = weight[woff : woff + mul_in * mul_out].reshape(mul_in, mul_out)
                woff += mul_in * mul_out
    assert woff == weight.numel()
    parts, boff = [], 0
    for mul_out, l, par in orc.parse_irreps(irreps_out):
        d = 2 * l + 1
        if (l, par) in w_of:
            mul_in, off = blocks_in[(l, par)]
            xb = x[:, off : off + mul_in * d].reshape(-1, mul_in, d)
            ob = torch.einsum("uw,num->nwm", w_of[(l, par)], xb) / math.sqrt(mul_in)
        else:
            ob = x.new_zeros((x.shape[0], mul_out, d))
        if l == 0 and par == 1 and bias is not None and bias.numel() > 0:
            ob = ob + bias[boff : boff + mul_out].reshape(1, mul_out, 1)
            boff += mul_out
        parts.append(ob.reshape(x.shape[0], mul_out * d))
    return torch.cat(parts, dim=-1)


def gate(irreps, x, eps=1e-5):
    """Gate(irreps, "silu", refine=False): every channel times sigmoid(Invariant) of its own irrep."""
    return orc.elementwise_tp(irreps, x, torch.sigmoid(orc.invariant(irreps, x, eps=eps)))


def polar_tensor(p6):
    """z I + A from the graph sums (z, dxy, dyz, dz2, dzx, dx2-y2), nn/output.py:301-320."""
    z, d = p6[:, 0], p6[:, 1:6]
    dn = torch.linalg.norm(d, dim=-1)
    dxy, dyz, dz2, dzx, dx2 = d.unbind(-1)
    c = 1 / math.sqrt(3)
    second = torch.stack([c * (dn - dz2) + dx2, dxy, dzx, dxy, c * (dn - dz2) - dx2, dyz, dzx, dyz, c * (dn + 2 * dz2)], dim=-1).reshape(-1, 3, 3)
    return torch.diag_embed(z.unsqueeze(-1).repeat(1, 3)) + second


def polar_nodes(s, x, p, node_irreps="128x0e + 64x1o + 32x2e", hidden_irreps="64x0e + 16x2e"):
    """t [n, 6]: (a0 t0, a2 t2) per node."""
    a = mlp(s, p, "scalar_out_mlp")
    h = o3_linear_rect(node_irreps, hidden_irreps, x, p["equi_out_mlp.0.weight"], p["equi_out_mlp.0.bias"])
    t = o3_linear_rect(hidden_irreps, "1x0e + 1x2e", gate(hidden_irreps, h), p["equi_out_mlp.2.weight"], p["equi_out_mlp.2.bias"])
    return torch.cat([a[:, :1] * t[:, :1], a[:, 1:2] * t[:, 1:6]], dim=-1)


def polar_out(s, x, batch, n_graphs, p, node_irreps="128x0e + 64x1o + 32x2e", hidden_irreps="64x0e + 16x2e"):
    alpha = polar_tensor(graph_sum(polar_nodes(s, x, p, node_irreps, hidden_irreps), batch, n_graphs))
    return alpha, torch.diagonal(alpha, dim1=-2, dim2=-1).mean(dim=-1)


def sub_params(state_dict, prefix):
    return {k[len(prefix):]: v for k, v in state_dict.items() if k.startswith(prefix)}


class HeadsOracle(orc.XPaiNNOracle):
    """XPaiNNOracle with the restated heads behind the trunk.  The energy head stays the oracle's; the other heads' outputs of the last
    call are kept in ``self.heads`` (with their autograd graph).  A model without an energy head is called with compute_forces=False.
    kwargs beyond the oracle's: ``hidden_irreps``, ``reduce_op``, ``conservation``."""

    def __init__(self, sd, **kwargs):
        super().__init__(sd, **kwargs)
        self.hidden_irreps = kwargs.get("hidden_irreps", "64x0e + 16x2e")
        self.reduce_op = kwargs.get("reduce_op", "sum")
        self.conservation = kwargs.get("conservation", True)
        self.heads = {}

    def energy_out(self, data):
        sd, s, batch = self.sd, data["node_invariant"], data["batch"]
        n_graphs = int(data["ptr"].numel()) - 1
        if any(k.startswith("mods.output_energy.") for k in sd):
            data = super().energy_out(data)
        else:
            data["atomic_energies"] = torch.zeros(s.shape[0], dtype=s.dtype)
            data["energy"] = torch.zeros(n_graphs, dtype=s.dtype)
        self.heads = {}
        if any(k.startswith("mods.output_scalar.") for k in sd):
            self.heads["scalar_output"] = scalar_out(s, batch, n_graphs, sub_params(sd, "mods.output_scalar."), self.reduce_op)
        for mode in ("charges", "atomic_charges"):
            if any(k.startswith(f"mods.output_{mode}.") for k in sd):
                self.heads["atomic_charges"] = charges_out(s, batch, n_graphs, sub_params(sd, f"mods.output_{mode}."), data.get("charge"),
                                                           self.conservation)
        if any(k.startswith("mods.output_polar.") for k in sd):
            alpha, iso = polar_out(s, data["node_equivariant"], batch, n_graphs, sub_params(sd, "mods.output_polar."), self.irreps,
                                   self.hidden_irreps)
            self.heads["polarizability"], self.heads["iso_polarizability"] = alpha, iso
        return data
