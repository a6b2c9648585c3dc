"""Float64 restatement of the reference's charge / spin embeddings (nn/electronic.py:13-90, ResidualLayer nn/basic.py:11-31) on
plain torch operations, for the fixture check (tests/test_electronic_host.py) and the model oracle of tests/test_gpu_electronic.py.

``p`` maps the module's state-dict names (``linear_q.weight``, ``linear_q.bias``, ``linear_k.weight``, ``linear_v.weight``,
``residual.mlp.0.weight``, ``residual.mlp.2.weight``) to tensors; autograd runs through them."""
import math

import torch


def _silu(x):
    return x * torch.sigmoid(x)


def electronic(s, batch, total, p, kind):
    """s + residual(attn v / A) for kind "charge" (a = relu([t, -t])) or "spin" (a = [t])."""
    t = total.reshape(-1).to(s.dtype)
    a = torch.stack([t.clamp(min=0), (-t).clamp(min=0)], dim=-1) if kind == "charge" else t.unsqueeze(-1)
    key_in = a / torch.clamp(a, min=1.0)
    batch = batch.long()
    q = s @ p["linear_q.weight"].T + p["linear_q.bias"]
    k = (key_in @ p["linear_k.weight"].T)[batch]
    v = (a @ p["linear_v.weight"].T)[batch]
    attn = torch.nn.functional.softplus((q * k).sum(-1, keepdim=True) / math.sqrt(s.shape[1]))
    total_attn = torch.zeros((a.shape[0], 1), dtype=s.dtype).index_add(0, batch, attn)[batch]
    c = attn * v / total_attn
    h = _silu(_silu(c @ p["residual.mlp.0.weight"].T) @ p["residual.mlp.2.weight"].T)
    return s + (c + h) / math.sqrt(2.0)


def sub_params(state_dict, prefix):
    """The electronic module's parameters out of a model state dict (``mods.charge_embedding.`` ...)."""
    return {k[len(prefix):]: v for k, v in state_dict.items() if k.startswith(prefix)}
