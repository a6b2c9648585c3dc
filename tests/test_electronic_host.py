"""CPU checks of the charge / spin embeddings (nn/electronic.py): the model builds with them in the reference's order and
state-dict layout, the batch container carries per-graph charge / spin, and the float64 restatement the GPU suite uses as its
oracle equals what the reference computes (tests/golden/electronic_f64.npz, written by make_golden_electronic.py)."""
import json
import os

import numpy as np
import pytest
import torch

from tests.electronic_oracle import electronic

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PARAMS = ("linear_q.weight", "linear_q.bias", "linear_k.weight", "linear_v.weight", "residual.mlp.0.weight", "residual.mlp.2.weight")


def _model(**kw):
    from xequinet_amd.nn import resolve_model

    return resolve_model("xpainn", charge_embed=True, spin_embed=True, **kw)


def test_model_builds_in_reference_order():
    from xequinet_amd.nn.electronic import ChargeEmbedding, SpinEmbedding

    model = _model()
    names = list(model.mods.keys())
    assert names[:4] == ["embedding", "charge_embedding", "spin_embedding", "message_0"], names
    assert isinstance(model.mods["charge_embedding"], ChargeEmbedding)
    assert isinstance(model.mods["spin_embedding"], SpinEmbedding)
    # the element-table front of the first block is not wired behind an electronic module
    assert model.mods["embedding"]._next_message == []
    from xequinet_amd.nn import resolve_model

    m = resolve_model("xpainn", spin_embed=True)
    assert "charge_embedding" not in m.mods and list(m.mods)[1] == "spin_embedding"
    assert m.mods["embedding"]._next_message == []
    plain = resolve_model("xpainn")
    assert plain.mods["embedding"]._next_message == [plain.mods["message_0"]]


@pytest.mark.parametrize("node_dim", [128, 16])
def test_state_dict_names_and_shapes_match_reference(node_dim):
    ref = json.load(open(os.path.join(GOLDEN, "electronic_keys.json")))[str(node_dim)]
    kw = {"node_dim": node_dim, "node_irreps": f"{node_dim}x0e + 8x1o + 4x2e", "hidden_dim": 16}
    sd = _model(**kw).state_dict()
    for mod in ("charge_embedding", "spin_embedding"):
        ours = {k[len(f"mods.{mod}."):]: list(v.shape) for k, v in sd.items() if k.startswith(f"mods.{mod}.")}
        assert ours == ref[mod], (mod, ours, ref[mod])


def test_load_reference_state_dict_strict():
    torch.manual_seed(3)
    src = _model()
    ref_sd = {k: v.clone() for k, v in src.state_dict().items()}
    dst = _model()
    dst.load_reference_state_dict(ref_sd)
    for k, v in dst.state_dict().items():
        assert torch.equal(v, ref_sd[k]), k
    bogus = dict(ref_sd)
    bogus["mods.charge_embedding.linear_k.bias"] = torch.zeros(128)
    with pytest.raises(KeyError):
        dst.load_reference_state_dict(bogus)
    missing = {k: v for k, v in ref_sd.items() if k != "mods.spin_embedding.linear_v.weight"}
    with pytest.raises(KeyError):
        dst.load_reference_state_dict(missing)


def test_batch_carries_charge_and_spin():
    from xequinet_amd import keys
    from xequinet_amd.data import XequiBatch

    assert keys.TOTAL_SPIN == "spin" and keys.TOTAL_CHARGE == "charge"
    b = XequiBatch(torch.randn(5, 3), torch.tensor([1, 1, 8, 6, 1]), torch.tensor([0, 3, 5]),
                   charge=torch.tensor([1, -1]), spin=torch.tensor([0, 2]))
    d = b.to("cpu").to_dict()
    assert d["charge"].tolist() == [1, -1] and d["spin"].tolist() == [0, 2]
    plain = XequiBatch(torch.randn(5, 3), torch.tensor([1, 1, 8, 6, 1]), torch.tensor([0, 3, 5]))
    assert "charge" not in plain.to_dict() and "spin" not in plain.to_dict()
    with pytest.raises(ValueError):
        XequiBatch(torch.randn(5, 3), torch.tensor([1, 1, 8, 6, 1]), torch.tensor([0, 3, 5]), charge=torch.tensor([1]))


def test_refuses_host_tensors():
    from xequinet_amd.nn.electronic import ChargeEmbedding

    m = ChargeEmbedding(node_dim=32)
    data = {"node_invariant": torch.randn(3, 32), "batch": torch.zeros(3, dtype=torch.long), "charge": torch.tensor([1])}
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(data)
    assert m({"node_invariant": data["node_invariant"]})["node_invariant"] is data["node_invariant"]   # no key: identity


@pytest.mark.parametrize("case", ["charge", "spin", "both"])
def test_restatement_equals_reference_fixture(case):
    g = np.load(os.path.join(GOLDEN, "electronic_f64.npz"))
    s = torch.tensor(g["s"], requires_grad=True)
    batch = torch.tensor(g["batch"])
    pc = {k: torch.tensor(g[f"w_c_{k}"], requires_grad=True) for k in PARAMS}
    ps = {k: torch.tensor(g[f"w_s_{k}"], requires_grad=True) for k in PARAMS}
    y = s
    used = []
    if case in ("charge", "both"):
        y = electronic(y, batch, torch.tensor(g["charge"]), pc, "charge")
        used.append(("c", pc))
    if case in ("spin", "both"):
        y = electronic(y, batch, torch.tensor(g["spin"]), ps, "spin")
        used.append(("s", ps))
    ref = g[f"out_{case}"]
    assert np.abs(y.detach().numpy() - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())
    (y * torch.tensor(g["probe"])).sum().backward()
    def close(a, b):
        return np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(b).max())

    assert close(s.grad.numpy(), g[f"g_{case}_input"])
    for tag, p in used:
        for k in PARAMS:
            assert close(p[k].grad.numpy(), g[f"g_{case}_{tag}_{k}"]), (case, tag, k)


def test_native_pass_not_taken_with_electronic_modules():
    from xequinet_amd.nn import resolve_model, training

    assert training.native_pass_supported(resolve_model("xpainn"))
    assert not training.native_pass_supported(_model())
    assert not training.native_pass_supported(resolve_model("xpainn", spin_embed=True))
