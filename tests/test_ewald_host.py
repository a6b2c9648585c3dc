"""Host checks of the XPaiNNEwald front (nn/ewald.py, nn/model.py): the factory and the state-dict layout against the reference's
(tests/golden/ewald_keys.json), the constructed buffers, the tensor form of every module and the restatement of tests/ewald_oracle.py
in f64 on CPU tensors against values the reference itself produced (tests/golden/ewald_f64.npz, make_golden_ewald.py), and the refusals
of the fronts that evaluate the energy chain alone.  No GPU is needed."""
import json
import os

import numpy as np
import pytest
import torch

from tests import ewald_oracle as eo
from xequinet_amd import keys
from xequinet_amd.nn import resolve_model
from xequinet_amd.nn.ewald import EwaldBlock, EwaldInitialNonPBC, EwaldInitialPBC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL = 1e-10
SMALL = dict(node_dim=32, node_irreps="32x0e+16x1o+8x2e", action_blocks=2, ewald_blocks=1)


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(GOLDEN, "ewald_f64.npz")))


@pytest.fixture(scope="module")
def ref_keys():
    with open(os.path.join(GOLDEN, "ewald_keys.json")) as f:
        return json.load(f)


def _modules(fx, tag):
    """The fixture's block and initial module (f64, on the CPU) with the fixture's weights."""
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        block = EwaldBlock(node_dim=32, projection_dim=8)
        init = EwaldInitialPBC([1, 1, 2], projection_dim=8) if tag == "pbc" else EwaldInitialNonPBC(0.4, 0.2, 20, projection_dim=8)
    finally:
        torch.set_default_dtype(old)
    block.load_state_dict({k[len("w_block_"):]: torch.from_numpy(v) for k, v in fx.items() if k.startswith("w_block_")})
    init.load_state_dict({k[len(f"w_{tag}_"):]: torch.from_numpy(v) for k, v in fx.items() if k.startswith(f"w_{tag}_")})
    return block, init


def _err(got, want):
    want = torch.as_tensor(want, dtype=torch.float64)
    return float((got.detach() - want).abs().max())


def test_factory_builds_the_reference_layout(ref_keys):
    """resolve_model("xpainn-ewald") builds; module order, state-dict names and shapes are the reference's; a reference state dict loads."""
    for use_pbc, init_key in ((True, "ewald_initial_pbc"), (False, "ewald_initial_nonpbc")):
        for node_dim, irreps in ((128, "128x0e + 64x1o + 32x2e"), (32, "32x0e+16x1o+8x2e")):
            model = resolve_model("xpainn-ewald", node_dim=node_dim, node_irreps=irreps, action_blocks=2, ewald_blocks=2, use_pbc=use_pbc)
            assert list(model.mods.keys()) == ["embedding", "message_0", "update_0", "message_1", "update_1", "output_energy", "ewald_initial",
                                               "ewald_0", "ewald_1", "ewald_output_energy"]
            sd = model.state_dict()
            expect = {f"mods.ewald_initial.{k}": v for k, v in ref_keys[str(node_dim)][init_key].items()}
            for i in range(2):
                expect.update({f"mods.ewald_{i}.{k}": v for k, v in ref_keys[str(node_dim)]["ewald_block"].items()})
            got = {k: list(v.shape) for k, v in sd.items() if k.startswith("mods.ewald_") and not k.startswith("mods.ewald_output")}
            assert got == expect
            assert [k for k in sd if k.startswith("mods.ewald_output_energy.")] == [f"mods.ewald_output_energy.out_mlp.{i}.{w}" for i in (0, 2)
                                                                                    for w in ("weight", "bias")]
            model.load_reference_state_dict({k: v.clone() for k, v in sd.items()})
            assert model.extra_properties == [keys.TOTAL_ENERGY, keys.ATOMIC_ENERGIES] * 2
    assert (keys.K_DOT_R, keys.SINC_DAMPING, keys.DOWN_PROJECTION) == ("k_dot_r", "sinc_damping", "down_projection")
    # a plain string is one mode; the kwargs are read as in the reference
    m = resolve_model("XPaiNN-Ewald", ewald_output_mode="energy", use_pbc=False, k_cutoff=0.6, delta_k=0.3, num_k_basis=12, projection_dim=4,
                      ewald_blocks=1, **{k: v for k, v in SMALL.items() if k != "ewald_blocks"})
    assert "ewald_output_energy" in m.mods and m.mods["ewald_initial"].down.weight.shape == (4, 12) and m.mods["ewald_0"].up.weight.shape == (32, 4)
    with pytest.raises(NotImplementedError):
        resolve_model("xpainn-ewald", ewald_output_mode="dipole", **SMALL)


def test_block_state_dict_names():
    assert list(EwaldBlock(node_dim=32).state_dict()) == [
        "norm.weight", "norm.bias", "pre_residual.mlp.0.weight", "pre_residual.mlp.2.weight", "up.weight", "update_layer.0.weight",
        "update_layer.2.mlp.0.weight", "update_layer.2.mlp.2.weight", "update_layer.3.mlp.0.weight", "update_layer.3.mlp.2.weight",
        "update_layer.4.mlp.0.weight", "update_layer.4.mlp.2.weight"]
    assert list(EwaldInitialPBC([1, 1, 2]).state_dict()) == ["down_projection", "k_index_product_set"]
    assert list(EwaldInitialNonPBC(0.4, 0.2, 20).state_dict()) == ["k_grid", "k_rbf_values", "down.weight"]


def test_buffers_equal_the_reference(ref_keys):
    ks = EwaldInitialPBC([3, 3, 3]).k_index_product_set
    assert ks.shape == (171, 3) and ks.long().tolist() == ref_keys["k_index_product_set_333"]
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        init = EwaldInitialNonPBC(0.4, 0.2, 20)
    finally:
        torch.set_default_dtype(old)
    assert init.k_grid.shape == (13, 3) and init.k_rbf_values.shape == (13, 20)
    assert _err(init.k_grid, ref_keys["nonpbc_k_grid"]) <= 1e-15
    assert _err(init.k_rbf_values, ref_keys["nonpbc_k_rbf_values"]) <= 1e-15


@pytest.mark.parametrize("tag", ["pbc", "nonpbc"])
def test_tensor_form_reproduces_the_reference(fx, tag):
    """Outputs and every gradient of L = sum(out * probe), f64 on CPU tensors, to 1e-10."""
    block, init = _modules(fx, tag)
    s = torch.from_numpy(fx["s"]).requires_grad_(True)
    pos = torch.from_numpy(fx["pos"]).requires_grad_(True)
    data = {keys.BATCH: torch.from_numpy(fx["batch"]), keys.BATCH_PTR: torch.from_numpy(fx["ptr"]), keys.NODE_INVARIANT: s, keys.POSITIONS: pos,
            keys.CELL: torch.from_numpy(fx["cell"])}
    out = block(init(data))[keys.NODE_INVARIANT]
    (out * torch.from_numpy(fx["probe"])).sum().backward()
    assert _err(out, fx[f"out_{tag}"]) <= TOL
    assert _err(s.grad, fx[f"g_{tag}_input"]) <= TOL
    assert _err(pos.grad, fx[f"g_{tag}_pos"]) <= TOL
    assert float(np.abs(fx[f"g_{tag}_pos"]).max()) > 1e-3   # the positions matter in the fixture
    for k, p in block.named_parameters():
        assert _err(p.grad, fx[f"g_{tag}_block_{k}"]) <= TOL, k
    for k, p in init.named_parameters():
        assert _err(p.grad, fx[f"g_{tag}_init_{k}"]) <= TOL, k


def test_tensor_form_differentiates_twice(fx):
    block, init = _modules(fx, "nonpbc")
    n = 3
    s = torch.from_numpy(fx["s"][:n]).requires_grad_(True)
    pos = torch.from_numpy(fx["pos"][:n]).requires_grad_(True)
    data = {keys.BATCH: torch.tensor([0, 1, 1]), keys.NODE_INVARIANT: s, keys.POSITIONS: pos}
    out = block(init(data))[keys.NODE_INVARIANT]
    (g,) = torch.autograd.grad(out.sum(), pos, create_graph=True)
    g.square().sum().backward()
    assert float(block.up.weight.grad.abs().max()) > 0 and float(pos.grad.abs().max()) > 0


@pytest.mark.parametrize("tag", ["pbc", "nonpbc"])
def test_oracle_reproduces_the_reference(fx, tag):
    pb = {k[len("w_block_"):]: torch.from_numpy(v).requires_grad_(v.dtype == np.float64) for k, v in fx.items() if k.startswith("w_block_")}
    pi = {k[len(f"w_{tag}_"):]: torch.from_numpy(v) for k, v in fx.items() if k.startswith(f"w_{tag}_")}
    learn = "down_projection" if tag == "pbc" else "down.weight"
    pi[learn].requires_grad_(True)
    s = torch.from_numpy(fx["s"]).requires_grad_(True)
    pos = torch.from_numpy(fx["pos"]).requires_grad_(True)
    batch = torch.from_numpy(fx["batch"])
    if tag == "pbc":
        kdr, damp, down = eo.initial_pbc(pos, torch.from_numpy(fx["cell"]), batch, pi)
    else:
        kdr, damp, down = eo.initial_nonpbc(pos, pi)
    out = eo.ewald_block(s, kdr, damp, down, batch, len(fx["ptr"]) - 1, pb)
    (out * torch.from_numpy(fx["probe"])).sum().backward()
    assert _err(out, fx[f"out_{tag}"]) <= TOL
    assert _err(s.grad, fx[f"g_{tag}_input"]) <= TOL
    assert _err(pos.grad, fx[f"g_{tag}_pos"]) <= TOL
    for k, p in pb.items():
        assert _err(p.grad, fx[f"g_{tag}_block_{k}"]) <= TOL, k
    assert _err(pi[learn].grad, fx[f"g_{tag}_init_{learn}"]) <= TOL


def test_native_pass_is_not_offered():
    from xequinet_amd.nn import training

    assert not training.native_pass_supported(resolve_model("xpainn-ewald", **SMALL))
    assert training.native_pass_supported(resolve_model("xpainn", **{k: v for k, v in SMALL.items() if k != "ewald_blocks"}))


FRONTS = ["GraphedModel", "GraphedStep", "GraphedLanes", "GraphedStepsInFlight", "GraphedChunks", "GraphedStepPBC"]


@pytest.mark.parametrize("front", FRONTS + ["GraphedTrainStep", "XPaiNNNative", "compile_model", "resolve_jit_model", "refuse_ewald"])
def test_energy_chain_fronts_refuse_the_model(front):
    """Every front that walks the energy chain itself refuses an XPaiNNEwald at construction, with a ValueError that names the model."""
    model = resolve_model("xpainn-ewald", use_pbc=False, **SMALL)
    with pytest.raises(ValueError, match="XPaiNNEwald"):
        if front in FRONTS:
            from xequinet_amd import runtime

            args = {"GraphedModel": (), "GraphedChunks": ([0, 3],), "GraphedStepPBC": (3, 64)}.get(front, ((8, 64, 1),))
            getattr(runtime, front)(model, *args)
        elif front == "GraphedTrainStep":
            from xequinet_amd import train

            train.GraphedTrainStep(model, torch.optim.SGD(model.parameters(), lr=1e-3), (8, 64, 1))
        elif front == "XPaiNNNative":
            from xequinet_amd.interface import scripted

            scripted.XPaiNNNative(model)
        elif front == "compile_model":
            from xequinet_amd.interface import scripted

            scripted.compile_model(model)
        elif front == "resolve_jit_model":
            from xequinet_amd.interface import resolve_jit_model

            resolve_jit_model("lmp", model_name="xpainn-ewald", **SMALL)
        else:
            from xequinet_amd.nn.output import refuse_ewald

            class Core:   # a plain callable around the module, as the MD fronts hold it
                def __init__(self, m):
                    self.model = m

            refuse_ewald(Core(model), "a front")
