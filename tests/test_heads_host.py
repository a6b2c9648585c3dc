"""Host-side checks of the property heads (nn/output.py: ScalarOut, AtomicChargesOut, PolarOut): the factory, names and shapes against
tests/golden/heads_keys.json, reference state dicts, what the heads ask of the trunk, properties of the f64 restatement
(tests/heads_oracle.py) and the C ABI.  No GPU."""
import json
import math
import os

import numpy as np
import pytest
import torch

from oracle import xpainn_oracle as orc
from tests import heads_oracle as ho
from xequinet_amd import keys, lib
from xequinet_amd.data import synthetic as syn
from xequinet_amd.nn import resolve_model, resolve_output

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NARROW = dict(node_dim=32, node_irreps="32x0e+16x1o+8x2e", hidden_dim=16, hidden_irreps="16x0e+4x2e")


def test_factory_builds_the_three_modes_and_the_alias():
    from xequinet_amd.nn.output import AtomicChargesOut, PolarOut, ScalarOut

    assert isinstance(resolve_output("scalar"), ScalarOut)
    assert isinstance(resolve_output("charges"), AtomicChargesOut) and isinstance(resolve_output("atomic_charges"), AtomicChargesOut)
    polar = resolve_output("polar")
    assert isinstance(polar, PolarOut) and polar.reads_equivariant
    assert resolve_output("scalar").extra_properties == [keys.SCALAR_OUTPUT] == ["scalar_output"]
    assert resolve_output("scalar", output_field="gap").extra_properties == ["gap"]
    assert resolve_output("charges").extra_properties == [keys.ATOMIC_CHARGES] == ["atomic_charges"]
    assert polar.extra_properties == [keys.POLARIZABILITY] == ["polarizability"]
    assert resolve_output("polar", isotropic=True).extra_properties == [keys.ISO_POLARIZABILITY] == ["iso_polarizability"]
    with pytest.raises(NotImplementedError):
        resolve_output("scalar", reduce_op="max")
    q = resolve_output("charges")
    assert float(q.out_mlp[0].bias.detach().abs().max()) == 0.0 and float(q.out_mlp[2].bias.detach().abs().max()) == 0.0
    s = resolve_output("scalar", node_shift=2.5, node_scale=3.0)
    assert float(s.out_mlp[2].bias.detach()) == 2.5


@pytest.mark.parametrize("mode,word", [("dipole", "DipoleOut"), ("spatial", "mass"), ("cartesian", "SelfMixTP")])
def test_modes_outside_the_scope_still_refuse_with_their_reason(mode, word):
    with pytest.raises(NotImplementedError, match=word):
        resolve_output(mode)
    with pytest.raises(NotImplementedError):
        resolve_model("painn", output_modes=["polar"])


@pytest.mark.parametrize("case", [0, 1])
def test_names_and_shapes_match_the_fixture(case):
    from xequinet_amd.nn import output

    with open(os.path.join(GOLDEN, "heads_keys.json")) as f:
        c = json.load(f)["cases"][case]
    for cls, want in c["keys"].items():
        sd = getattr(output, cls)(**c["kwargs"]).state_dict()
        assert {k: list(v.shape) for k, v in sd.items()} == want, cls


def test_reference_state_dict_with_e3nn_bookkeeping_loads_and_a_bogus_key_raises():
    torch.manual_seed(0)
    src = resolve_model("xpainn", output_modes=["energy", "scalar", "charges", "polar"])
    model = resolve_model("xpainn", output_modes=["energy", "scalar", "charges", "polar"])
    ref = {k: v.clone() for k, v in src.state_dict().items()}
    for extra in ("mods.output_polar.rsh_conv.weight", "mods.output_polar.rsh_conv.output_mask",
                  "mods.output_polar.equi_out_mlp.1.scalar_mul.weight", "mods.output_polar.equi_out_mlp.1.scalar_mul.output_mask",
                  "mods.output_polar.equi_out_mlp.1.invariant.tp.weight", "mods.output_polar.equi_out_mlp.1.invariant.tp.output_mask",
                  "mods.output_polar.equi_out_mlp.0.output_mask", "mods.output_polar.equi_out_mlp.2.output_mask"):
        ref[extra] = torch.zeros(0)
    model.load_reference_state_dict(ref)
    for k, v in src.state_dict().items():
        assert torch.equal(model.state_dict()[k], v), k
    ref["mods.output_polar.equi_out_mlp.1.activation.0.weight"] = torch.zeros(80, 80)   # Gate(refine=True): not what PolarOut builds
    with pytest.raises(KeyError):
        model.load_reference_state_dict(ref)


def test_polar_keeps_the_last_equivariant_output_and_scalar_drops_it():
    assert resolve_model("xpainn", output_modes=["energy", "polar"]).mods["update_2"].equivariant_output_unused is False
    assert resolve_model("xpainn", output_modes=["energy", "scalar"]).mods["update_2"].equivariant_output_unused is True
    assert resolve_model("xpainn", output_modes=["scalar", "charges"]).mods["update_2"].equivariant_output_unused is True
    assert resolve_model("xpainn").mods["update_2"].equivariant_output_unused is True
    m = resolve_model("xpainn", output_modes=["energy", "scalar", "polar"])
    assert m.extra_properties == ["energy", "atomic_energies", "scalar_output", "polarizability"]


def test_native_pass_and_derivatives_need_the_energy_head_alone():
    from xequinet_amd.nn import training

    assert training.native_pass_supported(resolve_model("xpainn"))
    assert not training.native_pass_supported(resolve_model("xpainn", output_modes=["energy", "scalar"]))
    m = resolve_model("xpainn", output_modes=["scalar"])
    with pytest.raises(KeyError, match="energy"):
        m({"pos": torch.zeros(2, 3)}, compute_forces=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        resolve_output("polar")({keys.NODE_INVARIANT: torch.zeros(2, 128), keys.NODE_EQUIVARIANT: torch.zeros(2, 480),
                                 keys.BATCH: torch.zeros(2, dtype=torch.long), keys.BATCH_PTR: torch.tensor([0, 2])})


def test_fronts_refuse_a_model_with_another_head_on_the_host():
    from xequinet_amd.interface.md_model import XPaiNNGMX, XPaiNNLMP

    with pytest.raises(ValueError, match="output head"):
        XPaiNNLMP(output_modes=["energy", "polar"])
    with pytest.raises(ValueError, match="output head"):
        XPaiNNGMX(output_modes=["energy", "charges"])


# ------------------------------------------------------------------------------------------------------ the restatement (f64)
def _random_rotation(rng):
    q, r = np.linalg.qr(rng.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


@pytest.fixture(scope="module")
def aspirin_polar():
    torch.manual_seed(0)
    model = resolve_model("xpainn", output_modes=["energy", "polar", "charges", "scalar"])
    with torch.no_grad():
        for name in ("output_polar", "output_charges", "output_scalar"):
            for p in model.mods[name].parameters():
                p.mul_(3.0)
    sd = {k: v.detach().double() for k, v in model.state_dict().items()}
    pos, z, ptr = syn.synth_aspirin()
    return sd, pos, z, ptr


def _oracle_heads(sd, pos, z, ptr, charge=None, **kw):
    ei = orc.radius_graph_canonical(pos, ptr, 5.0)
    batch = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
    data = {"pos": torch.tensor(pos, dtype=torch.float64), "atomic_numbers": torch.tensor(z.astype(np.int64)), "edge_index": torch.tensor(ei),
            "batch": torch.tensor(batch), "ptr": torch.tensor(ptr)}
    if charge is not None:
        data["charge"] = torch.tensor(charge)
    o = ho.HeadsOracle(sd, **kw)
    o(data, False, False)
    return {k: v.detach() for k, v in o.heads.items()}


def test_polarizability_is_symmetric_and_rotates_as_a_tensor(aspirin_polar):
    sd, pos, z, ptr = aspirin_polar
    a0 = _oracle_heads(sd, pos, z, ptr)["polarizability"][0]
    assert float((a0 - a0.T).abs().max()) == 0.0
    assert float(a0.abs().max()) > 1e-3
    rng = np.random.default_rng(0)
    for _ in range(3):
        R = _random_rotation(rng)
        a1 = _oracle_heads(sd, pos @ R.T, z, ptr)["polarizability"][0]
        Rt = torch.tensor(R)
        assert float((a1 - Rt @ a0 @ Rt.T).abs().max()) <= 1e-10 * max(1.0, float(a0.abs().max()))


def test_charges_add_up_to_the_total_and_mean_is_sum_over_count(aspirin_polar):
    sd = aspirin_polar[0]
    pos, z, ptr = syn.synth_qm9_batch(6, seed=2)
    batch = torch.tensor(np.repeat(np.arange(6), np.diff(ptr)))
    n = torch.tensor(np.diff(ptr), dtype=torch.float64)
    charge = np.array([2, -1, 0, 1, -2, 0])
    q = _oracle_heads(sd, pos, z, ptr, charge=charge)["atomic_charges"]
    assert float((ho.graph_sum(q, batch, 6) - torch.tensor(charge, dtype=torch.float64)).abs().max()) <= 1e-12
    q0 = _oracle_heads(sd, pos, z, ptr)["atomic_charges"]
    assert float(ho.graph_sum(q0, batch, 6).abs().max()) <= 1e-12
    raw = _oracle_heads(sd, pos, z, ptr, conservation=False)["atomic_charges"]
    assert float(ho.graph_sum(raw, batch, 6).abs().max()) > 1e-6
    total = _oracle_heads(sd, pos, z, ptr)["scalar_output"]
    mean = _oracle_heads(sd, pos, z, ptr, reduce_op="mean")["scalar_output"]
    assert float((mean - total / n).abs().max()) <= 1e-14 * float(total.abs().max())
    assert _oracle_heads(sd, pos, z, ptr, reduce_op=None)["scalar_output"].shape == (int(ptr[-1]),)


def test_rectangular_linear_restatement_equals_the_module_weights_layout():
    """The module's rectangular o3.Linear and the oracle's restatement read the same flat weight the same way (CPU: through the module's
    own block table, its forward refuses host tensors)."""
    from xequinet_amd import o3

    torch.manual_seed(1)
    lin = o3.Linear("32x0e+16x1o+8x2e", "16x0e+4x2e", biases=True)
    assert lin.weight.numel() == 32 * 16 + 8 * 4 and lin.bias.numel() == 16
    assert [(m_in, m_out, l) for m_in, m_out, l, _, _, _ in lin.paths()] == [(32, 16, 0), (8, 4, 2)]
    assert [(x_off, w_off) for _, _, _, x_off, w_off, _ in lin.paths()] == [(0, 0), (32 + 48, 32 * 16)]
    x = torch.randn(5, 32 + 48 + 40, dtype=torch.float64)
    w, b = lin.weight.detach().double(), torch.randn(16, dtype=torch.float64)
    got = ho.o3_linear_rect("32x0e+16x1o+8x2e", "16x0e+4x2e", x, w, b)
    want0 = x[:, :32] @ w[:512].reshape(32, 16) / math.sqrt(32) + b
    want2 = torch.einsum("uw,num->nwm", w[512:].reshape(8, 4), x[:, 80:].reshape(5, 8, 5)) / math.sqrt(8)
    assert torch.allclose(got, torch.cat([want0, want2.reshape(5, 20)], -1), rtol=0, atol=1e-14)
    x1 = x.clone()
    x1[:, 32:80] += 1.0    # the 1o block is unread
    assert torch.equal(ho.o3_linear_rect("32x0e+16x1o+8x2e", "16x0e+4x2e", x1, w, b), got)


# ------------------------------------------------------------------------------------------------------------------ the C ABI
def test_c_abi_exports_and_the_polar_envelope():
    h = lib.load()
    for name in ("xeq_head_polar_supported", "xeq_head_polar_nodes", "xeq_head_graph_reduce"):
        assert name in lib.EXPORTS and getattr(h, name) is not None
    assert h.xeq_head_polar_supported(lib.XEQ_F32, 128, 128, 32, 64, 64, 16) == 1
    assert h.xeq_head_polar_supported(lib.XEQ_F32, 32, 32, 8, 16, 16, 4) == 1
    assert h.xeq_head_polar_supported(lib.XEQ_F64, 128, 128, 32, 64, 64, 16) == 0
    assert h.xeq_head_polar_supported(lib.XEQ_F32, 48, 128, 32, 64, 64, 16) == 0
    assert h.xeq_head_polar_supported(lib.XEQ_F32, 256, 256, 64, 128, 128, 32) == 0    # past the tile's LDS
    # argument checks run before any launch (no GPU needed): a status and xeq_last_error
    st = h.xeq_head_graph_reduce(7, None, 8, 6, None, 1, None, None, None, None)
    assert st != 0 and b"mode" in h.xeq_last_error()
    st = h.xeq_head_graph_reduce(2, None, 8, 5, None, 1, None, None, None, None)
    assert st != 0 and b"six" in h.xeq_last_error()
    st = h.xeq_head_polar_nodes(None, 128, None, 480, 4, 48, 48, 32, 320, 64, 64, 16, None, None, None, None, None, None, None, 1e-5, None, None)
    assert st != 0 and b"envelope" in h.xeq_last_error()
    st = h.xeq_head_polar_nodes(None, 130, None, 480, 4, 128, 128, 32, 320, 64, 64, 16, None, None, None, None, None, None, None, 1e-5, None, None)
    assert st != 0 and b"stride" in h.xeq_last_error()
