"""Whole models at node_dim other than 128, where the two-layer MLPs run xeq_mlp2h_fwd / _bwd (csrc/xeq_mlp.hip): PaiNN takes its native
form (every launch this library's), XPaiNN keeps its MLPs off the library GEMMs, in the Python modules and in xeq::xpainn_eval alike.
Helpers, oracles and bounds are those of tests/test_gpu_painn.py (PaiNN) and tests/test_gpu_parity.py (XPaiNN)."""
import numpy as np
import pytest
import torch

from oracle import xpainn_oracle as orc
from xequinet_amd import lib
from xequinet_amd.data import synthetic as syn

from . import test_gpu_painn as TP
from . import test_gpu_parity as P

pytestmark = pytest.mark.gpu

PAINN_WIDTHS = (32, 64, 256)
XPAINN_CONFIGS = {"64": dict(node_dim=64, node_irreps="64x0e+32x1o+32x2e"),
                  "256": dict(node_dim=256, node_irreps="256x0e+64x1o+32x2e", action_blocks=1)}


# ------------------------------------------------------------------------------------------------------------------------- PaiNN
@pytest.mark.parametrize("F", PAINN_WIDTHS)
def test_painn_runs_its_native_form_at_other_widths(F):
    """qm9 x 8 against the f64 oracle; the second evaluation's launches are the library's, with the count and structure of the 128-wide
    model (tests/test_gpu_painn.py) and the MLPs under their new names; a molecule alone has the bits it has inside the batch."""
    from xequinet_amd.nn import painn
    from xequinet_amd.nn.basic import edge_graph

    model = TP._model(8, node_dim=F)
    assert painn.native_supported(model)
    pos, z, ptr = syn.synth_qm9_batch(8, seed=2)
    data = TP._batch(pos, z, ptr, model.cutoff_radius)
    edge_graph(data).n_rowptr
    TP._compare(model, data, tag=f"widths:qm9_8:F={F}")
    first = lib.launch_count()
    whole = TP._eval(model, data)
    names = lib.launch_names(first)
    print(names)
    assert all(n.startswith("xeq_") for n in names)
    assert sum(n.startswith("xeq_painn_") for n in names) == 3 * (1 + 2) + 3 * (1 + 2) + 2
    # two MLPs per block forward; in reverse the first block's scalar MLP is not differentiated (the embedding needs no gradient)
    assert names.count("xeq_mlp2h_fwd") == 6 and names.count("xeq_mlp2h_bwd") == 5 and not any(n.startswith("xeq_mlp2_") for n in names)
    assert len(names) == TP.LAUNCHES_PER_EVALUATION, len(names)
    for g in (0, 7):
        a0, a1 = int(ptr[g]), int(ptr[g + 1])
        one = TP._eval(model, TP._batch(pos[a0:a1], z[a0:a1], np.array([0, a1 - a0]), model.cutoff_radius))
        assert torch.equal(one["energy"], whole["energy"][g:g + 1]) and torch.equal(one["forces"], whole["forces"][a0:a1]), g


def test_painn_64_periodic_box_with_virial():
    model = TP._model(3, node_dim=64)
    pos, z, ptr, cell = syn.synth_water_box(4, seed=5)
    assert len(z) == 192
    TP._compare(model, TP._batch(pos, z, ptr, model.cutoff_radius, cell=cell), virial=True, tag="widths:water192:F=64")


# ------------------------------------------------------------------------------------------------------------------------ XPaiNN
def _mlps(model):
    return [s for m in model.mods.values() for s in (getattr(m, "scalar_mlp", None), getattr(m, "update_mlp", None)) if s is not None]


@pytest.mark.parametrize("cfg", sorted(XPAINN_CONFIGS))
def test_xpainn_other_widths_against_the_oracle(cfg):
    model, oracle = P._build(torch.float32, **XPAINN_CONFIGS[cfg])
    pos, z, ptr = syn.synth_qm9_batch(8, seed=21)
    ei = orc.radius_graph_canonical(pos.astype(np.float32), ptr, 5.0)
    first = lib.launch_count()
    P._check_model(model, oracle, pos, z, ptr, ei, torch.float32, label=f"widths:xpainn:{cfg}")
    names = lib.launch_names(first)
    mlps = _mlps(model)
    assert len(mlps) == 2 * sum(1 for k in model.mods if k.startswith("message_"))
    assert all(getattr(s, "_xeq_mlp_pack", None) is not None for s in mlps), "an MLP went to the library GEMMs"
    assert "xeq_mlp2h_fwd" in names and "xeq_mlp2h_bwd" in names and not any(n.startswith("xeq_mlp2_") for n in names)


@pytest.mark.parametrize("cfg", sorted(XPAINN_CONFIGS))
def test_xpainn_other_widths_both_fronts_and_replay(cfg):
    """The Python modules and xeq::xpainn_eval: the same launch names in the same order, the same bits; the captured graph replays the
    eager numbers."""
    from xequinet_amd import keys, ops, runtime
    from xequinet_amd.data import NeighborTransform, XequiBatch
    from xequinet_amd.interface.scripted import XPaiNNNative

    model, _ = P._build(torch.float32, **XPAINN_CONFIGS[cfg])
    native = XPaiNNNative(model)
    pos, z, ptr = syn.synth_qm9_batch(24, seed=13)
    data = NeighborTransform(5.0)(XequiBatch(P._t(pos, torch.float32), P._t(z), P._t(ptr))).to_dict()

    def py():
        d = dict(data)
        d[keys.EDGE_GRAPH] = ops.EdgeGraph(data["edge_index"], data["pos"].shape[0], center_sorted=True, ptr=data["ptr"], symmetric=True)
        with torch.enable_grad():
            return model(d, compute_forces=True, compute_virial=False)

    def cc():
        return native(data["pos"].detach(), data["atomic_numbers"], data["edge_index"], data["ptr"], None, None, True, True, True, False)

    py(), cc()
    c0 = lib.launch_count()
    want = py()
    seq_py = lib.launch_names(c0)
    c0 = lib.launch_count()
    got = cc()
    seq_cc = lib.launch_names(c0)
    assert seq_py == seq_cc, "\n".join(f"{a:36s} {b}" for a, b in zip(seq_py + ["-"] * len(seq_cc), seq_cc + ["-"] * len(seq_py)) if a != b)
    n_blocks = sum(1 for k in model.mods if k.startswith("message_"))
    assert seq_py.count("xeq_mlp2h_fwd") >= 2 * n_blocks - 1 and seq_py.count("xeq_mlp2h_bwd") >= 2 * n_blocks - 1, seq_py
    assert torch.equal(got[0], want["energy"].detach()) and torch.equal(got[1], want["atomic_energies"].detach())
    assert torch.equal(got[2], want["forces"].detach()), (got[2] - want["forces"]).abs().max()

    g = runtime.GraphedModel(model, tune_gemms=False)
    with torch.enable_grad():
        eager = model(dict(data), compute_forces=True, compute_virial=False)
    for _ in range(2):
        r = g(dict(data))
        assert torch.equal(r["energy"], eager["energy"]) and torch.equal(r["forces"], eager["forces"])
    assert g.captures == 1
