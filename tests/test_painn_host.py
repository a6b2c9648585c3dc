"""PaiNN on the host: the restated oracle (tests/painn_oracle.py) against the reference's own numbers (painn_twin_f64.npz,
painn_model_f64.npz), the model factory, the reference's state-dict names and shapes (painn_keys.json), and the tensor form of
xequinet_amd/nn/painn.py in f64 on the CPU against the oracle."""
import json
import os

import numpy as np
import torch

from tests import painn_oracle as po

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def _fixture():
    f = np.load(os.path.join(GOLDEN, "painn_model_f64.npz"))
    shapes = json.load(open(os.path.join(GOLDEN, "painn_keys.json")))["gfn2-xtb"]
    p = po.seeded_weights(shapes, int(f["seed"]))
    return f, shapes, p


def _f64_model(**kw):
    """A PaiNN model built under a float64 default dtype (element table and Bessel frequencies in full precision, as the fixture's)."""
    from xequinet_amd.nn.model import resolve_model

    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        return resolve_model("painn", **kw)
    finally:
        torch.set_default_dtype(old)


def _reference_buffers(p):
    """The non-weight entries of the reference's state dict (element table, Bessel frequencies) from a model of this package."""
    m = _f64_model()
    sd = {k[len("mods."):]: v for k, v in m.state_dict().items()}
    return {**{k: v for k, v in sd.items() if k not in p and not k.startswith("output_")}, **p}


def _mol_inputs(f):
    ptr = f["mol_ptr"]
    batch = torch.tensor(np.repeat(np.arange(len(ptr) - 1), np.diff(ptr)))
    return torch.tensor(f["mol_z"]).long(), torch.tensor(f["mol_pos"]), torch.tensor(f["mol_edge_index"]), batch, len(ptr) - 1


def test_oracle_reproduces_the_twin_fixture():
    f = np.load(os.path.join(GOLDEN, "painn_twin_f64.npz"))
    p = {k.replace("emb.", "embedding.", 1) if k.startswith("emb.") else k: torch.tensor(f[k]) for k in f.files if "." in k}
    ptr = f["ptr"]
    batch = torch.tensor(np.repeat(np.arange(len(ptr) - 1), np.diff(ptr)))
    pos = torch.tensor(f["pos"], requires_grad=True)
    ei = torch.tensor(f["edge_index"])
    s, x = po.blocks(torch.tensor(f["z"]).long(), po.edge_vectors(pos, ei), ei, p, 2, float(f["cutoff"]))
    energy = torch.zeros(len(ptr) - 1, dtype=torch.float64).index_add(0, batch, s @ torch.tensor(f["w_out"]))
    (g,) = torch.autograd.grad([energy], [pos], [torch.ones_like(energy)])
    assert _rel(s.detach(), f["node_invariant"]) <= 1e-10
    assert _rel(x.detach(), f["node_equivariant"]) <= 1e-10
    assert _rel(energy.detach(), f["energy"]) <= 1e-10
    assert _rel(-g, f["forces"]) <= 1e-10


def test_oracle_reproduces_the_model_fixture():
    f, _, p = _fixture()
    p = _reference_buffers(p)
    z, pos, ei, batch, ng = _mol_inputs(f)
    w_out = torch.tensor(f["w_out"])
    s_blocks = []
    s, x = po.blocks(z, po.edge_vectors(pos, ei), ei, p, int(f["blocks"]), float(f["cutoff"]), collect=s_blocks)
    assert _rel(torch.stack(s_blocks), f["mol_s_blocks"]) <= 1e-10
    assert _rel(x, f["mol_x_last"]) <= 1e-10
    assert float(x[-1].abs().max()) == 0.0   # the single-atom graph: no edge, no vector features
    out = po.model(p, z, pos, ei, batch, ng, int(f["blocks"]), float(f["cutoff"]), w_out=w_out)
    assert _rel(out["energy"].detach(), f["mol_energy"]) <= 1e-10
    assert _rel(out["forces"], f["mol_forces"]) <= 1e-10
    nb = len(f["box_z"])
    box = po.model(p, torch.tensor(f["box_z"]).long(), torch.tensor(f["box_pos"]), torch.tensor(f["box_edge_index"]),
                   torch.zeros(nb, dtype=torch.long), 1, int(f["blocks"]), float(f["cutoff"]), cell=torch.tensor(f["box_cell"]),
                   cell_offsets=torch.tensor(f["box_cell_offsets"]).double(), virial=True, w_out=w_out)
    assert _rel(box["energy"].detach(), f["box_energy"]) <= 1e-10
    assert _rel(box["forces"], f["box_forces"]) <= 1e-10
    assert _rel(box["virial"], f["box_virial"]) <= 1e-10


def test_factory_builds_painn_with_the_reference_state_dict_layout():
    from xequinet_amd.nn.model import PaiNN, resolve_model

    model = resolve_model("painn")
    assert isinstance(model, PaiNN)
    keys_json = json.load(open(os.path.join(GOLDEN, "painn_keys.json")))
    own = {k[len("mods."):]: list(v.shape) for k, v in model.state_dict().items() if k.startswith("mods.") and not k.startswith("mods.output_")}
    assert own == keys_json["gfn2-xtb"]
    onehot = resolve_model("painn", embed_basis="one-hot")
    own = {k[len("mods."):]: list(v.shape) for k, v in onehot.state_dict().items() if k.startswith("mods.embedding.")}
    assert own == keys_json["one-hot-embedding"]
    assert float(onehot.mods["embedding"].embedding.weight[0].abs().max()) == 0.0   # padding_idx = 0
    assert model.mods["update_2"].equivariant_output_unused and not model.mods["update_1"].equivariant_output_unused


def test_load_reference_state_dict_round_trips():
    from xequinet_amd.nn.model import resolve_model

    _, _, p = _fixture()
    a = _f64_model()
    sd = a.state_dict()
    sd.update({"mods." + k: v for k, v in p.items()})
    b = _f64_model()
    b.load_reference_state_dict(sd)
    for k, v in b.state_dict().items():
        assert torch.equal(v, sd[k]), k
    try:
        b.load_reference_state_dict({**sd, "mods.message_0.no_such.weight": torch.zeros(1)})
    except KeyError:
        pass
    else:
        raise AssertionError("an unknown key must be refused")


def test_tensor_form_f64_on_cpu_matches_the_oracle():
    from xequinet_amd.nn.model import resolve_model

    f, _, p = _fixture()
    model = _f64_model().eval().requires_grad_(False)
    sd = model.state_dict()
    sd.update({"mods." + k: v for k, v in p.items()})
    model.load_reference_state_dict(sd)
    z, pos, ei, batch, ng = _mol_inputs(f)
    data = {"pos": pos.clone(), "atomic_numbers": z, "edge_index": ei, "batch": batch, "ptr": torch.tensor(f["mol_ptr"])}
    seen = {}
    model.mods["update_1"].register_forward_hook(lambda mod, inp, out: seen.update(x=out["node_equivariant"], s=out["node_invariant"]))
    got = model(data, compute_forces=True)
    ref = po.model(model.state_dict(), z, pos, ei, batch, ng, 3, 5.0)
    assert _rel(got["energy"].detach(), ref["energy"].detach()) <= 1e-10
    assert _rel(got["forces"], ref["forces"]) <= 1e-10
    assert torch.isfinite(got["forces"]).all() and float(got["forces"][-1].abs().max()) == 0.0   # the single atom: zero, not NaN
    assert seen["x"].shape == (len(z), 3, 128)   # Cartesian [N, 3, F]
    assert _rel(seen["s"].detach(), f["mol_s_blocks"][1]) <= 1e-10
    # the periodic box with the virial
    nb = len(f["box_z"])
    data = {"pos": torch.tensor(f["box_pos"]), "atomic_numbers": torch.tensor(f["box_z"]).long(), "edge_index": torch.tensor(f["box_edge_index"]),
            "batch": torch.zeros(nb, dtype=torch.long), "ptr": torch.tensor([0, nb]), "cell": torch.tensor(f["box_cell"]),
            "cell_offsets": torch.tensor(f["box_cell_offsets"]).double()}
    got = model(data, compute_forces=True, compute_virial=True)
    ref = po.model(model.state_dict(), data["atomic_numbers"], torch.tensor(f["box_pos"]), data["edge_index"], data["batch"], 1, 3, 5.0,
                   cell=data["cell"], cell_offsets=data["cell_offsets"], virial=True)
    assert _rel(got["forces"], ref["forces"]) <= 1e-10 and _rel(got["virial"], ref["virial"]) <= 1e-10


def test_training_pass_is_twice_differentiable_on_cpu():
    """train() with parameters asking for gradients: a force loss backpropagates to the parameters (f64 tensor form against oracle autograd)."""
    from xequinet_amd.nn.model import resolve_model

    f, _, p = _fixture()
    model = _f64_model().train()
    sd = model.state_dict()
    sd.update({"mods." + k: v for k, v in p.items()})
    model.load_reference_state_dict(sd)
    z, pos, ei, batch, ng = _mol_inputs(f)
    data = {"pos": pos.clone(), "atomic_numbers": z, "edge_index": ei, "batch": batch, "ptr": torch.tensor(f["mol_ptr"])}
    out = model(data, compute_forces=True)
    loss = out["energy"].sum() + (out["forces"] ** 2).sum()
    names = [k for k, v in model.named_parameters() if "rbf.freq" not in k]
    grads = torch.autograd.grad(loss, [dict(model.named_parameters())[k] for k in names])
    q = {k: v.detach().clone().requires_grad_(v.is_floating_point()) for k, v in model.state_dict().items()}
    assert all(torch.isfinite(g).all() for g in grads)   # the single-atom graph included (|V| = 0 there)
    # the oracle keeps torch.linalg.norm, whose second derivative at V = 0 is 0 / 0: compare on the two molecules
    n = int(f["mol_ptr"][2])
    keep = (ei[0] < n) & (ei[1] < n)
    z, pos, ei, batch, ng = z[:n], pos[:n], ei[:, keep], batch[:n], 2
    data = {"pos": pos.clone(), "atomic_numbers": z, "edge_index": ei, "batch": batch, "ptr": torch.tensor(f["mol_ptr"][:3])}
    out = model(data, compute_forces=True)
    grads = torch.autograd.grad(out["energy"].sum() + (out["forces"] ** 2).sum(), [dict(model.named_parameters())[k] for k in names])
    ref = po.model(q, z, pos, ei, batch, ng, 3, 5.0, create_graph=True)
    ref_grads = torch.autograd.grad(ref["energy"].sum() + (ref["forces"] ** 2).sum(), [q[k] for k in names])
    for k, g, r in zip(names, grads, ref_grads):
        assert float((g - r).abs().max()) <= 1e-8 * max(1.0, float(r.abs().max())), k
