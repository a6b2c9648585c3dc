"""Generate the PaiNN model fixture by RUNNING THE REFERENCE's nn/painn.py in the build container (never on the GPU box):

    python tests/golden/make_golden_painn.py

Same container-only shims as make_golden.py.  Embedding + 3 x (PainnMessage, PainnUpdate) at node_dim 128, 20 Bessel functions,
cutoff 5.0, float64, on (a) a small QM9-shape batch that ends with a single-atom graph and (b) a small periodic water box.  The
parameters are overwritten with ``tests/painn_oracle.py::seeded_weights`` so the fixture stores the seed, not the weights; the energy
is a linear readout of the last node scalars (the reference's EnergyOut imports e3nn).  Writes painn_model_f64.npz and
painn_keys.json (state-dict names and shapes of the reference modules).
"""
import importlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "..", ".."))
import make_golden as mg  # noqa: E402
from oracle import xpainn_oracle as orc  # noqa: E402
from tests import painn_oracle as po  # noqa: E402
from xequinet_amd.data import synthetic as syn  # noqa: E402

SEED, F_, NB, RC, BLOCKS = 20250, 128, 20, 5.0, 3


def main():
    mg._install_shims()
    basic = importlib.import_module("xequinet.nn.basic")
    painn = importlib.import_module("xequinet.nn.painn")
    rg = mg._by_path("ref_radius_graph", f"{mg.REF}/xequinet/data/radius_graph.py")
    keys = importlib.import_module("xequinet.keys")
    torch.set_default_dtype(torch.float64)

    mods = {"embedding": painn.Embedding(node_dim=F_, num_basis=NB, embed_basis="gfn2-xtb", aux_basis="aux56", cutoff=RC)}
    for i in range(BLOCKS):
        mods[f"message_{i}"] = painn.PainnMessage(F_, NB)
        mods[f"update_{i}"] = painn.PainnUpdate(F_)
    shapes = {f"{n}.{k}": list(v.shape) for n, m in mods.items() for k, v in m.state_dict().items()}
    # the one-hot table of the other embedding form, for the key check only
    shapes_onehot = {f"embedding.{k}": list(v.shape) for k, v in painn.Embedding(node_dim=F_, num_basis=NB, embed_basis="one-hot", cutoff=RC).state_dict().items()}
    with open(os.path.join(HERE, "painn_keys.json"), "w") as f:
        json.dump({"gfn2-xtb": shapes, "one-hot-embedding": shapes_onehot}, f, indent=1, sort_keys=True)
    w = po.seeded_weights(shapes, SEED)
    for n, m in mods.items():
        m.load_state_dict({k[len(n) + 1:]: v for k, v in w.items() if k.startswith(n + ".")}, strict=False)
    w_out = torch.tensor(np.random.default_rng(SEED + 1).standard_normal(F_) / np.sqrt(F_))

    def run(data, n_graphs, virial):
        data = basic.compute_edge_data(data, compute_forces=True, compute_virial=virial)
        data = mods["embedding"](data)
        s_blocks = []
        for i in range(BLOCKS):
            data = mods[f"update_{i}"](mods[f"message_{i}"](data))
            s_blocks.append(data[keys.NODE_INVARIANT].detach().numpy())
        energy = torch.zeros(n_graphs).index_add(0, data[keys.BATCH], data[keys.NODE_INVARIANT] @ w_out)
        data[keys.TOTAL_ENERGY] = energy
        res = basic.compute_properties(data, compute_forces=True, compute_virial=virial, training=False)
        out = {"s_blocks": np.stack(s_blocks), "x_last": data[keys.NODE_EQUIVARIANT].detach().numpy(),
               "energy": energy.detach().numpy(), "forces": res[keys.FORCES].detach().numpy()}
        if virial:
            out["virial"] = res[keys.VIRIAL].detach().numpy()
        return out

    # (a) two QM9-shape molecules and one single-atom graph (an atom without an edge)
    pos, z, ptr = syn.synth_qm9_batch(2, seed=41)
    pos = np.concatenate([pos, [[30.0, 30.0, 30.0]]])
    z = np.concatenate([z, [8]])
    ptr = np.concatenate([ptr, [len(z)]])
    ei = orc.radius_graph_canonical(pos.astype(np.float32), ptr, RC)
    d = np.linalg.norm(pos[ei[0]] - pos[ei[1]], axis=-1)
    dall = np.linalg.norm(pos[:, None] - pos[None], axis=-1)
    assert np.all(np.abs(dall - RC) > 1e-4) and d.max() < RC
    batch = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
    data = {keys.POSITIONS: torch.tensor(pos), keys.ATOMIC_NUMBERS: torch.tensor(z.astype(np.int64)), keys.EDGE_INDEX: torch.tensor(ei),
            keys.BATCH: torch.tensor(batch), keys.BATCH_PTR: torch.tensor(ptr)}
    mol = run(data, len(ptr) - 1, False)
    out = {"mol_pos": pos, "mol_z": z, "mol_ptr": ptr, "mol_edge_index": ei, **{"mol_" + k: v for k, v in mol.items()}}

    # (b) a 24-atom periodic water box, the reference's own neighbour list
    bpos, bz, bptr, cell = syn.synth_water_box(2, seed=11)
    ei_b, co_b = rg.radius_graph_pbc(pos=torch.tensor(bpos, dtype=torch.float32), n_nodes_per_graph=torch.tensor([len(bz)]),
                                     pbc=torch.tensor([[True, True, True]]), cell=torch.tensor(cell, dtype=torch.float32), cutoff=RC)
    ei_wide, _ = rg.radius_graph_pbc(pos=torch.tensor(bpos, dtype=torch.float32), n_nodes_per_graph=torch.tensor([len(bz)]),
                                     pbc=torch.tensor([[True, True, True]]), cell=torch.tensor(cell, dtype=torch.float32), cutoff=RC + 2e-4)
    ei_narrow, _ = rg.radius_graph_pbc(pos=torch.tensor(bpos, dtype=torch.float32), n_nodes_per_graph=torch.tensor([len(bz)]),
                                       pbc=torch.tensor([[True, True, True]]), cell=torch.tensor(cell, dtype=torch.float32), cutoff=RC - 2e-4)
    assert ei_wide.shape == ei_b.shape == ei_narrow.shape, "a pair sits within 2e-4 of the cutoff"
    data = {keys.POSITIONS: torch.tensor(bpos), keys.ATOMIC_NUMBERS: torch.tensor(bz.astype(np.int64)), keys.EDGE_INDEX: ei_b,
            keys.CELL: torch.tensor(cell), keys.CELL_OFFSETS: co_b.to(torch.float64), keys.BATCH: torch.zeros(len(bz), dtype=torch.long),
            keys.BATCH_PTR: torch.tensor([0, len(bz)])}
    box = run(data, 1, True)
    out.update({"box_pos": bpos, "box_z": bz, "box_cell": cell, "box_edge_index": ei_b.numpy(), "box_cell_offsets": co_b.numpy().astype(np.int8),
                **{"box_" + k: v for k, v in box.items()}})
    np.savez_compressed(os.path.join(HERE, "painn_model_f64.npz"), seed=SEED, node_dim=F_, num_basis=NB, cutoff=RC, blocks=BLOCKS,
                        w_out=w_out.numpy(), **out)
    print("mol energy", mol["energy"], "box energy", box["energy"], "edges", ei.shape[1], ei_b.shape[1],
          "bytes", os.path.getsize(os.path.join(HERE, "painn_model_f64.npz")))


if __name__ == "__main__":
    main()
