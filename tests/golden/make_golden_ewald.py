"""Generate the Ewald fixtures by RUNNING THE REFERENCE's ``xequinet.nn.ewald`` under the shims of make_golden.py.  Run once, in the
build container (needs the reference checkout; never on the GPU box):

    python tests/golden/make_golden_ewald.py

Writes data only:
* ewald_f64.npz -- seeded weights of an EwaldBlock(node_dim 32, projection_dim 8), of an EwaldInitialPBC([1, 1, 2]) (K = 22) and of an
  EwaldInitialNonPBC(0.4, 0.2, 20) (K = 13); node scalars, positions of a few Angstrom, triclinic cells, batch / ptr of four graphs
  (1, 2, 29 and 70 atoms); for each initial module ("pbc", "nonpbc") the block's output and the autograd gradients of
  L = sum(out * probe) with respect to the input scalars, the positions and every parameter of the initial module and the block.
* ewald_keys.json -- the reference state-dict names and shapes of the three modules for node_dim 128 and 32, the
  k_index_product_set of [3, 3, 3] (171 rows) and the default non-periodic k_grid and k_rbf_values.
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

from make_golden import _install_shims  # noqa: E402

SIZES = [1, 2, 29, 70]
F = 32


def main():
    _install_shims()
    ew = importlib.import_module("xequinet.nn.ewald")
    torch.set_default_dtype(torch.float64)

    keys_out = {}
    for nd in (128, 32):
        keys_out[str(nd)] = {
            "ewald_block": {k: list(v.shape) for k, v in ew.EwaldBlock(node_dim=nd).state_dict().items()},
            "ewald_initial_pbc": {k: list(v.shape) for k, v in ew.EwaldInitialPBC([3, 3, 3]).state_dict().items()},
            "ewald_initial_nonpbc": {k: list(v.shape) for k, v in ew.EwaldInitialNonPBC(0.4, 0.2, 20).state_dict().items()},
        }
    default_nonpbc = ew.EwaldInitialNonPBC(0.4, 0.2, 20)
    keys_out["k_index_product_set_333"] = ew.EwaldInitialPBC([3, 3, 3]).k_index_product_set.long().tolist()
    keys_out["nonpbc_k_grid"] = default_nonpbc.k_grid.tolist()
    keys_out["nonpbc_k_rbf_values"] = default_nonpbc.k_rbf_values.tolist()
    with open(os.path.join(HERE, "ewald_keys.json"), "w") as f:
        json.dump(keys_out, f, sort_keys=True)

    torch.manual_seed(20261018)
    block = ew.EwaldBlock(node_dim=F, projection_dim=8)
    with torch.no_grad():   # the reference starts up.weight at 0.01 of its initialisation: a filter of order one keeps the Ewald term visible
        block.up.weight *= 100.0
        block.norm.weight.uniform_(0.5, 1.5)
        block.norm.bias.uniform_(-0.5, 0.5)
    inits = {"pbc": ew.EwaldInitialPBC([1, 1, 2], projection_dim=8), "nonpbc": ew.EwaldInitialNonPBC(0.4, 0.2, 20, projection_dim=8)}
    ptr = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
    n = int(ptr[-1])
    batch = np.repeat(np.arange(len(SIZES)), SIZES).astype(np.int64)
    s0 = torch.randn(n, F)
    probe = torch.randn(n, F)
    pos0 = 4.0 * torch.randn(n, 3)
    base = torch.tensor([[9.0, 0.0, 0.0], [1.5, 8.0, 0.0], [-1.0, 2.0, 10.0]])
    cell = torch.stack([base * (1.0 + 0.1 * g) + 0.3 * torch.randn(3, 3) for g in range(len(SIZES))])

    out = {"node_dim": np.array(F), "ptr": ptr, "batch": batch, "s": s0.numpy(), "probe": probe.numpy(), "pos": pos0.numpy(), "cell": cell.numpy()}
    for k, v in block.state_dict().items():
        out[f"w_block_{k}"] = v.numpy()
    for tag, mod in inits.items():
        for k, v in mod.state_dict().items():
            out[f"w_{tag}_{k}"] = v.numpy()

    for tag, init in inits.items():
        s = s0.clone().requires_grad_(True)
        pos = pos0.clone().requires_grad_(True)
        block.zero_grad()
        init.zero_grad()
        data = {"batch": torch.from_numpy(batch), "node_invariant": s, "pos": pos, "cell": cell}
        data = block(init(data))
        y = data["node_invariant"]
        (y * probe).sum().backward()
        out[f"out_{tag}"] = y.detach().numpy()
        out[f"g_{tag}_input"] = s.grad.numpy()
        out[f"g_{tag}_pos"] = pos.grad.numpy()
        for k, p in block.named_parameters():
            out[f"g_{tag}_block_{k}"] = p.grad.numpy().copy()
        for k, p in init.named_parameters():
            out[f"g_{tag}_init_{k}"] = p.grad.numpy().copy()
    np.savez_compressed(os.path.join(HERE, "ewald_f64.npz"), **out)
    print("wrote ewald_f64.npz and ewald_keys.json:", sorted(out))


if __name__ == "__main__":
    main()
