"""Generate the charge / spin embedding fixtures by RUNNING THE REFERENCE's ``xequinet.nn.electronic`` (e3nn-free) under the
shims of make_golden.py.  Run once, in the build container (needs the reference checkout; never on the GPU box):

    python tests/golden/make_golden_electronic.py

Writes data only:
* electronic_f64.npz -- seeded weights of a ChargeEmbedding and a SpinEmbedding (node_dim 32), node scalars, batch / ptr of five
  graphs (1, 2, 29, 100 and 1 atoms), charges {-3, -1, 0, +1, +2}, spins {0, 1, 2, 4, 1}, the outputs of the charge module, of
  the spin module and of both in sequence (charge first), and for each of the three the autograd gradients of
  L = sum(out * probe) with respect to every parameter and the input scalars.
* electronic_keys.json -- the reference state-dict names and shapes of both modules for node_dim 128 and 16.

The reference's SpinEmbedding applies Linear(1, F) to the spin tensor as given, so the spins are handed to it as [G, 1]
(a [G] tensor only works for one graph); the charge goes in as [G].
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

SIZES = [1, 2, 29, 100, 1]
CHARGES = [-3, -1, 0, 1, 2]
SPINS = [0, 1, 2, 4, 1]
F = 32


def main():
    _install_shims()
    el = importlib.import_module("xequinet.nn.electronic")
    torch.set_default_dtype(torch.float64)

    keys_out = {}
    for nd in (128, 16):
        keys_out[str(nd)] = {
            "charge_embedding": {k: list(v.shape) for k, v in el.ChargeEmbedding(node_dim=nd).state_dict().items()},
            "spin_embedding": {k: list(v.shape) for k, v in el.SpinEmbedding(node_dim=nd).state_dict().items()},
        }
    with open(os.path.join(HERE, "electronic_keys.json"), "w") as f:
        json.dump(keys_out, f, indent=1, sort_keys=True)

    torch.manual_seed(20261016)
    charge_mod = el.ChargeEmbedding(node_dim=F)
    spin_mod = el.SpinEmbedding(node_dim=F)
    ptr = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
    n = int(ptr[-1])
    batch = np.repeat(np.arange(len(SIZES)), SIZES).astype(np.int64)
    s0 = torch.randn(n, F)
    probe = torch.randn(n, F)
    charge = torch.tensor(CHARGES, dtype=torch.int64)
    spin = torch.tensor(SPINS, dtype=torch.int64)

    out = {"node_dim": np.array(F), "ptr": ptr, "batch": batch, "charge": charge.numpy(), "spin": spin.numpy(),
           "s": s0.numpy(), "probe": probe.numpy()}
    for tag, mod in (("c", charge_mod), ("s", spin_mod)):
        for k, v in mod.state_dict().items():
            out[f"w_{tag}_{k}"] = v.numpy()

    def run(mods, case):
        s = s0.clone().requires_grad_(True)
        data = {"batch": torch.from_numpy(batch), "node_invariant": s, "charge": charge, "spin": spin.view(-1, 1)}
        for m in mods:
            m.zero_grad()
            data = m(data)
        y = data["node_invariant"]
        (y * probe).sum().backward()
        out[f"out_{case}"] = y.detach().numpy()
        out[f"g_{case}_input"] = s.grad.numpy()
        for tag, m in (("c", charge_mod), ("s", spin_mod)):
            if m in mods:
                for k, p in m.named_parameters():
                    out[f"g_{case}_{tag}_{k}"] = p.grad.numpy().copy()

    run([charge_mod], "charge")
    run([spin_mod], "spin")
    run([charge_mod, spin_mod], "both")
    np.savez_compressed(os.path.join(HERE, "electronic_f64.npz"), **out)
    print("wrote electronic_f64.npz and electronic_keys.json:", sorted(out))


if __name__ == "__main__":
    main()
