"""Time one energy + force evaluation of PaiNN and of XPaiNN (64x0e+32x1o+32x2e; at 256: 256x0e+64x1o+32x2e) on the qm9_1024-shape
batch at node_dim 64 and 256, neighbour list given -- the widths whose two-layer MLPs run xeq_mlp2h_fwd / _bwd.

    python profiles/mlp_widths_timing.py measure <tree> <label>            one tree (a built checkout), one JSON line per point
    python profiles/mlp_widths_timing.py compare <parent tree> <this tree> [rounds]
                                                                           both trees alternately, `rounds` child processes each

Ten warm-up evaluations, then 9 groups of 5 evaluations between device events; `compare` prints per point the median over the rounds
of each tree's group median, and the spread of those medians.  Both trees see the same seeded batch and weights; the energies and
forces of every point are hashed into the line so that the two columns can be compared for what they computed."""
import json
import os
import subprocess
import sys

POINTS = (("painn", 64), ("painn", 256), ("xpainn", 64), ("xpainn", 256))


def _kw(kind, F):
    if kind == "painn":
        return dict(node_dim=F)
    return dict(node_dim=F, node_irreps="64x0e+32x1o+32x2e" if F == 64 else "256x0e+64x1o+32x2e")


def measure(tree, label):
    sys.path.insert(0, os.path.abspath(tree))
    import numpy as np
    import torch

    from xequinet_amd import lib
    from xequinet_amd.data import NeighborTransform, XequiBatch
    from xequinet_amd.data import synthetic as syn
    from xequinet_amd.nn import resolve_model

    assert os.path.abspath(lib.LIB_PATH).startswith(os.path.abspath(tree)), lib.LIB_PATH
    pos, z, ptr = syn.synth_qm9_batch(1024, seed=0)
    batch = XequiBatch(torch.tensor(pos, dtype=torch.float32), torch.tensor(z), torch.tensor(ptr)).to("cuda")
    for kind, F in POINTS:
        torch.manual_seed(0)
        model = resolve_model(kind, **_kw(kind, F)).cuda().eval().requires_grad_(False)
        data = NeighborTransform(model.cutoff_radius)(batch).to_dict()

        def run():
            with torch.enable_grad():
                return model(dict(data), compute_forces=True)

        for _ in range(10):
            out = run()
        torch.cuda.synchronize()
        first = lib.launch_count()
        run()
        names = lib.launch_names(first)
        ms = []
        for _ in range(9):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(5):
                run()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1) / 5)
        print(json.dumps({"label": label, "model": kind, "node_dim": F, "atoms": int(len(z)), "edges": int(data["edge_index"].shape[1]),
                          "ms_median": float(np.median(ms)), "ms_min": float(np.min(ms)), "ms_max": float(np.max(ms)),
                          "library_launches": len(names), "mlp_launches": sum(n.startswith("xeq_mlp2") for n in names),
                          "energy_sum": float(out["energy"].double().sum()), "forces_abs_sum": float(out["forces"].double().abs().sum())}),
              flush=True)


def compare(parent, this, rounds):
    import numpy as np

    rows = {}
    for r in range(rounds):
        for label, tree in (("parent", parent), ("this", this)):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "measure", tree, label], capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                raise SystemExit(f"{label} round {r} failed ({p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
            for line in p.stdout.splitlines():
                if line.startswith("{"):
                    d = json.loads(line)
                    rows.setdefault((d["model"], d["node_dim"]), {}).setdefault(label, []).append(d)
                    print(line, flush=True)
    print(f"ms per evaluation (energy + forces, list given), median [min .. max] over {rounds} processes of the median of 9 groups of 5")
    print(f"{'point':16s} {'parent':>28s} {'this commit':>28s}  ratio  MLP launches (parent -> this)  max |dE_sum| rel, |dF_sum| rel")
    for (kind, F), d in rows.items():
        cell, med = {}, {}
        for label in ("parent", "this"):
            m = [x["ms_median"] for x in d[label]]
            med[label] = float(np.median(m))
            cell[label] = f"{med[label]:8.3f} [{min(m):7.3f} .. {max(m):7.3f}]"
        a, b = d["parent"][0], d["this"][0]
        de = abs(a["energy_sum"] - b["energy_sum"]) / max(abs(a["energy_sum"]), 1e-30)
        df = abs(a["forces_abs_sum"] - b["forces_abs_sum"]) / max(abs(a["forces_abs_sum"]), 1e-30)
        print(f"{kind + ' F=' + str(F):16s} {cell['parent']:>28s} {cell['this']:>28s}  {med['this'] / med['parent']:5.3f}  "
              f"{a['mlp_launches']:3d} -> {b['mlp_launches']:3d} of {a['library_launches']} -> {b['library_launches']} library launches"
              f"   {de:.1e}, {df:.1e}")


if __name__ == "__main__":
    if len(sys.argv) >= 4 and sys.argv[1] == "measure":
        measure(sys.argv[2], sys.argv[3])
    elif len(sys.argv) >= 4 and sys.argv[1] == "compare":
        compare(sys.argv[2], sys.argv[3], int(sys.argv[4]) if len(sys.argv) > 4 else 3)
    else:
        raise SystemExit(__doc__)
