"""Writes profiles/lattice_lists.txt: per lattice case of tests/lattice_cases.py the atoms, edges, image counts, bins and ties per
atom (CPU), and for the FCC shell on the cutoff what tests/test_gpu_lattice_lists.py::fcc_evaluate measures on the GPU -- missing
mirrors, list differences against f64, the f32 oracle's own errors and the bounds that follow from them.

    python profiles/lattice_lists.py [output file]        (the model part of the FCC case needs the MI355X)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(path):
    from tests import lattice_cases as lc
    from tests.test_lattice_cases_host import bins_of

    lines = ["case                 atoms   edges  rep        bins                                     on the cutoff per atom"]
    for c in lc.all_cases():
        ei, _, ties = lc.exact(c.name)
        reps, nb = bins_of(c) if c.periodic else ("-", None)
        bins = "-" if nb is None else " ".join("x".join(str(v) for v in row) for row in nb.tolist())
        lines.append(f"{c.name:20s} {c.n_atoms:5d} {ei.shape[1]:7d}  {str(reps):10s} {bins:40s} {ties / max(c.n_atoms, 1):6.2f}  {c.note}")
    lines.append("")
    lines.append("FCC, a = f32(5 / sqrt 2) moved by `variant` f32 ulps, 3 x 3 x 3 cells (108 atoms), cutoff 5.0, f32 list and default f32 model")
    lines.append("against the f64 oracle on its own f64 list (same f32 numbers); `displaced`: every atom moved by 0.05 A")
    import torch

    from tests.test_lattice_cases_host import _fcc_lists

    for variant in lc.FCC_VARIANTS:
        for displaced in (False, True):
            n32, n64, diff, missing = _fcc_lists(variant, displaced)
            lines.append("")
            lines.append(f"  variant {variant:+d} ulp, displaced {displaced}: CPU oracles: f32 list {n32} edges, f64 list {n64}, {diff} differ, "
                         f"{missing} of the f32 list without a mirror")
            if not torch.cuda.is_available():
                lines.append("  (no GPU here: the model part was not measured)")
                continue
            from tests.test_gpu_lattice_lists import fcc_evaluate

            for k, v in fcc_evaluate(variant, displaced).items():
                lines.append(f"  {k:24s} {v:.6e}" if isinstance(v, float) else f"  {k:24s} {v}")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "lattice_lists.txt"))
