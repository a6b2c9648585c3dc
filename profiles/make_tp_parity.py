"""profiles/tp_parity.txt from the output of ``python -m pytest tests/test_gpu_tp.py -m gpu -s`` (its ``tp-parity`` lines):
    python profiles/make_tp_parity.py LOG > profiles/tp_parity.txt
One row per (case, precision, output); the 25 (channels, rows) cases of a tied-form sweep are one row per channel count, the worst over the
row counts.  Then the worst kernel/bound and the worst kernel/oracle32 per precision and output."""
import re
import sys

LINE = re.compile(r"tp-parity (\S+) (f\d\d) (\S+) (\S+): kernel (\S+) oracle32 (\S+) kernel/oracle32 \S+ largest (\S+) bound (\S+) kernel/bound (\S+)")
HEAD = """Measured errors of the general tensor-product kernels (csrc/xeq_tp.hip: k_tp_path, k_tp_fused, k_tp_tied, k_tp_wgrad behind
tp.TensorProduct) against oracle/tp_oracle.py in f64 (MI355X, gfx950), every case of tests/tp_cases.py in f64 and f32.
Source: the `tp-parity` lines of `python -m pytest tests/test_gpu_tp.py -m gpu -s`, tabulated by profiles/make_tp_parity.py.
forms: the form of the forward pass / the pass that writes dL/dx1 / the one that writes dL/dx2, as xeq_tensor_product_form states it
(tied: k_tp_tied, a wave per node; tileN: k_tp_fused on N nodes per workgroup; path: one k_tp_path launch per instruction); dL/dW is
k_tp_wgrad wherever a fused table exists (every case but limit-41-paths).
kernel = max |kernel - f64 oracle|, oracle32 = max |f32 oracle - f64 oracle| on the same inputs;
bound: f64 1e-12 (out) / 1e-11 (gradients) of the largest entry, f32 max(4 oracle32, 4 ulp of the largest entry).
"""


def main(path):
    rows, order = {}, []
    for line in open(path):
        for m in LINE.finditer(line):
            name, prec, forms, out, kernel, o32, top, bound, ratio = m.groups()
            sweep = re.fullmatch(r"((?:uuu|uuw|uvu|uvv)-.*-m\d+)-n\d+", name)
            key = ((sweep.group(1) + "-n*") if sweep else name, prec, forms, out)
            rec = (float(ratio), float(kernel), float(o32), float(top), float(bound), name)
            if key not in rows:
                order.append(key)
            if key not in rows or rec[0] > rows[key][0]:
                rows[key] = rec
    print(HEAD)
    worst, worst32, n = {}, {}, 0
    print(f"# {'case':<34} prec {'forms':<20} {'output':<8} {'kernel/bound':>12} {'kernel':>10} {'oracle32':>10} {'k/o32':>6} {'largest':>10} {'bound':>10}")
    for key in order:
        ratio, kernel, o32, top, bound, name = rows[key]
        case, prec, forms, out = key
        n += 1
        print(f"  {case:<34} {prec}  {forms:<20} {out:<8} {ratio:>12.3f} {kernel:>10.3e} {o32:>10.3e} {kernel / max(o32, 1e-300):>6.2f} {top:>10.3e} {bound:>10.3e}")
        if ratio > worst.get((prec, out), (-1,))[0]:
            worst[(prec, out)] = (ratio, name, forms)
        if prec == "f32" and kernel / max(o32, 1e-300) > worst32.get(out, (-1,))[0]:
            worst32[out] = (kernel / max(o32, 1e-300), name, forms, kernel, 4 * 2.0 ** -23 * top)
    print(f"\n# {n} rows; worst kernel/bound per precision and output")
    for (prec, out), (ratio, name, forms) in sorted(worst.items()):
        print(f"  {prec} {out:<8} {ratio:.3f}  ({name}, {forms})")
    print("\n# f32: worst kernel/oracle32 per output (where it exceeds 4 the kernel's error is below the floor of 4 ulp of the largest entry)")
    for out, (r, name, forms, kernel, floor) in sorted(worst32.items()):
        print(f"  {out:<8} {r:.2f}  kernel {kernel:.3e}  4 ulp floor {floor:.3e}  ({name}, {forms})")
    top = max(v[0] for k, v in worst.items() if k[0] == "f32")
    print(f"\nNo output needed more than the 4 x rule: the largest kernel/bound in f32 is {top:.3f}." if top <= 1 else "\nSOME OUTPUT LEFT ITS BOUND.")


if __name__ == "__main__":
    main(sys.argv[1])
