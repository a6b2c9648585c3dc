"""Compare the gfx950 code of two builds, kernel by kernel.

    python profiles/compare_device_isa.py PARENT_OBJDIR CHANGE_OBJDIR [--show NAME]

Each directory holds the host objects of csrc/build.py (xequinet_amd/csrc/build/*.o).  For every object present in both, the device
disassembly (build.device_isa) is split per symbol, addresses and encodings are stripped, and the instruction text is compared.
Prints one line per object (symbols identical / differing / only on one side) and, per differing symbol, the instruction and v_mfma
counts of both sides.  --show prints a unified diff of one symbol (substring match of the mangled name).
"""
import difflib
import os
import re
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from xequinet_amd.csrc.build import device_isa  # noqa: E402

SYMBOL = re.compile(r"^[0-9a-f]+ <(.+)>:$")


def kernels(obj):
    """{symbol: [instruction text, ...]} of one host object"""
    out, cur = {}, None
    for line in device_isa(obj).splitlines():
        m = SYMBOL.match(line.strip())
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None and line.strip() and line.strip() != "...":      # "...": objdump's mark for the zero padding behind a symbol
            cur.append(line.split("//")[0].strip())
    return out


def main(argv):
    show = argv[argv.index("--show") + 1] if "--show" in argv else None
    parent, change = argv[0], argv[1]
    names = sorted(f for f in os.listdir(parent) if f.endswith(".o"))
    missing = sorted(set(f for f in os.listdir(change) if f.endswith(".o")) ^ set(names))
    total_diff = 0
    for name in names:
        if name in missing:
            continue
        a, b = kernels(os.path.join(parent, name)), kernels(os.path.join(change, name))
        same = [k for k in a if k in b and a[k] == b[k]]
        diff = [k for k in a if k in b and a[k] != b[k]]
        only = sorted(set(a) ^ set(b))
        total_diff += len(diff) + len(only)
        print(f"{name}: {len(same)} identical, {len(diff)} differ, {len(only)} on one side only")
        for k in only:
            print(f"    only in {'parent' if k in a else 'change'}: {k}")
        for k in diff:
            na, nb = len(a[k]), len(b[k])
            ma, mb = sum("v_mfma" in i for i in a[k]), sum("v_mfma" in i for i in b[k])
            print(f"    {k}: instructions {na} | {nb}, v_mfma {ma} | {mb}")
            if show and show in k:
                print("\n".join(difflib.unified_diff(a[k], b[k], "parent", "change", lineterm="", n=2)))
    if missing:
        print("objects on one side only:", " ".join(missing))
    print(f"total: {total_diff} symbols differ")
    return 1 if total_diff or missing else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
