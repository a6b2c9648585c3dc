"""The record behind "L-BFGS joined the resident drivers' shared records, box, wrap and checks and nothing moved"
(profiles/resident_shared_refactor.txt): every resident driver under the PARENT commit's package with the parent's libraries, then under
this tree's package with its own, in child processes of their own on one MI355X in one session, each under its own time limit; a process
starts only if the one before it ended cleanly.

    python profiles/resident_shared_refactor.py --resources PARENT_OBJDIR CHANGE_OBJDIR
        (no GPU) per kernel of xeq_md.o and xeq_lbfgs.o whose instructions differ (profiles/compare_device_isa.py): VGPRs, SGPRs, scratch
        and LDS from the code objects' metadata and the multiset of floating-point instructions (mnemonics containing _f32 / _f64).
    python profiles/resident_shared_refactor.py --parent DIR --out FILE [--rounds 3] [--bench-repeats 1]
        DIR holds the parent commit's built ``xequinet_amd/`` (Python files AND libxeq_hip.so / libxeq_torch.so) and its ``bench.py``.
        --rounds: processes per side, the sides taken in turn, their blocks pooled (two processes of one build differ by 1 to 5 %:
        profiles/neighbor_search_refactor.txt).  Exit status 1 unless every digest and launch sequence agrees and every median of the
        branch lies inside the parent's min .. max.
    python profiles/resident_shared_refactor.py --record FILE.json
        (what the driver starts, once per side and round) whichever package sys.path finds first.

Systems: aspirin (21 atoms, open: one chunk, one launch per L-BFGS entry) and a 375-atom water box (periodic: two chunks, two launches
per L-BFGS entry); the default XPaiNN with fresh weights (seed 0), f32 and f64.  Forms: optimize.LBFGS with memory 4 and 32 and
optimize.FIRE on both systems (fmax 1e-7: every graph stays active); md.Dynamics nve and langevin on the molecule, npt_berendsen on the box.
Recorded per form: SHA-256 of every tensor of ``_state()`` and of the trajectory behind 40 iterations with the recorder on every 5; the
library's launch names from the driver's construction to there (lib.launch_names); ms per iteration of the resident run (device events
around RESIDENT_STEPS iterations, RESIDENT_BLOCKS blocks) and of the driver's two entries alone, without the step's graph between them
(ALONE_STEPS iterations, ALONE_BLOCKS blocks; the state this leaves is discarded).  The margin is measured, not chosen: the branch's
median has to lie inside the parent's own pooled min .. max.
"""
import argparse
import hashlib
import json
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile
from collections import Counter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.abspath(__file__)
DEV = "cuda"
ITERATIONS, RECORD_EVERY = 40, 5
RESIDENT_STEPS, RESIDENT_BLOCKS, ALONE_STEPS, ALONE_BLOCKS = 100, 3, 200, 5
RECORD_TIMEOUT, BENCH_TIMEOUT = 540, 300
MASS = {1: 1.008, 6: 12.011, 7: 14.007, 8: 15.999, 9: 18.998}
ENTRIES = {f"xeq_{d}_{half}" for d in ("md", "npt", "fire", "lbfgs") for half in ("front", "back")}
DIFFERING = ("k_fire_back", "k_lbfgs_back_chunk", "k_lbfgs_back_fused")      # the kernels whose box is a kernel argument by value: the ones a shared position store can change


# ---------------------------------------------------------------------------------------------------------------- no GPU: --resources
def resources(parent, change):
    sys.path.insert(0, ROOT)
    from profiles.compare_device_isa import kernels
    from xequinet_amd.csrc.build import LLVM_BIN

    def metadata(obj):
        with tempfile.TemporaryDirectory() as tmp:
            local = os.path.join(tmp, os.path.basename(obj))
            shutil.copy(obj, local)
            subprocess.run([os.path.join(LLVM_BIN, "llvm-objdump"), "--offloading", local], check=True, capture_output=True)
            part = [f for f in os.listdir(tmp) if "gfx950" in f][0]
            text = subprocess.run([os.path.join(LLVM_BIN, "llvm-readelf"), "--notes", os.path.join(tmp, part)], check=True, capture_output=True, text=True).stdout
        out = {}
        for block in text.split("- .agpr_count")[1:]:
            get = lambda k: re.search(r"\." + k + r":\s*(\S+)", block).group(1)
            out[get("name")] = " ".join(f"{k} {get(k)}" for k in ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size"))
        return out

    floating = lambda ins: Counter(i.split()[0] for i in ins if "_f32" in i.split()[0] or "_f64" in i.split()[0])
    worse = False
    for name in ("xeq_md.o", "xeq_lbfgs.o"):
        a, b = kernels(os.path.join(parent, name)), kernels(os.path.join(change, name))
        ma, mb = metadata(os.path.join(parent, name)), metadata(os.path.join(change, name))
        for k in a:
            if a[k] == b[k] and not any(d in k for d in DIFFERING):
                continue
            fa, fb = floating(a[k]), floating(b[k])
            print(f"{k}: instructions {'identical' if a[k] == b[k] else 'differ'} ({len(a[k])} | {len(b[k])})\n    parent {ma[k]}   floating-point instructions "
                  f"{sum(fa.values())}\n    change {mb[k]}   floating-point instructions {sum(fb.values())}   multiset equal: {fa == fb}")
            worse |= fa != fb or ma[k] != mb[k]
    return 1 if worse else 0


# ---------------------------------------------------------------------------------------------------------------- one side: --record
def record(path):
    import numpy as np
    import torch

    import xequinet_amd
    from xequinet_amd import lib, md, optimize
    from xequinet_amd.data import synthetic as syn
    from xequinet_amd.nn import resolve_model

    t = lambda a, dt=None: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).to(DEV)
    a_pos, a_z, a_ptr = syn.synth_aspirin()
    w_pos, w_z, _, w_cell = syn.synth_water_box(5, seed=5)
    assert len(a_pos) <= 256 < len(w_pos) <= 512
    systems = {"aspirin": (a_pos, a_z, dict(ptr=t(a_ptr))), "water box 375": (w_pos, w_z, dict(cell=np.asarray(w_cell).reshape(3, 3)))}
    units = dict(energy_unit="eV", length_unit="Angstrom")
    forms = {}
    for dname, dtype in (("f32", torch.float32), ("f64", torch.float64)):
        torch.manual_seed(0)
        model = resolve_model("xpainn").to(DEV).to(dtype).eval().requires_grad_(False)
        for sname, (pos, z, where) in systems.items():
            where = {k: t(v, dtype) if k == "cell" else v for k, v in where.items()}
            common = (model, t(pos, dtype), t(z))
            for memory in (4, 32):
                forms[f"LBFGS memory {memory}, {sname}, {dname}"] = lambda c=common, w=where, m=memory: optimize.LBFGS(*c, fmax=1e-7, memory=m, **w, **units)
            forms[f"FIRE, {sname}, {dname}"] = lambda c=common, w=where: optimize.FIRE(*c, fmax=1e-7, **w, **units)
            mass = torch.tensor([MASS[int(a)] for a in z], dtype=torch.float64, device=DEV)
            if "ptr" in where:
                forms[f"Dynamics nve, {sname}, {dname}"] = lambda c=common, w=where, m=mass: md.Dynamics(*c, m, timestep_fs=0.1, ensemble="nve", **w, **units)
                forms[f"Dynamics langevin, {sname}, {dname}"] = lambda c=common, w=where, m=mass: md.Dynamics(
                    *c, m, timestep_fs=0.1, ensemble="langevin", temperature_K=300.0, friction_per_fs=0.01, seed=7, **w, **units)
            else:
                forms[f"Dynamics npt_berendsen, {sname}, {dname}"] = lambda c=common, w=where, m=mass: md.Dynamics(
                    *c, m, timestep_fs=0.1, ensemble="npt_berendsen", temperature_K=300.0, taut_fs=100.0, pressure_GPa=0.0, taup_fs=1000.0,
                    compressibility_per_GPa=0.46, **w, **units)

    def window(fn, steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn(steps)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / steps

    out = {"package": os.path.dirname(os.path.abspath(xequinet_amd.__file__)), "library": lib.LIB_PATH, "forms": {}}
    L = lib.load()
    for tag, make in forms.items():
        mark = lib.launch_count()
        d = make()
        d.run(ITERATIONS, check_every=20, record_every=RECORD_EVERY)
        torch.cuda.synchronize()
        names = lib.launch_names(mark)
        tensors = list(d._state()) + [d.trajectory[k] for k in sorted(d.trajectory)]
        rec = out["forms"][tag] = {"launches": names, "digests": [hashlib.sha256(x.detach().cpu().contiguous().numpy().tobytes()).hexdigest() for x in tensors]}
        rec["resident"] = [window(lambda n: d.run(n, check_every=20), RESIDENT_STEPS) for _ in range(RESIDENT_BLOCKS)]
        front, back, stream = getattr(L, d._front_name), getattr(L, d._back_name), lib.stream()
        fa, ba = (*d._front_args(), stream), (*d._back_args(True), stream)

        def own(n):
            for _ in range(n):
                assert front(*fa) == 0 and back(*ba) == 0

        own(20)
        rec["alone"] = [window(own, ALONE_STEPS) for _ in range(ALONE_BLOCKS)]
        own_names = [n for n in names if n in (d._front_name, d._back_name)]
        print(f"{tag}: {len(names)} launches, {len(own_names)} of the driver's entries; resident {statistics.median(rec['resident']):.4f} ms, "
              f"entries alone {statistics.median(rec['alone']):.4f} ms", flush=True)
        del d
        torch.cuda.empty_cache()
    with open(path, "w") as f:
        json.dump(out, f)


# ---------------------------------------------------------------------------------------------------------------- the driver
def child(cmd, seconds, package_root, log):
    """One GPU process under its own time limit; a failure ends the whole run (nothing more is started on the GPU)."""
    env = {k: v for k, v in os.environ.items() if k != "XEQ_LIB_PATH"}
    env["PYTHONPATH"] = package_root
    p = subprocess.run(["timeout", "-k", "10", str(seconds)] + cmd, env=env, cwd=package_root, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    log.write(f"$ {' '.join(cmd)}   [{package_root}] -> {p.returncode}\n{p.stdout}\n")
    log.flush()
    if p.returncode != 0:
        print(p.stdout[-3000:], flush=True)
        sys.exit(f"{' '.join(cmd)} ended with status {p.returncode}: the run stops here")
    return p.stdout


def verdict(samples_parent, samples_side):
    lo, hi, med_p, med = min(samples_parent), max(samples_parent), statistics.median(samples_parent), statistics.median(samples_side)
    word = "inside the parent's spread" if lo <= med <= hi else ("BELOW the parent's spread (faster)" if med < lo else "ABOVE the parent's spread (slower)")
    return lo <= med <= hi, med_p, med, word


def drive(parent, out_path, bench_repeats, rounds):
    work = os.path.dirname(os.path.abspath(out_path))
    os.makedirs(work, exist_ok=True)
    sides = {"parent": os.path.abspath(parent), "branch": ROOT}
    for root in sides.values():
        assert os.path.isfile(os.path.join(root, "xequinet_amd", "libxeq_hip.so")) and os.path.isfile(os.path.join(root, "bench.py")), root
    lines, same, timed, slower = [], True, True, []
    with open(os.path.join(work, "resident_shared_refactor_children.log"), "w") as log:
        recs = {}
        for r in range(rounds):
            for side, root in sides.items():
                path = os.path.join(work, f"resident_shared_refactor_{side}_{r}.json")
                child([sys.executable, HERE, "--record", path], RECORD_TIMEOUT, root, log)
                one = json.load(open(path))
                print(f"recorded {side}, round {r}: {one['package']} with {one['library']}", flush=True)
                for tag, f in one["forms"].items():               # a side's rounds agree with each other; their blocks are pooled
                    g = recs.setdefault(side, one)["forms"][tag]
                    assert (f["launches"], f["digests"]) == (g["launches"], g["digests"]), (side, r, tag)
                    if g is not f:
                        g["resident"] += f["resident"]
                        g["alone"] += f["alone"]
        assert len({r["library"] for r in recs.values()}) == len(recs), "every side runs its own library"
        lines += [f"Per form: library launches from the driver's construction to the end of {ITERATIONS} iterations (recorder every {RECORD_EVERY}) and how many of them are",
                  "the driver's own two entries; whether the launch-name sequence and the SHA-256 of EVERY tensor of _state() and of the trajectory",
                  f"are the parent's; ms per iteration, median [min .. max] over {rounds} process(es) per side taken in turn: the resident run",
                  f"({RESIDENT_BLOCKS} blocks of {RESIDENT_STEPS} iterations per process) and the driver's two entries alone ({ALONE_BLOCKS} blocks of {ALONE_STEPS}), and whether the",
                  "branch's median lies inside the parent's min .. max.", ""]
        for tag, a in recs["parent"]["forms"].items():
            b = recs["branch"]["forms"][tag]
            own = sum(n in ENTRIES for n in a["launches"])
            same_seq, same_bits = b["launches"] == a["launches"], b["digests"] == a["digests"]
            same &= same_seq and same_bits
            lines.append(f"== {tag}: {len(a['launches'])} launches, {own} of the driver's entries; launches equal: {same_seq}   bits equal: {same_bits}   "
                         f"digests {' '.join(d[:8] for d in a['digests'])}")
            for what in ("resident", "alone"):
                inside, med_p, med, word = verdict(a[what], b[what])
                timed &= inside
                if med > max(a[what]):
                    slower.append(f"{tag} ({what})")
                lines.append(f"   {what:8s} parent {med_p:8.4f} ms [{min(a[what]):.4f} .. {max(a[what]):.4f}]   branch {med:8.4f} ms [{min(b[what]):.4f} .. {max(b[what]):.4f}] "
                             f"({(med / med_p - 1) * 100:+.2f} %): {word}")
        lines += ["", f"every launch sequence and digest agrees: {same}", f"the branch's median inside the parent's spread for every form: {timed}",
                  f"medians of the branch above the parent's spread: {', '.join(slower) or 'none'}", ""]
        open(out_path, "w").write("\n".join(lines) + "\n")
        print("\n".join(lines), flush=True)

        ms = {"parent": [], "branch": []}
        for _ in range(bench_repeats):
            for side in ms:
                text = child([sys.executable, os.path.join(sides[side], "bench.py"), "--gpus", "1", "--no-cpu-baseline"], BENCH_TIMEOUT, sides[side], log)
                ms[side].append(float(json.loads([ln for ln in text.splitlines() if ln.startswith("{")][-1])["ms_per_step"]))
        if bench_repeats:
            lines += [f"bench.py --gpus 1 (it does not run these drivers): ms_per_step, parent and branch in turn, {bench_repeats} process(es) each.",
                      f"   parent {' '.join(f'{v:.4f}' for v in ms['parent'])}", f"   branch {' '.join(f'{v:.4f}' for v in ms['branch'])}"]
            print("\n".join(lines[-3:]), flush=True)
        open(out_path, "w").write("\n".join(lines) + "\n")
    return 0 if same and timed else 1


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--record", default=None)
    ap.add_argument("--resources", nargs=2, default=None)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--bench-repeats", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    if args.resources:
        sys.exit(resources(*args.resources))
    if args.record:
        record(args.record)
    else:
        sys.exit(drive(args.parent, args.out, args.bench_repeats, args.rounds))
