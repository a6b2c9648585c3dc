"""The record behind "the runtime refactor moved no launch, no bit and no millisecond" (profiles/runtime_refactor.txt): the capture classes of
xequinet_amd/runtime.py under TWO copies of the Python package -- the parent commit's and this tree's -- against the SAME built
libxeq_hip.so (XEQ_LIB_PATH), each run in a process of its own, the two taken in turn.

    python profiles/runtime_refactor.py --parent DIR --out FILE [--repeats 3]
        DIR holds the parent commit's ``xequinet_amd/`` (Python files; no library) and ``bench.py``.  Writes FILE; exit status 1 unless every
        sequence and digest agrees.  Every child process runs under ``timeout -k 10``; the first one that fails ends the run.
    python profiles/runtime_refactor.py --record FILE.json
        (what the driver starts, once per package) the sequences and digests of whichever package sys.path finds first.

Recorded per configuration and size: the entry-point names (lib.launch_names) of every launch from the construction of the object through
its first call -- the warm-up runs and the capture -- then through a call behind lib.bump_pack_epoch() (captured again), for GraphedStepPBC
also through a call behind grow(); ``captures``; SHA-256 of the bytes of every result tensor behind each of those calls.
Sizes: six aspirin frames and the 192-atom water box; QM9-1024 and water_512 (what bench.py runs).
Times: bench.py's ms_per_step in its default mode (two steps in flight), with --lanes 2, chunked and periodic, parent and branch in turn, ``--repeats`` times each.  The margin is measured, not chosen: the
branch's median has to lie inside the parent's own min .. max of this very run.
"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.abspath(__file__)
DEV = "cuda"
BENCH_MODES = [
    ("default (qm9_1024; the default IS --in-flight 2: GraphedStepsInFlight)", ["--steps", "200", "--warmup", "20"]),
    ("--lanes 2 (GraphedLanes)", ["--lanes", "2", "--steps", "200", "--warmup", "20"]),
    ("chunked (qm9_8192_sharded, 900 000 edges per chunk, two in flight)", ["--workload", "qm9_8192_sharded", "--max-chunk-edges", "900000", "--steps", "50", "--warmup", "5"]),
    ("periodic (water_512)", ["--workload", "water_512", "--steps", "200", "--warmup", "20"]),
]
RECORD_TIMEOUT, BENCH_TIMEOUT = 420, 300


# ---------------------------------------------------------------------------------------------------------------- one package: --record
def record(path):
    if ROOT not in sys.path:
        sys.path.append(ROOT)                 # (behind whatever PYTHONPATH put in front: the parent's copy, when the driver says so)
    import numpy as np
    import torch

    import xequinet_amd
    from xequinet_amd import lib, runtime
    from xequinet_amd.data import NeighborTransform, XequiBatch
    from xequinet_amd.data import synthetic as syn
    from xequinet_amd.nn import resolve_model

    torch.manual_seed(0)
    model = resolve_model("xpainn").eval().requires_grad_(False).to(DEV)
    cutoff = float(model.cutoff_radius)
    t = lambda a, dt=None: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).to(DEV)
    out = {"package": os.path.dirname(os.path.abspath(xequinet_amd.__file__)), "library": lib.LIB_PATH, "configs": {}}

    def digests(res):
        torch.cuda.synchronize()
        return {k: hashlib.sha256(v.detach().cpu().contiguous().numpy().tobytes()).hexdigest() for k, v in sorted(res.items()) if isinstance(v, torch.Tensor)}

    def run(tag, make, call, grow=None):
        """make() -> object; call(object) -> results; grow(object): the PBC step's own re-capture."""
        rec, mark = {}, lib.launch_count()

        def segment(name, res):
            nonlocal mark
            rec[name] = {"launches": lib.launch_names(mark), "results": digests(res)}
            mark = lib.launch_count()

        obj = make()
        segment("first call", call(obj))
        segment("second call", call(obj))
        lib.bump_pack_epoch()
        segment("behind a bumped pack epoch", call(obj))
        if grow is not None:
            grow(obj)
            segment("behind grow()", call(obj))
        rec["captures"] = int(obj.captures) if hasattr(obj, "captures") else [int(st.captures) for st in obj.steps]
        out["configs"][tag] = rec
        print(tag, {k: len(v["launches"]) for k, v in rec.items() if isinstance(v, dict)}, "captures", rec["captures"], flush=True)
        del obj

    def open_batch(size, pos, z, ptr):
        pos_d, z_d, ptr_d = t(pos, torch.float32), t(z), t(ptr)
        batch_d = t(np.repeat(np.arange(len(ptr) - 1), np.diff(ptr)))
        cap = (len(pos) + 64, len(ptr) - 1, runtime.pair_capacity(ptr))
        data = NeighborTransform(cutoff)(XequiBatch(pos_d, z_d, ptr_d)).to_dict()
        run(f"{size} / GraphedModel", lambda: runtime.GraphedModel(model, tune_gemms=False), lambda g: g(data))
        run(f"{size} / GraphedStep", lambda: runtime.GraphedStep(model, cap), lambda g: g(pos_d, z_d, ptr_d, batch=batch_d))
        run(f"{size} / GraphedLanes(2)", lambda: runtime.GraphedLanes(model, cap, lanes=2), lambda g: g(pos_d, z_d, ptr_d, batch_d, ptr))
        run(f"{size} / GraphedStepsInFlight(2)", lambda: runtime.GraphedStepsInFlight(model, cap, depth=2), lambda g: g(pos_d, z_d, ptr_d, batch_d))

        def chunks():
            g = runtime.GraphedChunks(model, ptr, max_edges=cap[2] // 3 + cap[2] // 50, depth=2)
            assert g.n_chunks >= 3, g.n_chunks
            return g

        run(f"{size} / GraphedChunks(depth 2)", chunks, lambda g: g(pos_d, z_d, ptr_d, batch_d))

    def box(size, pos, z, cell):
        pos_d, z_d, cell_d = t(pos, torch.float32), t(z), t(np.asarray(cell).reshape(3, 3), torch.float32)
        n0 = int(NeighborTransform(cutoff)(XequiBatch(pos_d, z_d, t(np.array([0, len(pos)])), pbc=torch.tensor([[True, True, True]], device=DEV),
                                                      cell=cell_d.reshape(1, 3, 3))).edge_index.shape[1])
        for tag, kw in (("GraphedStepPBC", {}), ("GraphedStepPBC(device_cell, virial)", dict(device_cell=True, compute_virial=True))):
            run(f"{size} / {tag}", lambda: runtime.GraphedStepPBC(model, len(pos), int(1.25 * n0) + 1024, **kw),
                lambda g: g(pos_d, z_d, cell_d, [True, True, True]), grow=lambda g: g.grow(n0))

    pos, z, ptr = syn.synth_md17_frames(6)
    open_batch("aspirin x 6", pos, z, ptr)
    pos, z, ptr, cell = syn.synth_water_box(4, seed=5)
    box("water box, 192 atoms", pos, z, cell)
    pos, z, ptr, _ = syn.make_workload("qm9_1024", seed=1234)
    open_batch("qm9_1024", pos, z, ptr)
    pos, z, ptr, cell = syn.make_workload("water_512", seed=1234)
    box("water_512", pos, z, cell)
    with open(path, "w") as f:
        json.dump(out, f)


# ---------------------------------------------------------------------------------------------------------------- the driver
def child(cmd, seconds, package_root, log):
    """One GPU process under its own time limit; a failure ends the whole run (nothing more is started on the GPU)."""
    env = dict(os.environ, XEQ_LIB_PATH=os.path.join(ROOT, "xequinet_amd", "libxeq_hip.so"), PYTHONPATH=package_root)
    p = subprocess.run(["timeout", "-k", "10", str(seconds)] + cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    log.write(f"$ {' '.join(cmd)}   [{package_root}] -> {p.returncode}\n{p.stdout}\n")
    log.flush()
    if p.returncode != 0:
        print(p.stdout[-3000:], flush=True)
        sys.exit(f"{' '.join(cmd)} ended with status {p.returncode}: the run stops here")
    return p.stdout


def drive(parent, out_path, repeats):
    work = os.path.dirname(os.path.abspath(out_path))
    os.makedirs(work, exist_ok=True)
    sides = {"parent": os.path.abspath(parent), "branch": ROOT}
    assert os.path.isdir(os.path.join(sides["parent"], "xequinet_amd")) and os.path.isfile(os.path.join(sides["parent"], "bench.py")), parent
    lines, ok = [], True
    with open(os.path.join(work, "runtime_refactor_children.log"), "w") as log:
        recs = {}
        for side, root in sides.items():
            path = os.path.join(work, f"runtime_refactor_{side}.json")
            child([sys.executable, HERE, "--record", path], RECORD_TIMEOUT, root, log)
            recs[side] = json.load(open(path))
            print(f"recorded {side}: {recs[side]['package']}", flush=True)
        assert recs["parent"]["package"] != recs["branch"]["package"] and recs["parent"]["library"] == recs["branch"]["library"], "two packages, one library"
        lines += ["Launch sequences (entry points of libxeq_hip.so, lib.launch_names), captures and results of the capture classes of xequinet_amd/runtime.py",
                  "under the parent commit's Python package and under the refactored one, both on the SAME libxeq_hip.so, one process each, one MI355X, one",
                  "session (profiles/runtime_refactor.py).  Per call: launches of the library, SHA-256 (first 16 digits) of the sequence of their names,",
                  "and whether the sequence and EVERY result tensor's bytes (energy, atomic energies, forces, n_edges, virial ...) are the parent's.", ""]
        for tag in recs["parent"]["configs"]:
            a, b = recs["parent"]["configs"][tag], recs["branch"]["configs"].get(tag, {})
            same_caps = a["captures"] == b.get("captures")
            ok &= same_caps
            lines.append(f"== {tag}: captures parent {a['captures']} | branch {b.get('captures')}{'' if same_caps else '   <-- DIFFER'}")
            for seg, ra in a.items():
                if not isinstance(ra, dict):
                    continue
                rb = b.get(seg, {"launches": None, "results": None})
                same_seq, same_res = ra["launches"] == rb["launches"], ra["results"] == rb["results"]
                ok &= same_seq and same_res
                sha = hashlib.sha256("\n".join(ra["launches"]).encode()).hexdigest()[:16]
                lines.append(f"   {seg:28s} {len(ra['launches']):4d} launches  {sha}  sequence equal: {same_seq}  results equal ({len(ra['results'])} tensors): {same_res}")
                if seg == "first call":
                    lines.append(f"      energy {ra['results']['energy'][:16]}  forces {ra['results']['forces'][:16]}")
        lines += ["", f"every sequence, capture count and digest agrees: {ok}", ""]
        open(out_path, "w").write("\n".join(lines) + "\n")

        lines += [f"bench.py --gpus 1 --no-cpu-baseline <mode>: ms_per_step, parent and branch in turn, {repeats} processes each (same call, same card).",
                  "Verdict per mode: the branch's median inside the parent's own min .. max of this run, or not; a spread above 5 % of the parent's",
                  "median is marked as too wide to decide anything.", ""]
        for name, extra in BENCH_MODES:
            ms = {"parent": [], "branch": []}
            for _ in range(repeats):
                for side, root in sides.items():
                    text = child([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--no-cpu-baseline"] + extra, BENCH_TIMEOUT, root, log)
                    ms[side].append(float(json.loads([ln for ln in text.splitlines() if ln.startswith("{")][-1])["ms_per_step"]))
            lo, hi, med_p, med_b = min(ms["parent"]), max(ms["parent"]), statistics.median(ms["parent"]), statistics.median(ms["branch"])
            inside, wide = lo <= med_b <= hi, (hi - lo) > 0.05 * med_p
            verdict = ("inside the parent's spread" if inside else ("BELOW the parent's spread (faster)" if med_b < lo else "ABOVE the parent's spread (slower)"))
            if wide:
                verdict += "; the spread is too wide to decide anything"
            lines += [f"== {name}",
                      f"   parent {' '.join(f'{v:.4f}' for v in ms['parent'])}   min {lo:.4f} max {hi:.4f} ({(hi - lo) / med_p * 100:.2f} % of the median) median {med_p:.4f}",
                      f"   branch {' '.join(f'{v:.4f}' for v in ms['branch'])}   median {med_b:.4f} ({(med_b / med_p - 1) * 100:+.2f} %): {verdict}"]
            print("\n".join(lines[-3:]), flush=True)
            open(out_path, "w").write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--record", default=None)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    if args.record:
        record(args.record)
    else:
        sys.exit(drive(args.parent, args.out, args.repeats))
