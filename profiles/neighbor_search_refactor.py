"""The record behind "the neighbour-search refactor moved no launch, no bit and no microsecond" (profiles/neighbor_search_refactor.txt):
every search form under the PARENT commit's package with the parent's libraries, then under this tree's package with its own, one child
process per side on one MI355X in one session, each under its own time limit; a side starts only if the one before it ended cleanly.

    python profiles/neighbor_search_refactor.py --parent DIR --out FILE [--rounds 1] [--bench-repeats 3]
        DIR holds the parent commit's built ``xequinet_amd/`` (Python files AND libxeq_hip.so / libxeq_torch.so) and its ``bench.py``.
        --rounds: processes per side, the sides taken in turn, their blocks pooled.  With one process per side two builds of IDENTICAL
        device code land outside each other's spread (a process's own blocks agree to 1 %, two processes differ by up to 5 %): the
        spread that decides has to hold the process-to-process part, so the record is taken with several rounds.
        Writes FILE; exit status 1 unless every digest and launch sequence agrees and every median lies inside the parent's spread.
    python profiles/neighbor_search_refactor.py --record FILE.json
        (what the driver starts, once per side) whichever package sys.path finds first.

Inputs (seeded, f32 and f64, cutoff 5): the QM9-like batch of 1 024 molecules (pair sweep, sized and capacity form, the registered
operator); the 1 536-atom water box (periodic: all images, pruned sized, pruned capacity, the registered operator); a 6 591-atom water box
above both bin-grid thresholds (open bin grid on its positions as one cluster, periodic bin grid).
Recorded per form and dtype: SHA-256 of every tensor the form returns or fills (edge_index, cell_offsets, row pointer, count); the
library launches of ONE call (lib.launch_names), compared under RENAMED; the time of one call -- the form's whole host sequence (bin
sort, count, scan, fill and, in the sized forms, the read-back of the edge count): a host clock around as many calls as fill
BLOCK_SECONDS (at least MIN_BLOCK_CALLS; the count is fixed per form after the warm-up), ending in a device synchronise, BLOCKS times, the forms taken in turn so that a drift of the machine reaches all of them; median and min .. max of
the blocks.  The margin is measured, not chosen: a side's median has to lie inside the parent's own min .. max of this very run.
Then bench.py in its default mode, parent and branch in turn.
"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.abspath(__file__)
DEV = "cuda"
CUTOFF = 5.0
WARMUP_CALLS, MIN_BLOCK_CALLS, BLOCK_SECONDS, BLOCKS = 50, 300, 0.2, 9
RECORD_TIMEOUT, BENCH_TIMEOUT = 420, 300
# the parent's entry names -> this tree's (the launch-name ring holds one name per entry call)
RENAMED = {f"xeq_radius_graph{pbc}_{what}{form}": f"xeq_neighbors_{what}" for pbc in ("", "_pbc") for what in ("count", "fill")
           for form in ("", "_cl", "_pruned")}
RENAMED.update({"xeq_radius_graph_bin_ids": "xeq_neighbors_bin_ids", "xeq_radius_graph_pbc_bin_ids": "xeq_neighbors_bin_ids"})


# ---------------------------------------------------------------------------------------------------------------- one side: --record
def record(path):
    import numpy as np
    import torch

    import xequinet_amd
    from xequinet_amd import lib, ops
    from xequinet_amd.data import synthetic as syn
    from xequinet_amd.data.radius_graph import _host_cell_tables, _with_bins, _wrap_on_device
    from xequinet_amd.interface.scripted import load_torch_library

    load_torch_library()
    t = lambda a, dt=None: torch.as_tensor(np.ascontiguousarray(a), dtype=dt).to(DEV)
    pbc = [True, True, True]
    forms = {}

    def periodic(pos, cell, dtype):
        """what ops.radius_graph_pbc_raw takes, formed as data.radius_graph.radius_graph_pbc forms it"""
        pos_d, cell_d = t(pos, dtype), t(np.asarray(cell).reshape(1, 3, 3), dtype)
        ptr_d = t(np.array([0, len(pos)]))
        reps, _, tab = _host_cell_tables(cell_d, pbc, CUTOFF, with_inverse=True)
        pw, shift = _wrap_on_device(pos_d, ptr_d, cell_d, tab["cell_inv"], pbc)
        return (pw, ptr_d, tab["pbc_offsets"], tab["cell_offsets"], shift, CUTOFF), (tab["recip"], tab["thr"], reps), pos_d, cell_d

    q_pos, _, q_ptr, _ = syn.make_workload("qm9_1024", seed=1234)
    w_pos, _, _, w_cell = syn.make_workload("water_512", seed=1234)
    b_pos, _, _, b_cell = syn.synth_water_box(13, seed=5)
    assert len(w_pos) == 1536 and len(b_pos) == 6591
    for name, dtype in (("f32", torch.float32), ("f64", torch.float64)):
        qp, qptr = t(q_pos, dtype), t(q_ptr)
        forms[f"pair sweep, QM9-1024, {name}"] = lambda qp=qp, qptr=qptr: ops.radius_graph_raw(qp, qptr, CUTOFF)
        n_q = int(ops.radius_graph_raw(qp, qptr, CUTOFF)[0].shape[1])
        q_buf = torch.zeros((2, n_q + 1024), dtype=torch.int64, device=DEV)
        forms[f"pair sweep, capacity form, QM9-1024, {name}"] = lambda qp=qp, qptr=qptr, q_buf=q_buf: (*ops.radius_graph_capacity(qp, qptr, CUTOFF, q_buf), q_buf)
        forms[f"registered xeq::radius_graph, QM9-1024, {name}"] = lambda qp=qp, qptr=qptr: torch.ops.xeq.radius_graph(qp, qptr, CUTOFF)
        args, prune, wp, wc = periodic(w_pos, w_cell, dtype)
        forms[f"periodic all images, water 1 536, {name}"] = lambda args=args: ops.radius_graph_pbc_raw(*args)
        forms[f"periodic pruned, water 1 536, {name}"] = lambda args=args, prune=prune: ops.radius_graph_pbc_raw(*args, prune=prune)
        n_w = int(ops.radius_graph_pbc_raw(*args, prune=prune)[0].shape[1])
        e_buf, o_buf = torch.zeros((2, n_w + 1024), dtype=torch.int64, device=DEV), torch.zeros((n_w + 1024, 3), dtype=dtype, device=DEV)
        forms[f"periodic pruned, capacity form, water 1 536, {name}"] = lambda args=args, prune=prune, e_buf=e_buf, o_buf=o_buf: (
            *ops.radius_graph_pbc_capacity(*args, prune, e_buf, o_buf), e_buf, o_buf)
        pbc_d = torch.tensor(pbc, device=DEV)
        forms[f"registered xeq::radius_graph_pbc, water 1 536, {name}"] = lambda wp=wp, wc=wc, pbc_d=pbc_d: torch.ops.xeq.radius_graph_pbc(wp, wc[0], pbc_d, CUTOFF)
        bp, bptr = t(b_pos, dtype), t(np.array([0, len(b_pos)]))
        assert ops._use_cell_list(len(b_pos), 1)
        forms[f"open bin grid, 6 591 atoms, {name}"] = lambda bp=bp, bptr=bptr: ops.radius_graph_raw(bp, bptr, CUTOFF)
        args_b, prune_b, _, _ = periodic(b_pos, b_cell, dtype)
        binned = _with_bins(prune_b, pbc)
        forms[f"periodic bin grid, 6 591 atoms, {name}"] = lambda args_b=args_b, binned=binned: ops.radius_graph_pbc_raw(*args_b, prune=binned)

    out = {"package": os.path.dirname(os.path.abspath(xequinet_amd.__file__)), "library": lib.LIB_PATH, "forms": {}}
    for tag, call in forms.items():
        for _ in range(WARMUP_CALLS):
            res = call()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(WARMUP_CALLS):
            call()
        torch.cuda.synchronize()
        calls = max(MIN_BLOCK_CALLS, int(BLOCK_SECONDS * WARMUP_CALLS / (time.perf_counter() - t0)))
        mark = lib.launch_count()
        res = call()
        torch.cuda.synchronize()
        out["forms"][tag] = {"launches": lib.launch_names(mark), "us": [], "calls": calls,
                             "digests": [hashlib.sha256(r.detach().cpu().contiguous().numpy().tobytes()).hexdigest() for r in res],
                             "edges": int(res[0].shape[1]) if res[0].dim() == 2 else int(res[1].item())}
    for _ in range(BLOCKS):
        for tag, call in forms.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            calls = out["forms"][tag]["calls"]
            for _ in range(calls):
                call()
            torch.cuda.synchronize()
            out["forms"][tag]["us"].append((time.perf_counter() - t0) / calls * 1e6)
    for tag, rec in out["forms"].items():
        print(f"{tag}: {rec['edges']} edges, {len(rec['launches'])} launches, median {statistics.median(rec['us']):.1f} us", flush=True)
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
    return lo <= med <= hi, lo, hi, med_p, med, word


def drive(parent, out_path, bench_repeats, rounds):
    work = os.path.dirname(os.path.abspath(out_path))
    os.makedirs(work, exist_ok=True)
    sides = {"parent": os.path.abspath(parent), "branch": ROOT}
    for root in sides.values():
        assert os.path.isfile(os.path.join(root, "xequinet_amd", "libxeq_hip.so")) and os.path.isfile(os.path.join(root, "bench.py")), root
    lines, same, timed, slower = [], True, True, False
    with open(os.path.join(work, "neighbor_search_refactor_children.log"), "w") as log:
        recs = {}
        for r in range(rounds):
            for side, root in sides.items():
                path = os.path.join(work, f"neighbor_search_refactor_{side}_{r}.json")
                child([sys.executable, HERE, "--record", path], RECORD_TIMEOUT, root, log)
                one = json.load(open(path))
                print(f"recorded {side}, round {r}: {one['package']} with {one['library']}", flush=True)
                for tag, f in one["forms"].items():               # a side's rounds agree with each other; their blocks are pooled
                    g = recs.setdefault(side, one)["forms"][tag]
                    assert (f["launches"], f["digests"], f["edges"]) == (g["launches"], g["digests"], g["edges"]), (side, r, tag)
                    if g is not f:
                        g["us"] += f["us"]
        assert len({r["library"] for r in recs.values()}) == len(recs), "every side runs its own library"
        lines += ["Every neighbour-search form under the parent commit's package and libraries and under this tree's, each side in processes of its",
                  "own, one MI355X, one session (profiles/neighbor_search_refactor.py).  Per form: edges; library launches of one call and whether their names",
                  "are the parent's under the old-to-new table; whether the SHA-256 of EVERY tensor the form returns or fills (edge_index,",
                  "cell_offsets, row pointer, count) is the parent's; microseconds per call (host clock around %.1f s of calls ending in a synchronise," % BLOCK_SECONDS,
                  "%d such blocks per process, the forms in turn, %d process(es) per side taken in turn): median [min .. max], and whether the" % (BLOCKS, rounds),
                  "side's median lies inside the parent's min .. max.", ""]
        for tag, a in recs["parent"]["forms"].items():
            names = [RENAMED.get(n, n) for n in a["launches"]]
            lo, hi = min(a["us"]), max(a["us"])
            lines.append(f"== {tag}: {a['edges']} edges, {len(names)} launches: {' '.join(names)}")
            lines.append(f"   {'parent':8s} {statistics.median(a['us']):8.1f} us [{lo:.1f} .. {hi:.1f}]   digests {' '.join(d[:12] for d in a['digests'])}")
            for side in list(sides)[1:]:
                b = recs[side]["forms"][tag]
                same_seq, same_bits = b["launches"] == names, b["digests"] == a["digests"] and b["edges"] == a["edges"]
                inside, _, _, med_p, med, word = verdict(a["us"], b["us"])
                same &= same_seq and same_bits
                timed &= inside or side != "branch"
                slower |= side == "branch" and med > max(a["us"])
                lines.append(f"   {side:8s} {med:8.1f} us [{min(b['us']):.1f} .. {max(b['us']):.1f}] ({(med / med_p - 1) * 100:+.2f} %): {word}"
                             f"   launches equal: {same_seq}   bits equal: {same_bits}")
        lines += ["", f"every launch sequence and digest agrees: {same}", f"the branch's median inside the parent's spread for every form: {timed}",
                  f"no median of the branch above the parent's spread: {not slower}", ""]
        open(out_path, "w").write("\n".join(lines) + "\n")
        print("\n".join(lines), flush=True)

        lines += [f"bench.py --gpus 1 (default mode: qm9_1024, two steps in flight): ms_per_step, parent and branch in turn, {bench_repeats} processes each.", ""]
        ms = {"parent": [], "branch": []}
        for _ in range(bench_repeats):
            for side in ms:
                text = child([sys.executable, os.path.join(sides[side], "bench.py"), "--gpus", "1", "--no-cpu-baseline"], BENCH_TIMEOUT, sides[side], log)
                ms[side].append(float(json.loads([ln for ln in text.splitlines() if ln.startswith("{")][-1])["ms_per_step"]))
        if bench_repeats:
            inside, lo, hi, med_p, med, word = verdict(ms["parent"], ms["branch"])
            timed &= inside
            lines += [f"   parent {' '.join(f'{v:.4f}' for v in ms['parent'])}   min {lo:.4f} max {hi:.4f} median {med_p:.4f}",
                      f"   branch {' '.join(f'{v:.4f}' for v in ms['branch'])}   median {med:.4f} ({(med / med_p - 1) * 100:+.2f} %): {word}"]
            print("\n".join(lines[-2:]), flush=True)
        open(out_path, "w").write("\n".join(lines) + "\n")
    return 0 if same and timed else 1


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--record", default=None)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--bench-repeats", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=1)
    args = ap.parse_args()
    if args.record:
        record(args.record)
    else:
        sys.exit(drive(args.parent, args.out, args.bench_repeats, args.rounds))
