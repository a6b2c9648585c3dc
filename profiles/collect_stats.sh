#!/bin/bash
# Run ON THE GPU BOX from the repo root:  profiles/collect_stats.sh <round-tag> [bench.py flags]
# Per-kernel time of the bench command: rocprofv3 --kernel-trace --stats (no counters in this pass).
# Leaves $XEQ_PROFILE_OUT/<tag>_kernel_stats.csv (default profile_out/; copied to profiles/ by hand after review) and the bench JSON line.
tag=${1:-r01}; shift
R=${GRAFT_REPO_ROOT:-$(pwd)}
O=$(realpath -m "${XEQ_PROFILE_OUT:-$R/profile_out}")
mkdir -p $O
cd /tmp && export TMPDIR=/tmp
# library-GEMM selections are timed in an un-profiled run and replayed under the profiler (no tuning kernels in the trace);
# --full: the bench line keeps its roofline and the trace its host-launched calibration steps
python3 $R/bench.py --full --steps 2 --warmup 3 --no-cpu-baseline --gemm-results $O/gemm_$tag.csv "$@" > $O/tune_$tag.log 2>&1
rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_$tag -- python3 $R/bench.py --full --steps 10 --warmup 3 --no-cpu-baseline --gemm-results $O/gemm_$tag.csv "$@" > $O/prof_$tag.log 2>&1
rc=$?
f=$(find $O/prof_$tag -name '*kernel_stats.csv' | head -1)
[ -n "$f" ] && cp "$f" $O/${tag}_kernel_stats.csv
grep '^{"metric"' $O/prof_$tag.log > $O/${tag}_bench_under_rocprof.json
rm -rf $O/prof_$tag   # raw traces are large
exit $rc
