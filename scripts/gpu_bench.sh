#!/bin/bash
# usage: gpu_bench.sh [bench args]   -- bench + rocprof kernel stats on the GPU box
set -u
OUT="${OUT:-out}"
cd "${GRAFT_REPO_ROOT:-/root/repo}"
mkdir -p $OUT
export TMPDIR=/tmp
timeout 900 python bench.py --full --steps 2 --warmup 1 --no-cpu-baseline "$@" 2>&1 | tail -3 | tee $OUT/bench.log
rm -rf $OUT/prof
timeout 900 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof -- python bench.py --full --steps 1 --warmup 1 --no-cpu-baseline "$@" > $OUT/bench_prof.log 2>&1
f=$(find $OUT/prof -name "*kernel_stats.csv" | head -1)
[ -n "$f" ] && cp "$f" $OUT/kernel_stats.csv && head -14 "$f" | cut -c1-160
find $OUT/prof -name "*kernel_trace.csv" -size +20M -delete
