#!/bin/bash
# kernel trace of the bench (2 steps), grouped per (kernel, grid)
set -u
OUT="${OUT:-out}"
cd "${GRAFT_REPO_ROOT:-/root/repo}"
mkdir -p $OUT
export TMPDIR=/tmp
rm -rf $OUT/prof
timeout 900 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof -- python3 bench.py --full --steps 2 --warmup 1 --no-cpu-baseline > $OUT/bench_prof.log 2>&1
tail -1 $OUT/bench_prof.log | cut -c1-200
f=$(find $OUT/prof -name "*kernel_stats.csv" | head -1)
[ -n "$f" ] && cp "$f" $OUT/kernel_stats.csv
python scripts/trace_summary.py "$(find $OUT/prof -name '*kernel_trace.csv' | head -1)" 60 > $OUT/trace_summary.txt
find $OUT/prof -name "*kernel_trace.csv" -size +20M -delete
grep -E "stream|pix_gemm" $OUT/trace_summary.txt
