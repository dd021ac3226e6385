#!/bin/bash
# Round-4 evidence, call C: smoke, default bench line (precision + accuracy objects, PMC traffic from profiles/pmc_traffic.json), rocprof kernel stats
set -u
OUT="${OUT:-out}"
cd "${GRAFT_REPO_ROOT:-/root/repo}"
. scripts/gpu_final_common.sh
mkdir -p $OUT
export TMPDIR=/tmp
step 300 smoke python3 -c "import __graft_entry__ as g; g.smoke()" > $OUT/smoke.log 2>&1; tail -2 $OUT/smoke.log
step 700 bench python3 bench.py --full > $OUT/bench_default.log 2> $OUT/bench_default.err; tail -1 $OUT/bench_default.log | cut -c1-300
rm -rf /tmp/prof
step 400 prof rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/prof -- python3 bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --no-precision > $OUT/bench_prof.log 2>&1
f=$(find /tmp/prof -name "*kernel_stats.csv" | head -1)
[ -n "$f" ] && cp "$f" $OUT/kernel_stats.csv
python3 scripts/trace_summary.py "$(find /tmp/prof -name '*kernel_trace.csv' | head -1)" 60 > $OUT/trace_summary.txt; head -5 $OUT/trace_summary.txt | cut -c1-200
