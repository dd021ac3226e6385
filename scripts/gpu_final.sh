#!/bin/bash
# Round-end evidence: GPU tests, smoke, default bench (with cpu baseline), rocprof kernel stats, PMC traffic.
set -u
OUT="${OUT:-out}"
cd "${GRAFT_REPO_ROOT:-/root/repo}"
mkdir -p $OUT
export TMPDIR=/tmp
timeout -k 10 900 python -u -m pytest tests -m gpu -v --timeout 420 > $OUT/pytest_gpu_full.log 2>&1; tail -4 $OUT/pytest_gpu_full.log | tee $OUT/pytest_gpu.log
timeout 300 python -c "import __graft_entry__ as g; g.build(); g.smoke()" 2>&1 | tail -2 | tee $OUT/smoke.log
timeout 900 python bench.py --full 2>&1 | tail -1 | tee $OUT/bench_default.log
rm -rf $OUT/prof
timeout 900 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof -- python bench.py --full --steps 2 --warmup 1 --no-cpu-baseline > $OUT/bench_prof.log 2>&1
f=$(find $OUT/prof -name "*kernel_stats.csv" | head -1)
[ -n "$f" ] && cp "$f" $OUT/kernel_stats.csv
python scripts/trace_summary.py "$(find $OUT/prof -name '*kernel_trace.csv' | head -1)" 40 > $OUT/trace_summary.txt
find $OUT/prof -name "*kernel_trace.csv" -size +20M -delete
rm -rf $OUT/pmc
for c in FETCH_SIZE WRITE_SIZE; do
  timeout 1500 rocprofv3 --pmc $c --output-format csv -d $OUT/pmc/$c -- python bench.py --full --steps 1 --warmup 0 --no-cpu-baseline > $OUT/pmc_$c.log 2>&1
done
python scripts/pmc_summary.py $OUT/pmc > /dev/null
python scripts/pmc_traffic.py $OUT/pmc/pmc_summary.json $OUT/pmc_traffic.json | head -12
find $OUT/pmc -name "*counter_collection.csv" -delete
