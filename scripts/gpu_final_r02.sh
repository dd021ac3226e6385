#!/bin/bash
# Round-2 evidence on one box: PMC traffic first (two passes; the bench line reads the resulting file, stamped with the kernel-source
# hash), then GPU tests, smoke, default bench (with cpu baseline), rocprof kernel stats, SQ counters (one pass).
# Outputs under $OUT/; scripts/collect_r02.sh copies the summaries into profiles/.
set -u
OUT="${OUT:-out}"
cd "${GRAFT_REPO_ROOT:-/root/repo}"
mkdir -p $OUT
export TMPDIR=/tmp
rm -rf $OUT/pmc
for c in FETCH_SIZE WRITE_SIZE; do
  timeout -k 10 1200 rocprofv3 --pmc $c --output-format csv -d $OUT/pmc/$c -- python3 bench.py --full --steps 1 --warmup 0 --no-cpu-baseline > $OUT/pmc_$c.log 2>&1
done
python scripts/pmc_summary.py $OUT/pmc > /dev/null
W=$(grep -o 'windows/launch=[0-9]*' $OUT/pmc_FETCH_SIZE.log | tail -1 | cut -d= -f2)
python scripts/pmc_traffic.py $OUT/pmc/pmc_summary.json $OUT/pmc_traffic.json ${W:-} | head -12
find $OUT/pmc -name "*counter_collection.csv" -delete
cp $OUT/pmc_traffic.json profiles/pmc_traffic.json
timeout -k 10 900 python -u -m pytest tests -m gpu -q --timeout 420 > $OUT/pytest_gpu_full.log 2>&1; tail -3 $OUT/pytest_gpu_full.log | tee $OUT/pytest_gpu.log
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -2 | tee $OUT/smoke.log
timeout -k 10 900 python bench.py --full 2>$OUT/bench_default.err | tail -1 | tee $OUT/bench_default.log | cut -c1-400
rm -rf $OUT/prof
timeout -k 10 900 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof -- python3 bench.py --full --steps 2 --warmup 1 --no-cpu-baseline > $OUT/bench_prof.log 2>&1
f=$(find $OUT/prof -name "*kernel_stats.csv" | head -1)
[ -n "$f" ] && cp "$f" $OUT/kernel_stats.csv
python scripts/trace_summary.py "$(find $OUT/prof -name '*kernel_trace.csv' | head -1)" 60 > $OUT/trace_summary.txt
find $OUT/prof -name "*kernel_trace.csv" -size +20M -delete
rm -rf $OUT/pmc_sq
timeout -k 10 900 rocprofv3 --pmc SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_VALU_MFMA_BUSY_CYCLES SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE --output-format csv -d $OUT/pmc_sq/a -- python3 bench.py --full --steps 1 --warmup 0 --no-cpu-baseline --seconds 60 > $OUT/pmc_sq.log 2>&1
timeout -k 10 900 rocprofv3 --pmc GRBM_GUI_ACTIVE --output-format csv -d $OUT/pmc_sq/b -- python3 bench.py --full --steps 1 --warmup 0 --no-cpu-baseline --seconds 60 >> $OUT/pmc_sq.log 2>&1
python scripts/pmc_summary.py $OUT/pmc_sq > /dev/null
python scripts/sq_table.py $OUT/pmc_sq/pmc_summary.json > $OUT/sq_table.txt 2>&1; head -8 $OUT/sq_table.txt | cut -c1-220
find $OUT/pmc_sq -name "*counter_collection.csv" -delete
