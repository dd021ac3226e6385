#!/bin/bash
# HBM traffic counters for the bench kernels: separate --pmc passes (FETCH_SIZE, WRITE_SIZE), no tracing domains.
set -u
OUT="${OUT:-out}"
cd "${GRAFT_REPO_ROOT:-/root/repo}"
mkdir -p $OUT
export TMPDIR=/tmp
rm -rf $OUT/pmc
for c in FETCH_SIZE WRITE_SIZE; do
  timeout 900 rocprofv3 --pmc $c --output-format csv -d $OUT/pmc/$c -- python bench.py --full --steps 1 --warmup 0 --no-cpu-baseline --seconds 60 > $OUT/pmc_$c.log 2>&1
  tail -2 $OUT/pmc_$c.log | cut -c1-300
done
python scripts/pmc_summary.py $OUT/pmc | head -60
find $OUT/pmc -name "*counter_collection.csv" -size +8M -delete
