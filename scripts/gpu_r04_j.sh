#!/bin/bash
# round 4, call j: kernel trace of the Mel-Band Roformer workload (half precision) -> busy / idle split
set -u
OUT="${OUT:-out}"
cd "${GRAFT_REPO_ROOT:-/root/repo}"
mkdir -p $OUT
R=$(pwd); case "$OUT" in /*) ;; *) OUT="$R/$OUT";; esac
cd /tmp && export TMPDIR=/tmp
timeout -k 10 500 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/prof -- python3 "$R/bench.py" --full --workload model --model vocals_mel_band_roformer.ckpt --dtype f16 --steps 2 --warmup 1 --no-cpu-baseline > $OUT/r04_j_bench.log 2>&1
rc=$?; echo "prof rc $rc"
cd $GRAFT_REPO_ROOT
f=$(ls /tmp/prof/*/*_kernel_trace.csv | head -1)
python3 scripts/trace_gaps.py $f 0.6 | tee $OUT/r04_mel_half_trace_gaps.txt
cp $(ls /tmp/prof/*/*_kernel_stats.csv | head -1) $OUT/r04_roformer_mel_half_kernel_stats.csv
tail -1 $OUT/r04_j_bench.log | cut -c1-300
exit $rc
