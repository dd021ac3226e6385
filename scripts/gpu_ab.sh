#!/bin/bash
# A/B of an environment switch on the bench: usage gpu_ab.sh VAR v1 v2 ...
set -u
OUT="${OUT:-out}"
cd "${GRAFT_REPO_ROOT:-/root/repo}"
mkdir -p $OUT
var=$1; shift
: > $OUT/ab.log
for v in "$@"; do
  env $var=$v timeout 600 python bench.py --full --steps 2 --warmup 1 --no-cpu-baseline 2>&1 | tail -1 | python -c "import sys,json; d=json.loads(sys.stdin.read()); print('$var=$v','value',d['value'],'ms/step',d['ms_per_step'], 'roofline',d['roofline']['kernel'],d['roofline']['avg_us'], {k:v['avg_us'] for k,v in d['kernels'].items()})" | tee -a $OUT/ab.log
done
