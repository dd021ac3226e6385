#!/bin/bash
# TEST-ONLY: the resampling sum pass (alsep_mix_sum_rates) under AddressSanitizer as a stand-alone host program (elementwise.hip, which
# includes mixdown.h, + the emulation runtime + mix_rate_asan.cpp); no GPU, no Python.
set -euo pipefail
HERE="$(cd "$(dirname "$0")" && pwd)"
ROOT="$(cd "$HERE/../.." && pwd)"
CXX="${ALSEP_HOST_CXX:-/opt/rocm/lib/llvm/bin/clang++}"
OUT="${TMPDIR:-/tmp}/alsep_mix_rate_asan"
$CXX -std=c++17 -O1 -g -fsanitize=address -fno-omit-frame-pointer -pthread -I"$HERE" -I"$ROOT/audiolab_amd/csrc" \
  -Wno-unused-value -Wno-pass-failed -Wno-unknown-pragmas \
  -x c++ "$ROOT/audiolab_amd/csrc/elementwise.hip" -x c++ "$HERE/emul_runtime.cpp" -x c++ "$HERE/mix_rate_asan.cpp" -o "$OUT"
"$OUT"
