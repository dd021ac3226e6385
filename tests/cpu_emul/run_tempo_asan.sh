#!/bin/bash
# TEST-ONLY: the tempo entry points under AddressSanitizer as a stand-alone host program (reverb.hip + the emulation
# runtime + tempo_asan.cpp); no GPU, no Python.
set -euo pipefail
HERE="$(cd "$(dirname "$0")" && pwd)"
ROOT="$(cd "$HERE/../.." && pwd)"
CXX="${ALSEP_HOST_CXX:-/opt/rocm/lib/llvm/bin/clang++}"
OUT="${TMPDIR:-/tmp}/alsep_tempo_asan"
$CXX -std=c++17 -O1 -g -fsanitize=address -fno-omit-frame-pointer -pthread -I"$HERE" -I"$ROOT/audiolab_amd/csrc" \
  -Wno-unused-value -Wno-pass-failed -Wno-unknown-pragmas \
  -x c++ "$ROOT/audiolab_amd/csrc/reverb.hip" -x c++ "$HERE/emul_runtime.cpp" -x c++ "$HERE/tempo_asan.cpp" -o "$OUT"
"$OUT"
