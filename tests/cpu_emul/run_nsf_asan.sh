#!/bin/bash
# TEST-ONLY: the NSF vocoder entry points (csrc/nsf.h) under AddressSanitizer as a stand-alone host program (nn.hip + the emulation
# runtime + nsf_asan.cpp); no GPU, no Python.
set -euo pipefail
HERE="$(cd "$(dirname "$0")" && pwd)"
ROOT="$(cd "$HERE/../.." && pwd)"
CXX="${ALSEP_HOST_CXX:-/opt/rocm/lib/llvm/bin/clang++}"
OUT="${TMPDIR:-/tmp}/alsep_nsf_asan"
$CXX -std=c++17 -O1 -g -fsanitize=address -fno-omit-frame-pointer -pthread -I"$HERE" -I"$ROOT/audiolab_amd/csrc" \
  -Wno-unused-value -Wno-pass-failed -Wno-unknown-pragmas \
  -x c++ "$ROOT/audiolab_amd/csrc/nn.hip" -x c++ "$HERE/emul_runtime.cpp" -x c++ "$HERE/nsf_asan.cpp" -o "$OUT"
"$OUT"
