"""Generated-code check of the VR networks' half-precision kernels (csrc/vrnet_h.h, compiled in nn_half.hip): the convolution issues
v_mfma_f32_16x16x32_f16, so no packed float32 instruction (v_pk_*_f32) may appear in any of them, and none may use
scratch.  The Demucs convolution next to them keeps its 16 instantiations."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("vr_conv_h_kernel", "vr_depthwise_h_kernel", "vr_resize_h_kernel", "vr_copy_slice_h_kernel", "vr_mean_hh_kernel")


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_half_vr_kernels_have_mfma_no_packed_f32_and_no_scratch(tmp_path):
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    assert "vrnet_h.h" in g.HEADERS                                            # a change to the header rebuilds the library
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    asm = str(tmp_path / "nn_half.s")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I", g.CSRC] + g.unit_flags("nn_half.hip") +
                   ["--cuda-device-only", "-S", os.path.join(g.CSRC, "nn_half.hip"), "-o", asm], check=True, capture_output=True, timeout=900)
    text = open(asm).read()
    bodies = {m.group(1): m.group(2) for m in re.finditer(r"^(_Z\S+):[^\n]*\n(.*?)^\.Lfunc_end", text, re.S | re.M)}
    ours = {n: b for n, b in bodies.items() if any(k in n for k in KERNELS)}
    found = {k for k in KERNELS if any(k in n for n in ours)}
    assert found == set(KERNELS), f"kernels not found in the assembly: {set(KERNELS) - found}"
    convs = [n for n in ours if "vr_conv_h_kernel" in n]
    assert len(convs) == 16                                                     # NJ 1/2/4/8 x vector / element staging x plain / fused input
    for n in convs:
        assert "v_mfma_f32_16x16x32_f16" in ours[n], f"{n}: no f16 MFMA"
    for name, body in ours.items():
        assert not re.search(r"\bv_pk_\w+_f32\b", body), f"{name}: packed float32 instruction"
        meta = re.search(r"\.amdhsa_kernel " + re.escape(name) + r"\n(.*?)\.end_amdhsa_kernel", text, re.S)
        assert meta and re.search(r"\.amdhsa_private_segment_fixed_size 0\n", meta.group(1)), f"{name}: uses scratch"
    assert sum("nn_dconv_h_kernel" in n for n in bodies) == 16                  # tests/test_codegen_demucs_half.py's count still holds
