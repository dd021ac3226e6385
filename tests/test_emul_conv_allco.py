"""CPU emulation of the unchanged kernel sources: the 3x3 convs of c = 144 on conv3x3_bf16_allco_kernel (all output channels per
patch, k-step-major weight ring, two patch buffers, fragment reads running ahead across the stage barrier) against the kernel it
replaces (ALSEP_CONV_ALLCO=0: conv3x3_bf16_big_kernel<3>).  Same 48-channel chunks and
k-step order, same epilogue arithmetic and rounding: the network's output must be the same bits; the launch counts say which kernel ran.
Shapes and cases: conv_allco_common.py.  One subprocess per environment: the switches are read once."""
import pytest

from conv_allco_common import OFF, ON, check, run


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("c", [144])
def test_all_channels_conv_same_bits(emul_lib_path, tmp_path, dtype, c):
    """grid capped at 5 (several tiles per workgroup, a partial last round) and uncapped (one tile per workgroup)"""
    off = run(emul_lib_path, tmp_path, "off", dtype, c, OFF, 900)
    check(off, run(emul_lib_path, tmp_path, "on5", dtype, c, dict(ON, ALSEP_CONV_ALLCO_GRID="5"), 900), "grid 5", dtype, c)
    check(off, run(emul_lib_path, tmp_path, "on", dtype, c, ON, 900), "one tile per workgroup", dtype, c)
