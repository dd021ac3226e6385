"""CPU emulation of the unchanged kernel sources: the 3x3 convs of c = 192 / 288 on conv3x3_bf16_allco_kernel<6, 48 | 64> in two / three
output groups of 96 channels (ALSEP_CONV_ALLCO=2) against the plain kernel (ALSEP_CONV_ALLCO=0: conv3x3_bf16_kernel<64>).  Same
48-channel chunks and k-step order, same epilogue arithmetic and rounding: the network's output must be the same bits; the launch counts
say which kernel ran.  Shapes and cases: conv_allco_groups_common.py.  One subprocess per environment: the switches are read once."""
import pytest

from conv_allco_groups_common import CASES, DEFAULT_TW, ROUTED_192, check, off_run, on_env, run


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("c,tw", CASES)
@pytest.mark.parametrize("grid", [5, 0])
def test_output_groups_same_bits(emul_lib_path, tmp_path, dtype, c, tw, grid):
    """grid capped at 5 (several tiles per workgroup, a partial last round) and uncapped (the groups of one tile per workgroup)"""
    off = off_run(emul_lib_path, tmp_path, dtype, c, 900)
    check(off, run(emul_lib_path, tmp_path, "on", dtype, c, on_env(tw, grid), 900), f"c {c}, 8 x {tw}, grid {grid}", dtype, c, tw)


def test_default_routing(emul_lib_path, tmp_path):
    """ALSEP_CONV_ALLCO unset, no tile floor: c = 192 goes where kConvAllcoRouted says, at the default tile width"""
    off = off_run(emul_lib_path, tmp_path, "bf16", 192, 900)
    check(off, run(emul_lib_path, tmp_path, "dflt", "bf16", 192, {"ALSEP_CONV_BIG": "2"}, 900), "default routing", "bf16", 192, DEFAULT_TW,
          routed=ROUTED_192)
