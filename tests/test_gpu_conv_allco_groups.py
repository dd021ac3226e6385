"""GPU (-m gpu): the 3x3 convs of c = 192 / 288 on conv3x3_bf16_allco_kernel<6, 48 | 64> in two / three output groups of 96 channels
against the plain kernel (ALSEP_CONV_ALLCO=0), as test_emul_conv_allco_groups.py does on the emulated sources.  The asynchronous parts
only exist here -- counted vmcnt waits, LDS-DMA landing under the MFMAs, one raw barrier per stage, the weight ring running from one
group's image into the next -- so every forward is made twice in its process and must equal itself: a race in the rings shows as a
mismatch.  ALSEP_CONV_ALLCO=2 forces every shape the kernel serves, whatever the product routes (kConvAllcoRouted)."""
import pytest

from conv_allco_groups_common import CASES, DEFAULT_TW, ROUTED_192, check, off_run, on_env, run

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("c,tw", CASES)
@pytest.mark.parametrize("grid", [5, 0])
def test_output_groups_same_bits(tmp_path, dtype, c, tw, grid):
    """grid capped at 5 (several tiles per workgroup, a partial last round) and uncapped (the groups of one tile per workgroup)"""
    off = off_run("cuda", tmp_path, dtype, c, 300)
    check(off, run("cuda", tmp_path, "on", dtype, c, on_env(tw, grid), 300), f"c {c}, 8 x {tw}, grid {grid}", dtype, c, tw)


def test_default_routing(tmp_path):
    """ALSEP_CONV_ALLCO unset, no tile floor: c = 192 goes where kConvAllcoRouted says, at the default tile width"""
    off = off_run("cuda", tmp_path, "bf16", 192, 300)
    check(off, run("cuda", tmp_path, "dflt", "bf16", 192, {"ALSEP_CONV_BIG": "2"}, 300), "default routing", "bf16", 192, DEFAULT_TW,
          routed=ROUTED_192)
