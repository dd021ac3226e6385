"""GPU (-m gpu): the 3x3 convs of c = 144 on conv3x3_bf16_allco_kernel against the kernel it replaces (ALSEP_CONV_ALLCO=0), as
test_emul_conv_allco.py does on the emulated sources.  The asynchronous parts only exist here -- counted vmcnt waits, LDS-DMA landing
under the MFMAs, one raw barrier per stage -- so every forward is made twice in its process and must equal itself: a race in the rings
shows as a mismatch.  ALSEP_CONV_ALLCO=2 forces every shape the kernel serves, whatever the product routes (kConvAllcoRouted)."""
import pytest

from conv_allco_common import OFF, ON, check, run

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("c", [144])
def test_all_channels_conv_same_bits(tmp_path, dtype, c):
    """grid capped at 5 (several tiles per workgroup, a partial last round) and uncapped (one tile per workgroup)"""
    off = run("cuda", tmp_path, "off", dtype, c, OFF, 300)
    check(off, run("cuda", tmp_path, "on5", dtype, c, dict(ON, ALSEP_CONV_ALLCO_GRID="5"), 300), "grid 5", dtype, c)
    check(off, run("cuda", tmp_path, "on", dtype, c, ON, 300), "one tile per workgroup", dtype, c)
