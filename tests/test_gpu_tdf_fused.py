"""GPU (-m gpu): both TDF linears of a block on tdf_bf16_fused_kernel against the two tdf_bf16_kernel launches it replaces
(ALSEP_TDF_FUSED=0), as test_emul_tdf_fused.py does on the emulated sources.  The asynchronous parts only exist here -- the tile of
the next item arriving by LDS-DMA under this item's MFMAs, one counted vmcnt wait per item with the stores of the item before still
in flight, raw barriers -- so every forward is made twice in its process and must equal itself: a race in the buffers shows as a
mismatch.  ALSEP_TDF_FUSED=2 forces every shape an instance serves, whatever the product routes (kTdfFusedRouted and its floor).
Shapes and cases: tdf_fused_common.py."""
import pytest
import torch

from tdf_fused_common import DEEP, L2, L3, NEW, OFF, ON, check, check_oracle, run

pytestmark = pytest.mark.gpu

# tdfnet.hip: kTdfFusedRouted and kTdfFusedFloor -- which levels the default sends to the fused kernel, and from how many items
ROUTED = {768: True, 384: True}
# batch at which a one-block network of L2 / L3 has exactly the floor's items: 832 * 4 * 3 = 9984, 416 * 4 * 4 / 2 = 3328
FLOOR_BATCH = {768: 832, 384: 416}


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("cfg", [L2, L3], ids=["F768-c144", "F384-c192"])
def test_one_block_same_bits(tmp_path, dtype, cfg):
    """grid capped at 5 (several items per workgroup, a partial last round) and uncapped (one item per workgroup); random weights and
    the shifting all-passthrough network, the latter also against the storage oracle"""
    off = run("cuda", tmp_path, "off", dtype, cfg, OFF, 300)
    on5 = run("cuda", tmp_path, "on5", dtype, cfg, dict(ON, ALSEP_TDF_FUSED_GRID="5"), 300)
    check(off, on5, "grid 5", 1)
    check_oracle(on5, dtype, cfg, "grid 5")
    on = run("cuda", tmp_path, "on", dtype, cfg, ON, 300)
    check(off, on, "one item per workgroup", 1)
    check_oracle(on, dtype, cfg, "one item per workgroup")


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_both_levels_from_the_top(tmp_path, dtype):
    """seven blocks: level 2 in the encoder and the decoder, level 3 at the bottleneck -- three fused launches; levels 0 and 1 keep
    their kernels (the pinned counts are equal)"""
    off = run("cuda", tmp_path, "off", dtype, DEEP, OFF, 300, kinds="random")
    on = run("cuda", tmp_path, "on", dtype, DEEP, ON, 300, kinds="random")
    check(off, on, "seven blocks", 3)
    assert off["random"][2]["tdf_bf16_persist_kernel"] > 0
    on5 = run("cuda", tmp_path, "on5", dtype, DEEP, dict(ON, ALSEP_TDF_FUSED_GRID="5"), 300, kinds="random")
    check(off, on5, "seven blocks, grid 5", 3)


@pytest.mark.parametrize("f", [768, 384])
def test_default_routing_at_the_floor(tmp_path, f):
    """ALSEP_TDF_FUSED unset, exactly the floor's items: the level goes where kTdfFusedRouted says; the same bits as the old pair"""
    cfg = L2 if f == 768 else L3
    off = run("cuda", tmp_path, "off", "bf16", cfg, OFF, 300, kinds="random", batch=FLOOR_BATCH[f])
    dflt = run("cuda", tmp_path, "dflt", "bf16", cfg, {}, 300, kinds="random", batch=FLOOR_BATCH[f])
    check(off, dflt, "default routing at the floor", 1 if ROUTED[f] else 0)


def test_default_routing_below_the_floor(tmp_path):
    """ALSEP_TDF_FUSED unset, 36 items: the old pair, the same bits"""
    off = run("cuda", tmp_path, "off", "bf16", L2, OFF, 300, kinds="random")
    dflt = run("cuda", tmp_path, "dflt", "bf16", L2, {}, 300, kinds="random")
    check(off, dflt, "default routing below the floor", 0)
    assert dflt["random"][2]["tdf_bf16_kernel"] == 2


@pytest.mark.parametrize("f", [768, 384])
def test_default_routing_one_batch_under_the_floor(tmp_path, f):
    """one batch entry fewer than the floor (12 / 8 items under it): the old pair"""
    got = run("cuda", tmp_path, "under", "bf16", L2 if f == 768 else L3, {}, 300, kinds="random", batch=FLOOR_BATCH[f] - 1)["random"]
    assert got[2][NEW] == 0 and got[2]["tdf_bf16_kernel"] == 2, got[2]
    assert torch.equal(got[0], got[1])


@pytest.mark.parametrize("case", [dict(cfg=dict(L2, bn=0), dtype="bf16"), dict(cfg=L2, dtype="f32"),
                                  dict(cfg=dict(DEEP, dim_f=2048, num_blocks=5), dtype="bf16")], ids=["bn0", "float32", "kuielab-2048"])
def test_fallbacks_stay_where_they_were(tmp_path, case):
    """a single TDF linear (bn = 0), a float32 network and a geometry whose level-2 F (512) no instance serves never reach the new
    name: the switch changes neither counts nor bits"""
    off = run("cuda", tmp_path, "off", case["dtype"], case["cfg"], OFF, 300, kinds="random")
    on = run("cuda", tmp_path, "on", case["dtype"], case["cfg"], ON, 300, kinds="random")
    check(off, on, "fallback", 0)
    assert on["random"][2][NEW] == 0
