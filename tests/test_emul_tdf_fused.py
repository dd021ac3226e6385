"""CPU emulation of the unchanged kernel sources: both TDF linears of a block on tdf_bf16_fused_kernel (the block's input tile resident
in LDS, the hidden tile never written to memory, all weight fragments in registers) against the two tdf_bf16_kernel launches it
replaces (ALSEP_TDF_FUSED=0).  Same MFMA sequence per output element, same rounding of the hidden tile, same epilogue arithmetic:
the network's output must be the same bits; the launch counts say which kernel ran.  Shapes and cases: tdf_fused_common.py.  One
subprocess per environment: the switches are read once."""
import pytest

from tdf_fused_common import L2, L3, NEW, OFF, ON, check, check_oracle, run


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("cfg", [L2, L3], ids=["F768-c144", "F384-c192"])
def test_one_block_same_bits(emul_lib_path, tmp_path, dtype, cfg):
    """grid capped at 5 (several items per workgroup, a partial last round) and uncapped (one item per workgroup); random weights and
    the shifting all-passthrough network, the latter also against the storage oracle"""
    off = run(emul_lib_path, tmp_path, "off", dtype, cfg, OFF, 900)
    on5 = run(emul_lib_path, tmp_path, "on5", dtype, cfg, dict(ON, ALSEP_TDF_FUSED_GRID="5"), 900)
    check(off, on5, "grid 5", 1)
    check_oracle(on5, dtype, cfg, "grid 5")
    on = run(emul_lib_path, tmp_path, "on", dtype, cfg, ON, 900)
    check(off, on, "one item per workgroup", 1)
    check_oracle(on, dtype, cfg, "one item per workgroup")


def test_below_the_floor_default_is_the_old_pair(emul_lib_path, tmp_path):
    """ALSEP_TDF_FUSED unset: 36 items are far below the floor of the routed levels, so the default runs the two old launches"""
    off = run(emul_lib_path, tmp_path, "off", "bf16", L2, OFF, 900, kinds="random")
    dflt = run(emul_lib_path, tmp_path, "dflt", "bf16", L2, {}, 900, kinds="random")
    check(off, dflt, "default routing below the floor", 0)
    assert dflt["random"][2]["tdf_bf16_kernel"] == 2


@pytest.mark.parametrize("case", [dict(cfg=dict(L2, bn=0), dtype="bf16"), dict(cfg=dict(L2, dim_f=512, n_fft=1024), dtype="bf16")],
                         ids=["bn0", "F512"])
def test_fallbacks_stay_where_they_were(emul_lib_path, tmp_path, case):
    """a single TDF linear (bn = 0) and an F no instance serves never reach the new name: the switch changes neither counts nor bits
    (the float32 network and the seven-block network that reaches both levels from the top run on the GPU only: emulated they
    take minutes)"""
    off = run(emul_lib_path, tmp_path, "off", case["dtype"], case["cfg"], OFF, 900, kinds="random")
    on = run(emul_lib_path, tmp_path, "on", case["dtype"], case["cfg"], ON, 900, kinds="random")
    check(off, on, "fallback", 0)
    assert on["random"][2][NEW] == 0
