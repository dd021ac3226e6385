"""CPU emulation of the unchanged kernel sources: the 96 -> 48 upsampling folded into the level-1 residual TDF launch
(tdf_bf16_persist_kernel<3, false, true>) against the two launches it replaces (ALSEP_TDF_US_FOLD=0).  The folded epilogue rounds the
block's output to the storage type exactly where the store did, runs us_stream_kernel<96, 48>'s accumulator chains (one per tap,
16-channel m-tile and 16-pixel block, over the k-steps ascending) on those rounded pixels and forms relu(bn(acc)) * skip in fp32 with
one rounding, so the network's output must be the same bits; the launch counts say which route ran.  Shapes and cases:
tdf_us_fold_common.py.  The GPU twin is test_gpu_tdf_us_fold.py."""
import pytest

from tdf_us_fold_common import DEEP, F384, F768, NEW, OFF, ON, check, check_oracle, run

TIMEOUT = 900


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_one_row_block_same_bits(emul_lib_path, tmp_path, dtype):
    """level-1 F = 384, batch 3 = 12 items: one item per workgroup, then one workgroup walking all twelve; also the storage oracle"""
    off = run(emul_lib_path, tmp_path, "off", dtype, F384, OFF, TIMEOUT, batch=3)
    on = run(emul_lib_path, tmp_path, "on", dtype, F384, ON, TIMEOUT, batch=3, oracle=True)
    check(off, on, "F384 batch 3", 1)
    check_oracle(on, dtype, "F384 batch 3")
    on1 = run(emul_lib_path, tmp_path, "on1", dtype, F384, dict(ON, ALSEP_TDF_PERSIST_GRID="1"), TIMEOUT, batch=3)
    check(off, on1, "F384 batch 3, grid 1", 1)


def test_two_row_blocks_same_bits(emul_lib_path, tmp_path):
    """level-1 F = 768: every wave runs the folded epilogue twice per item; batch 1 = 4 items on 2 workgroups"""
    off = run(emul_lib_path, tmp_path, "off", "bf16", F768, OFF, TIMEOUT)
    on = run(emul_lib_path, tmp_path, "on", "bf16", F768, dict(ON, ALSEP_TDF_PERSIST_GRID="2"), TIMEOUT)
    check(off, on, "F768 batch 1, grid 2", 1)


def test_behind_a_deeper_decoder(emul_lib_path, tmp_path):
    """five blocks: the folded launch belongs to the first decoder block, whose input is itself an upsampling's output"""
    off = run(emul_lib_path, tmp_path, "off", "bf16", DEEP, OFF, TIMEOUT)
    on = run(emul_lib_path, tmp_path, "on", "bf16", DEEP, ON, TIMEOUT)
    check(off, on, "five blocks", 1)


@pytest.mark.parametrize("case", [dict(dtype="bf16", env={"ALSEP_TDF_PERSIST": "0"}), dict(dtype="f32", env={})], ids=["persist0", "float32"])
def test_fallbacks_keep_the_two_launches(emul_lib_path, tmp_path, case):
    """without the persistent kernel, and in a float32 network, the upsampling stays a launch of its own: same counts, same bits"""
    off = run(emul_lib_path, tmp_path, "off", case["dtype"], F384, dict(OFF, **case["env"]), TIMEOUT)
    on = run(emul_lib_path, tmp_path, "on", case["dtype"], F384, dict(ON, **case["env"]), TIMEOUT)
    check(off, on, "fallback", 0)
    assert on[2][NEW] == 0
