"""GPU (-m gpu): the 96 -> 48 upsampling folded into the level-1 residual TDF launch (tdf_bf16_persist_kernel<3, false, true>) against
the two launches it replaces (ALSEP_TDF_US_FOLD=0), as test_emul_tdf_us_fold.py does on the emulated sources.  What only exists here:
the skip runs requested chunks ahead of their use with counted waits beside the weight loads of the next row block, the LDS-DMA fill of
the next item behind the last chunk's stores, and the staging rows reused three ways inside a wave -- so every forward is made twice in
its process and must equal itself, and every folded forward must equal the unfolded one bit for bit.  ALSEP_TDF_US_FOLD is set
explicitly in every run: the test holds whatever the product's default is.  Shapes and cases: tdf_us_fold_common.py."""
import pytest

from tdf_us_fold_common import DEEP, F384, F768, NEW, OFF, ON, T16, check, check_oracle, run, run_jobs

pytestmark = pytest.mark.gpu
TIMEOUT = 300


JOBS = [(cfg, batch) for cfg in (F384, F768, T16) for batch in (1, 3)]
IDS = [f"{name}, batch {batch}" for name in ("F384", "F768", "F384-T16") for batch in (1, 3)]
_OFF = {}


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("grid", [None, "1", "2"], ids=["uncapped", "grid1", "grid2"])
def test_same_bits(tmp_path, dtype, grid):
    """level-1 F = 384 and 768 (one and two row blocks per wave), 4 and 8 level-1 frames, batch 1 and 3: one item per workgroup, then 1
    and 2 workgroups walking all the items (4 to 24 of them); one process per route runs all six shapes"""
    if dtype not in _OFF:                                      # the reference forwards: once per storage type, never changed
        _OFF[dtype] = run_jobs("cuda", tmp_path, "off", dtype, JOBS, OFF, TIMEOUT)
    off = _OFF[dtype]
    on = run_jobs("cuda", tmp_path, "on", dtype, JOBS, dict(ON, ALSEP_TDF_PERSIST_GRID=grid) if grid else ON, TIMEOUT)
    for what, a, b in zip(IDS, off, on):
        check(a, b, what, 1)


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_behind_a_deeper_decoder(tmp_path, dtype):
    """five blocks: the folded launch belongs to the first decoder block, whose input is itself an upsampling's output"""
    off = run("cuda", tmp_path, "off", dtype, DEEP, OFF, TIMEOUT, batch=3)
    on = run("cuda", tmp_path, "on", dtype, DEEP, ON, TIMEOUT, batch=3)
    check(off, on, "five blocks", 1)


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_storage_oracle(tmp_path, dtype):
    on = run("cuda", tmp_path, "on", dtype, F384, ON, TIMEOUT, batch=3, oracle=True)
    assert on[2][NEW] == 1, on[2]
    check_oracle(on, dtype, "F384 batch 3")


@pytest.mark.parametrize("case", [dict(dtype="bf16", cfg=F384, env={"ALSEP_TDF_PERSIST": "0"}), dict(dtype="f32", cfg=F384, env={}),
                                  dict(dtype="bf16", cfg=dict(F384, g=96), env={})], ids=["persist0", "float32", "level1-c192"])
def test_fallbacks_keep_the_two_launches(tmp_path, case):
    """without the persistent kernel, in a float32 network, and where level 1 has 192 channels (g = 96), the upsampling stays a launch of
    its own: the switch changes neither counts nor bits"""
    off = run("cuda", tmp_path, "off", case["dtype"], case["cfg"], dict(OFF, **case["env"]), TIMEOUT, batch=3)
    on = run("cuda", tmp_path, "on", case["dtype"], case["cfg"], dict(ON, **case["env"]), TIMEOUT, batch=3)
    check(off, on, "fallback", 0)
    assert on[2][NEW] == 0
