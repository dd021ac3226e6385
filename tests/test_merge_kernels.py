"""Stem mixdown (audiolab_amd/merge.py -> csrc/mixdown.h: alsep_mix_sum / alsep_mix_power / alsep_mix_finish) on the emulated kernels
(-m "not gpu") and on the GPU (-m gpu), same bodies, against tests/golden/merge.npz -- what the stdlib C module ``audioop`` (the arithmetic
under pydub, which the reference's wrappers/merge.py runs) computes on the cases of tests/merge_cases.py (scripts/make_golden_merge.py).

Everything here is integer arithmetic: every sample, every peak and every rms must EQUAL the fixture, no tolerance.  The one place a
tolerance exists is the host's f1 / f2 (Python floats through ``10 **`` and ``log10``): 4 ulp against the stored ones, and where they are not
bit-equal the samples may differ by 1 LSB (the floor of a product whose factor moved by an ulp); where they are bit-equal, by nothing."""
import math

import numpy as np
import pytest
import torch

from tests.conftest import host, on
from tests.merge_cases import CASES, VARIANTS, exact_sum_squares, fixture_of, make_case, np_mul


def ulps(a: float, b: float) -> int:
    if a == b:
        return 0
    if not (math.isfinite(a) and math.isfinite(b)):
        return 1 << 62
    return abs(int(np.float64(a).view(np.int64)) - int(np.float64(b).view(np.int64)))


def run_passes(dev, name, bits, g, acc_buffer=None):
    """sum, power, finish fed the STORED f1 / f2 -> everything equal to the fixture"""
    from audiolab_amd import merge
    stems, widths, _, _, _ = make_case(name, bits)
    acc, peak = merge.mix_sum(dev, [on(dev, s) for s in stems], widths, bits, acc=acc_buffer)
    assert acc.dtype == torch.int32 and acc.device.type == dev.device.type and tuple(acc.shape) == g["acc"].shape
    assert np.array_equal(host(acc).astype(np.int64), g["acc"])
    assert peak == g["peak"]
    if g["peak"] == 0:
        assert not g["y2"].any()
        return
    count = g["acc"].size
    peak1, s = merge.mix_power(dev, acc, bits, g["f1"])
    assert peak1 == g["peak1"]
    assert int(math.sqrt(s / count)) == g["rms"]
    assert s == exact_sum_squares(np_mul(g["acc"], g["f1"], bits))           # the sum itself is exact, not only its root
    y2, yf = merge.mix_finish(dev, acc, bits, g["f1"], g["f2"], want_float=True)
    assert np.array_equal(host(y2).astype(np.int64), g["y2"])
    assert np.array_equal(host(yf), (g["y2"].astype(np.float64) / (1 << (bits - 1))).astype(np.float32))


@pytest.mark.parametrize("name,bits", VARIANTS)
def test_passes_equal_audioop(dev, golden_dir, name, bits):
    run_passes(dev, name, bits, fixture_of(golden_dir, name, bits))


@pytest.mark.parametrize("name,bits", [("odd_63", 16), ("odd_63", 32), ("three_ragged", 32), ("single_sample", 32), ("hot", 32)])
def test_rows_off_the_16_byte_grid(dev, golden_dir, name, bits):
    """a dense [2, N] mix with odd N: its second row starts off the 16-byte grid, every pass takes its scalar path"""
    g = fixture_of(golden_dir, name, bits)
    assert g["acc"].shape[1] % 2 == 1
    buf = torch.empty(g["acc"].shape, dtype=torch.int32, device=dev.device)
    assert buf.stride(0) == g["acc"].shape[1]
    run_passes(dev, name, bits, g, acc_buffer=buf)


def full_mix(dev, name, bits, max_per_launch=0, explicit=True):
    from audiolab_amd import merge
    stems, widths, source, source_width, prevent = make_case(name, bits)
    return merge.mixdown_array([on(dev, s) for s in stems], (on(dev, source), source_width), prevent_clipping=prevent,
                               bits=bits if explicit else None, src_bits=widths, max_per_launch=max_per_launch, ctx=dev)


@pytest.mark.parametrize("name,bits", VARIANTS)
def test_host_maths_and_whole_mixdown(dev, golden_dir, name, bits):
    g = fixture_of(golden_dir, name, bits)
    out, rec = full_mix(dev, name, bits)
    assert out.dtype == torch.int32 and tuple(out.shape) == g["y2"].shape and rec.bits == bits
    assert rec.peak == g["peak"] and rec.rms == g["rms"]
    d1, d2 = ulps(rec.f1, g["f1"]), ulps(rec.f2, g["f2"])
    assert d1 <= 4 and d2 <= 4, f"f1 {rec.f1!r} / {g['f1']!r}, f2 {rec.f2!r} / {g['f2']!r}"
    assert ulps(rec.target_dBFS, g["target"]) <= 4 and ulps(rec.current_dBFS, g["current"]) <= 4
    assert ulps(rec.gain_dB, g["gain"]) <= 16                                 # a difference of two values within 4 ulp each
    got = host(out).astype(np.int64)
    if d1 == 0 and d2 == 0:
        assert np.array_equal(got, g["y2"])
    else:
        print(f"{name}/{bits}: f1 {rec.f1!r} vs {g['f1']!r} ({d1} ulp), f2 {rec.f2!r} vs {g['f2']!r} ({d2} ulp)")
        assert np.max(np.abs(got - g["y2"])) <= 1


@pytest.mark.parametrize("name", ["nine_stems", "hot"])
@pytest.mark.parametrize("bits", [16, 32])
def test_chaining_does_not_change_a_bit(dev, golden_dir, name, bits):
    """1 and 2 stems per launch against as many as one launch holds (nine stems: 8 + 1 even then)"""
    assert len(CASES["nine_stems"]["stems"]) > 8
    whole, rec = full_mix(dev, name, bits)
    for per in (1, 2):
        part, rec_p = full_mix(dev, name, bits, max_per_launch=per)
        assert np.array_equal(host(part), host(whole)) and rec_p == rec
    dev.launch_counts_reset()
    full_mix(dev, name, bits, max_per_launch=2)
    n_stems = len(CASES[name]["stems"])
    assert dev.launch_count("mix_sum_kernel") == 1 + (n_stems + 1) // 2      # the source alone, then the stems two by two


def test_width_of_the_mix_follows_the_stems(dev, golden_dir):
    assert full_mix(dev, "all16", 16, explicit=False)[1].bits == 16
    out, rec = full_mix(dev, "rereverb16", 32, explicit=False)
    assert rec.bits == 32 and np.array_equal(host(out).astype(np.int64), fixture_of(golden_dir, "rereverb16", 32)["y2"])
    from audiolab_amd import merge
    stems, _, source, _, _ = make_case("one_stem", 32)
    out, rec = merge.mixdown_array(stems, source, ctx=dev)                    # host arrays, no widths: float stems, a 32-bit mix
    assert rec.bits == 32 and np.array_equal(host(out).astype(np.int64), fixture_of(golden_dir, "one_stem", 32)["y2"])
    # a precomputed target instead of a source signal
    out2, rec2 = merge.mixdown_array(stems, rec.target_dBFS, ctx=dev)
    assert rec2 == rec and np.array_equal(host(out2), host(out))


def test_source_dbfs_on_its_own_grid(dev, golden_dir):
    from audiolab_amd import merge
    _, _, source, _, _ = make_case("three_ragged", 16)
    assert merge.source_dbfs(on(dev, source), dev, 16) == fixture_of(golden_dir, "three_ragged", 16)["target"]
    assert merge.source_dbfs(on(dev, source), dev, 24) == fixture_of(golden_dir, "three_ragged", 32)["target"]
    assert merge.source_dbfs(np.zeros((2, 9), np.float32), dev) == -math.inf


def test_argument_errors(dev):
    from audiolab_amd import _lib, merge
    from audiolab_amd._lib import AlsepError
    a, b3 = torch.zeros((2, 40), device=dev.device), torch.zeros((3, 40), device=dev.device)
    with pytest.raises(AlsepError):                                          # 3 channels into 2 ... or 2 into 3
        merge.mix_sum(dev, [a, b3], [32, 32], 32)
    with pytest.raises(AlsepError):                                          # a 32-bit stem into a 16-bit mix
        merge.mixdown_array([a], 0.0, bits=16, src_bits=[32], ctx=dev)
    with pytest.raises(AlsepError):
        merge.mixdown_array([], 0.0, ctx=dev)
    # the C entry points themselves
    lib = dev.lib
    acc, peak = torch.empty((2, 40), dtype=torch.int32, device=dev.device), torch.empty((1,), dtype=torch.int32, device=dev.device)
    stems = (_lib.MixStem * 9)(*[_lib.MixStem(a.data_ptr(), 40, 40, 2, 32)] * 9)

    def call(n_stems, bits=32, channels=2, n=40, ld=40, prev=None):
        return lib.alsep_mix_sum(dev.handle, prev, ld, stems, n_stems, channels, n, bits, acc.data_ptr(), ld, peak.data_ptr())
    assert call(8) == 0 and call(8, prev=acc.data_ptr()) == 0
    assert call(9) == -1 and call(0) == -1 and call(1, bits=24) == -1 and call(1, bits=16) == -1 and call(1, ld=39) == -1
    assert call(1, channels=3) == -1 and call(1, n=0) == -1
    assert call(0, prev=acc.data_ptr()) == 0                                 # a copy with its peak
    assert lib.alsep_mix_power_workspace_bytes(2, 40) == 24 and lib.alsep_mix_power_workspace_bytes(0, 40) == -1
    ws, out = torch.empty((3,), dtype=torch.int64, device=dev.device), torch.empty((3,), dtype=torch.int64, device=dev.device)
    assert lib.alsep_mix_power(dev.handle, acc.data_ptr(), 2, 40, 40, 32, 1.0, ws.data_ptr(), 24, out.data_ptr()) == 0
    assert lib.alsep_mix_power(dev.handle, acc.data_ptr(), 2, 40, 40, 32, 1.0, ws.data_ptr(), 23, out.data_ptr()) == -1
    assert lib.alsep_mix_finish(dev.handle, acc.data_ptr(), 2, 40, 40, 8, 1.0, 1.0, acc.data_ptr(), 40, None, 0) == -1
    assert lib.alsep_mix_finish(dev.handle, acc.data_ptr(), 2, 40, 40, 32, 1.0, 1.0, acc.data_ptr(), 40, None, 0) == 0   # in place
    dev.synchronize()
