"""Stems of differing sample rates in the mixdown (audiolab_amd/merge.py -> csrc/mixdown.h: alsep_mix_sum_rates, alsep_mix_ratecv_length) on
the emulated kernels (-m "not gpu") and on the GPU (-m gpu), same bodies, against tests/golden/merge_rates.npz -- what the stdlib C module
``audioop`` computes on the cases of tests/merge_rate_cases.py (scripts/make_golden_merge_rates.py): ``ratecv`` alone, and pydub's overlay
chain with ``tostereo`` / ``ratecv`` / ``lin2lin`` / ``add``.

Integer arithmetic throughout: every sample, length, peak and rms must EQUAL the fixture.  The one tolerance is the host's f1 / f2 rule of
tests/test_merge_kernels.py (4 ulp; where they are not bit-equal the samples may differ by 1 LSB)."""
import numpy as np
import pytest
import torch

from tests.conftest import host, on
from tests.merge_cases import VARIANTS, make_case, quantise
from tests.merge_rate_cases import (CHAIN_VARIANTS, CHAINS, CHANNELS, LENGTHS, NUMPY_RATE_OPS, PAIRS, WIDTHS, chain_fixture, digest, make_chain,
                                    np_ratecv, ratecv_fixture, ratecv_input, ratecv_length, reference_mix_rates)


def ulps(a: float, b: float) -> int:
    return abs(int(np.float64(a).view(np.int64)) - int(np.float64(b).view(np.int64)))


def expect_ratecv(got: np.ndarray, u: np.ndarray, want, what: str):
    """``want``: (samples or None, digest, length) of the fixture; ``u``: the input on its grid, for the message"""
    full, sha, k = want
    assert got.shape == (u.shape[0], k), f"{what}: {got.shape[1]} samples, audioop returns {k}"
    if full is not None:
        assert np.array_equal(got, full), f"{what}: first difference at {np.argwhere(got != full)[0]}"
    elif not np.array_equal(digest(got), sha):
        near = np_ratecv(u, *what[1:2], *what[0])                            # checked against the same digest by the CPU-only test below
        raise AssertionError(f"{what}: digest differs; against the closed form the first difference is at {np.argwhere(got != near)[:1]}")


# ---- 1. ratecv alone ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}-{p[1]}")
def test_ratecv_equals_audioop(dev, golden_dir, pair, width):
    from audiolab_amd import merge
    for channels in CHANNELS:
        for n in LENGTHS:
            x = ratecv_input(pair, width, channels, n)
            u = quantise(x, width, width)
            want = ratecv_fixture(golden_dir, pair, width, channels, n)
            assert want[2] == ratecv_length(n, *pair) == merge.ratecv_length(n, *pair) == dev.lib.alsep_mix_ratecv_length(n, *pair)
            got = merge.ratecv_array(on(dev, x), pair[0], pair[1], width, ctx=dev)                      # float32, quantised on the grid first
            assert got.dtype == torch.int32 and got.device.type == dev.device.type
            expect_ratecv(host(got).astype(np.int64), u, want, (pair, width, channels, n, "float32"))
            got = merge.ratecv_array(on(dev, u.astype(np.int32)), pair[0], pair[1], width, ctx=dev)     # int32 already on the grid
            expect_ratecv(host(got).astype(np.int64), u, want, (pair, width, channels, n, "int32"))


def test_extremes_are_neighbours_in_the_inputs():
    """what the cases above rest on: INT_MIN beside INT_MAX in every input that has room for it"""
    for width in WIDTHS:
        lo, hi = -(1 << (width - 1)), (1 << (width - 1)) - 1
        for n in (5, 147, 4099):
            u = quantise(ratecv_input(PAIRS[0], width, 2, n), width, width)
            for row in u:
                pairs = set(zip(row[:-1].tolist(), row[1:].tolist()))
                assert {(lo, hi), (hi, lo), (lo, lo), (hi, hi)} <= pairs


# ---- 2. chains ------------------------------------------------------------------------------------------------------------------------
def run_chain(dev, name, bits, max_per_launch=0):
    from audiolab_amd import merge
    stems, widths, rates, source = make_chain(name, bits)
    return merge.mixdown_array([on(dev, s) for s in stems], (on(dev, source), bits), bits=bits, src_bits=widths, max_per_launch=max_per_launch,
                               ctx=dev, rates=rates)


@pytest.mark.parametrize("name,bits", CHAIN_VARIANTS)
def test_chain_passes_equal_audioop(dev, golden_dir, name, bits):
    """sum (with the resampling inside), then power and finish fed the STORED f1 / f2: everything equal to the fixture"""
    from audiolab_amd import merge
    g = chain_fixture(golden_dir, name, bits)
    stems, widths, rates, _ = make_chain(name, bits)
    acc, peak, rate = merge.mix_sum_rates(dev, [on(dev, s) for s in stems], widths, rates, bits)
    assert rate == g["rate"] == max(rates) and acc.dtype == torch.int32 and tuple(acc.shape) == g["acc"].shape
    assert np.array_equal(host(acc).astype(np.int64), g["acc"])
    assert peak == g["peak"]
    peak1, s = merge.mix_power(dev, acc, bits, g["f1"])
    assert peak1 == g["peak1"] and int((s / g["acc"].size) ** 0.5) == g["rms"]
    y2 = merge.mix_finish(dev, acc, bits, g["f1"], g["f2"])
    assert np.array_equal(host(y2).astype(np.int64), g["y2"])


@pytest.mark.parametrize("name,bits", CHAIN_VARIANTS)
def test_chain_whole_mixdown(dev, golden_dir, name, bits):
    g = chain_fixture(golden_dir, name, bits)
    out, rec = run_chain(dev, name, bits)
    assert rec.rate == g["rate"] and rec.bits == bits and rec.peak == g["peak"] and rec.rms == g["rms"]
    d1, d2 = ulps(rec.f1, g["f1"]), ulps(rec.f2, g["f2"])
    assert d1 <= 4 and d2 <= 4, f"f1 {rec.f1!r} / {g['f1']!r}, f2 {rec.f2!r} / {g['f2']!r}"
    got = host(out).astype(np.int64)
    assert got.shape == g["y2"].shape
    if d1 == 0 and d2 == 0:
        assert np.array_equal(got, g["y2"])
    else:
        print(f"{name}/{bits}: f1 {rec.f1!r} vs {g['f1']!r} ({d1} ulp), f2 {rec.f2!r} vs {g['f2']!r} ({d2} ulp)")
        assert np.max(np.abs(got - g["y2"])) <= 1


# ---- 3. the split into launches does not matter ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["hot_rise", "nine_rise_at_5"])
@pytest.mark.parametrize("bits", [16, 32])
def test_chaining_does_not_change_a_bit(dev, name, bits):
    whole, rec = run_chain(dev, name, bits, max_per_launch=8)
    for per in (1, 2):
        part, rec_p = run_chain(dev, name, bits, max_per_launch=per)
        assert np.array_equal(host(part), host(whole)) and rec_p == rec
    from audiolab_amd import merge
    _, widths, rates, _ = make_chain(name, bits)
    dev.launch_counts_reset()
    run_chain(dev, name, bits, max_per_launch=2)
    assert dev.launch_count("mix_sum_rate_kernel") == len(merge.plan_rates(rates, widths, 2))
    assert dev.launch_count("mix_sum_kernel") == 1                           # the source's loudness alone


# ---- 4. rows off the 16-byte grid -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair,width", [((44100, 48000), 32), ((48000, 44100), 16), ((8000, 192000), 32), ((192000, 8000), 16)])
def test_rows_off_the_16_byte_grid(dev, golden_dir, pair, width):
    """dense [2, N] buffers with odd N and an odd output length: the second row of the operand and of acc start off the 16-byte grid, the
    pass takes its scalar paths, the integers are the same"""
    from audiolab_amd import _lib
    for n in (147, 4099) if pair[0] < pair[1] else (4099,):
        u = quantise(ratecv_input(pair, width, 2, n), width, width)
        want = ratecv_fixture(golden_dir, pair, width, 2, n)
        k = want[2]
        for kind in ("float32", "int32"):
            x = on(dev, ratecv_input(pair, width, 2, n)) if kind == "float32" else on(dev, u.astype(np.int32))
            acc = torch.empty((2, k), dtype=torch.int32, device=dev.device)
            peak = torch.empty((1,), dtype=torch.int32, device=dev.device)
            assert x.stride(0) == n and n % 2 == 1 and (acc.stride(0) == k and k % 4 != 0)
            op = (_lib.MixOperand * 1)(_lib.MixOperand(x.data_ptr(), n, n, pair[0], pair[1], 2, width, int(kind == "int32")))
            assert dev.lib.alsep_mix_sum_rates(dev.handle, op, 1, 2, k, width, acc.data_ptr(), k, peak.data_ptr()) == 0
            got = host(acc).astype(np.int64)
            expect_ratecv(got, u, want, (pair, width, 2, n, kind + ", dense"))
            assert int(peak.item()) & 0xFFFFFFFF == int(np.max(np.abs(got)))


@pytest.mark.parametrize("name,bits", [("ragged_ends", 32), ("nine_rise_at_5", 16), ("narrow_mix_rises", 32)])
def test_chain_with_dense_odd_stems(dev, golden_dir, name, bits):
    """every stem one sample shorter where its length is even would change the case: instead the stems are handed over as dense views whose
    second rows start off the grid (an odd row stride)"""
    from audiolab_amd import merge
    g = chain_fixture(golden_dir, name, bits)
    stems, widths, rates, _ = make_chain(name, bits)
    dense = []
    for s in stems:
        buf = torch.zeros((s.shape[0], s.shape[1] + 1 + s.shape[1] % 2), dtype=torch.float32, device=dev.device)   # an odd stride
        buf[:, :s.shape[1]] = on(dev, s)
        dense.append(buf[:, :s.shape[1]])
        assert dense[-1].stride(0) % 2 == 1
    acc, peak, _ = merge.mix_sum_rates(dev, dense, widths, rates, bits)
    assert np.array_equal(host(acc).astype(np.int64), g["acc"]) and peak == g["peak"]


# ---- 5. equal rates: today's path, bit for bit -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,bits", [("three_ragged", 32), ("nine_stems", 16), ("hot", 32)])
def test_equal_rates_change_nothing(dev, name, bits):
    from audiolab_amd import merge
    assert (name, bits) in VARIANTS
    stems, widths, source, source_width, prevent = make_case(name, bits)

    def mix(**kw):
        return merge.mixdown_array([on(dev, s) for s in stems], (on(dev, source), source_width), prevent_clipping=prevent, bits=bits,
                                   src_bits=widths, ctx=dev, **kw)
    dev.launch_counts_reset()
    plain, rec = mix()
    launches = dev.launch_count("mix_sum_kernel")
    dev.launch_counts_reset()
    same, rec_r = mix(rates=[44100] * len(stems))
    assert dev.launch_count("mix_sum_kernel") == launches and dev.launch_count("mix_sum_rate_kernel") == 0
    assert np.array_equal(host(same), host(plain))
    assert rec.rate == 0 and rec_r.rate == 44100
    rec_r.rate = 0
    assert rec_r == rec


# ---- 6. argument errors ---------------------------------------------------------------------------------------------------------------
def test_argument_errors(dev):
    from audiolab_amd import _lib, merge
    from audiolab_amd._lib import AlsepError
    lib = dev.lib
    n, k = 400, ratecv_length(400, 44100, 48000)
    x = torch.zeros((2, n), device=dev.device)
    mix = torch.full((2, n), 7, dtype=torch.int32, device=dev.device)
    acc = torch.full((2, k), -5, dtype=torch.int32, device=dev.device)
    peak = torch.full((1,), -5, dtype=torch.int32, device=dev.device)

    def call(data=None, in_rate=44100, out_rate=48000, width=32, is_mix=0, n_out=k, out=acc, bits=32, count=1, channels=2, n_in=n):
        data = x if data is None else data
        ops = (_lib.MixOperand * 9)(*[_lib.MixOperand(data.data_ptr(), n_in, n_in, in_rate, out_rate, 2, width, is_mix)] * 9)
        return lib.alsep_mix_sum_rates(dev.handle, ops, count, channels, n_out, bits, out.data_ptr(), out.shape[1], peak.data_ptr())
    assert call(in_rate=0) == -1 and call(out_rate=0) == -1 and call(in_rate=-44100) == -1 and call(out_rate=-1) == -1
    assert call(in_rate=-3, out_rate=-3) == -1
    assert call(in_rate=1048577, out_rate=1048576) == -1 and call(in_rate=3, out_rate=2097152) == -1     # reduced rates above 2^20
    assert call(width=24) == -1 and call(width=8) == -1                      # no grid to resample on
    assert call(n_out=k - 1) == -1 and call(n_out=k + 1) == -1 and call(n_out=n) == -1                     # not ratecv_length
    assert call(count=0) == -1 and call(count=9) == -1 and call(channels=3) == -1 and call(bits=24) == -1
    assert call(data=mix, is_mix=1, count=2) == -1                           # the mix is operand 0 only
    # a resampled mix that is acc itself, or overlaps it
    wide = torch.full((2, k), 7, dtype=torch.int32, device=dev.device)       # n samples per row, row stride k: it becomes k samples per row
    alias = (_lib.MixOperand * 1)(_lib.MixOperand(wide.data_ptr(), n, k, 44100, 48000, 2, 32, 1))
    assert lib.alsep_mix_sum_rates(dev.handle, alias, 1, 2, k, 32, wide.data_ptr(), k, peak.data_ptr()) == -1
    big = torch.zeros((2 * k + 2 * n,), dtype=torch.int32, device=dev.device)
    inside = big[8:8 + 2 * n].view(2, n)
    assert lib.alsep_mix_sum_rates(dev.handle, (_lib.MixOperand * 1)(_lib.MixOperand(inside.data_ptr(), n, n, 44100, 48000, 2, 32, 1)), 1, 2, k, 32,
                                   big.data_ptr(), k, peak.data_ptr()) == -1
    dev.synchronize()
    assert (host(acc) == -5).all() and (host(mix) == 7).all() and (host(wide) == 7).all() and not host(big).any() and int(peak.item()) == -5     # nothing was written
    # what is allowed: a resampled mix into another buffer, the mix as it is in place, equal rates with any width
    assert call(data=mix, is_mix=1) == 0
    assert call(data=mix, is_mix=1, in_rate=0, out_rate=0, n_out=n, out=mix) == 0
    assert call(in_rate=48000, out_rate=48000, width=24, n_out=n, out=mix) == 0
    dev.synchronize()
    assert lib.alsep_mix_ratecv_length(0, 1, 1) == -1 and lib.alsep_mix_ratecv_length(5, 0, 1) == -1 and lib.alsep_mix_ratecv_length(5, 1, -2) == -1
    assert lib.alsep_mix_ratecv_length(5, 1048577, 1048576) == -1 and lib.alsep_mix_ratecv_length(5, 2097152, 2097150) == 4
    # the Python layer
    with pytest.raises(AlsepError):
        merge.ratecv_array(x, 0, 48000, 32, ctx=dev)
    with pytest.raises(AlsepError):
        merge.ratecv_array(x, 44100, 48000, 24, ctx=dev)
    with pytest.raises(AlsepError):
        merge.ratecv_length(10, 1048577, 1048576)
    with pytest.raises(AlsepError):                                          # width 24 with a rate pair
        merge.mixdown_array([x, x], 0.0, src_bits=[32, 24], rates=[48000, 44100], ctx=dev)
    with pytest.raises(AlsepError):
        merge.mixdown_array([x, x], 0.0, rates=[48000, -1], ctx=dev)
    with pytest.raises(AlsepError):
        merge.mixdown_array([x, x], 0.0, rates=[48000], ctx=dev)


# ---- 7. CPU only ----------------------------------------------------------------------------------------------------------------------
def test_numpy_restatement_reproduces_the_fixture(golden_dir):
    """keeps tests/golden/merge_rates.npz auditable where ``audioop`` is absent (Python 3.13 and later)"""
    for pair in PAIRS:
        for width in WIDTHS:
            for channels in CHANNELS:
                for n in LENGTHS:
                    u = quantise(ratecv_input(pair, width, channels, n), width, width)
                    expect_ratecv(np_ratecv(u, width, *pair), u, ratecv_fixture(golden_dir, pair, width, channels, n), (pair, width, channels, n))
    for name, bits in CHAIN_VARIANTS:
        g = chain_fixture(golden_dir, name, bits)
        stems, widths, rates, source = make_chain(name, bits)
        r = reference_mix_rates(stems, widths, rates, bits, source, True, NUMPY_RATE_OPS)
        assert np.array_equal(r["acc"], g["acc"]) and np.array_equal(r["y2"], g["y2"])
        assert (r["rate"], r["peak"], r["peak1"], r["rms"], r["f1"], r["f2"]) == (g["rate"], g["peak"], g["peak1"], g["rms"], g["f1"], g["f2"])


def test_the_cases_cover_what_they_claim():
    assert len(CHAINS["nine_rise_at_5"]["stems"]) == 9 and CHAINS["nine_rise_at_5"]["stems"][4][4] > CHAINS["nine_rise_at_5"]["stems"][3][4]
    n_mix = ratecv_length(CHAINS["ragged_ends"]["stems"][0][1], 44100, 48000)
    ends = [ratecv_length(n, r, 48000) for _, n, _, _, r in CHAINS["ragged_ends"]["stems"][1:]]
    assert any(e < n_mix for e in ends[:2]) and any(e > n_mix for e in ends[:2]) and any(e < n_mix for e in ends[2:]) and any(e > n_mix for e in ends[2:])


def test_plan_rates():
    from audiolab_amd.merge import AlsepError, plan_rates

    def shape(plan):
        return [(p.mix, p.mix_width, p.stems, p.rate, p.length) for p in plan]
    # equal: one launch, nothing resampled
    assert shape(plan_rates([44100] * 3, [32] * 3, 0, 100)) == [(None, 0, [(0, None), (1, None), (2, None)], 44100, 100)]
    # falling: one launch, the later stems carry their pair
    assert shape(plan_rates([48000, 44100, 40000], [32, 16, 32], 0, 100)) == \
        [(None, 0, [(0, None), (1, (44100, 48000)), (2, (40000, 48000))], 48000, 100)]
    # rising: every rise is a launch boundary, the mix carries the pair on the grid of the widest stem in it
    assert shape(plan_rates([22050, 44100, 48000], [16, 32, 16], 0, 1001)) == \
        [(None, 0, [(0, None)], 22050, 1001), ((22050, 44100), 16, [(1, None)], 44100, 2001), ((44100, 48000), 32, [(2, None)], 48000, 2177)]
    # the length is optional
    assert [p.length for p in plan_rates([22050, 44100], [16, 16])] == [None, None]
    # nine stems, the rise at the fifth: 4, then the mix + 5; with the mix a launch holds 7 stems at most
    rates = [44100] * 4 + [48000, 44100, 48000, 40000, 48000]
    plan = plan_rates(rates, [32] * 9, 0, 2049)
    assert [[k for k, _ in p.stems] for p in plan] == [[0, 1, 2, 3], [4, 5, 6, 7, 8]] and plan[1].mix == (44100, 48000)
    assert plan[1].stems[1] == (5, (44100, 48000)) and plan[1].stems[3] == (7, (40000, 48000)) and plan[1].length == 2230
    plan = plan_rates(rates, [32] * 9, 2)
    assert [[k for k, _ in p.stems] for p in plan] == [[0, 1], [2, 3], [4, 5], [6, 7], [8]]
    assert [p.mix for p in plan] == [None, (44100, 44100), (44100, 48000), (48000, 48000), (48000, 48000)]
    plan = plan_rates([48000] * 9 + [96000] + [48000] * 9, [16] * 19)
    assert [len(p.stems) for p in plan] == [8, 1, 7, 3] and [p.mix for p in plan] == [None, (48000, 48000), (48000, 96000), (96000, 96000)]
    assert all(len(p.stems) <= 3 for p in plan_rates(rates, [32] * 9, 3))
    for bad in ([], [0, 44100], [44100, -1]):
        with pytest.raises(AlsepError):
            plan_rates(bad, [32] * len(bad))
    with pytest.raises(AlsepError):
        plan_rates([44100], [32, 32])
