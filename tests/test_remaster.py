"""audiolab_amd.master (csrc/master.h, the ``alsep_master_*`` entry points) on the emulated kernels (-m "not gpu") and on the GPU (-m gpu), same
bodies, against tests/remaster_oracle.py -- scipy's own stft, fftconvolve, filtfilt, lfilter, butter, maximum_filter1d and interp1d.

Stage tests hand the ORACLE's input of a stage to the entry point under test and compare every element, nothing masked.

Tolerance of a float64 stage: max|ours - want| <= 1e-12 max|want|.  Each stage is a sum of at most a few thousand products per output (a
256 .. 4096-point transform, a block of an overlap-save convolution, a geometric sum with ratio up to 0.999962, whose terms and partial
sums never exceed the output's own peak by more than a small factor), so it rounds by about 1e-16 * log2(terms) * O(10) < 1e-14; scipy's
own lfilter differs from an extended-precision recurrence by 3.7e-15 of the peak for the release pole at n = 40000.  The bound keeps a
margin of a hundred or more over both, and a single-precision stage (6e-8) cannot pass, on purpose.

Selections (sliding maxima) and the PCM24 pack of our own float64 result are compared bit for bit with numpy.

The loudest-piece mask is a threshold on values that differ from the oracle's in the last bits, so every multi-piece input used here is
first checked, on the oracle, to keep each piece's RMS more than 1e-6 (relative) away from the average."""
import numpy as np
import pytest
import torch

from tests import remaster_oracle as ro
from tests.conftest import host, on

SR = 44100
THRESHOLD = (2 ** 15 - 61) / 2 ** 15
SMALL = dict(n_fft=256, P=3000)
STAGE = 1e-12
# remaster_arrays against the oracle, relative to the peak: 16 times the largest figure measured over CASES on the emulated kernels
# (1.9e-14, see test_end_to_end); far below the 6e-8 of a single-precision stage
END_TO_END = 16 * 1.9e-14

_ORACLE = {}


def signal(n: int, seed: int, gain: float = 1.0, channels: int = 2, spikes: int = 0, spike_gain: float = 1.0) -> np.ndarray:
    """noise plus two sines under a slow envelope, [n, channels] (or [n] for channels = 0); ``spikes`` short bursts raise the crest
    factor, so that the level-matched track rises above the threshold and the limiter has work"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / SR
    env = 0.55 + 0.45 * np.sin(2 * np.pi * 1.3 * np.arange(n) / n + seed)
    rows = []
    for c in range(max(channels, 1)):
        x = env * (0.08 * rng.standard_normal(n) + 0.3 * np.sin(2 * np.pi * 440.0 * t + c) + 0.2 * np.sin(2 * np.pi * 3613.7 * t + 1.0 + 0.5 * c))
        for s in range(spikes):
            at = int((s + 0.37) * n / spikes)
            width = min(40, n - at)
            x[at:at + width] += spike_gain * (1.6 if c == 0 else 1.1) * np.hanning(40)[:width] * np.cos(0.9 * np.arange(width))
        rows.append(gain * x)
    return rows[0] if channels == 0 else np.stack(rows, axis=1)


# name -> (target, reference, config); both at 44.1 kHz
def _cases():
    big = dict(n_fft=4096, P=3 * 4096 + 5)
    return {
        "4 pieces with a tail of 3 against 5": (signal(10007, 1, 0.9, spikes=5), signal(12000, 2, 0.5), SMALL),     # d = 4, p = 2501; d = 5, p = 2400
        "one piece against one frame": (signal(2999, 3, 0.9, spikes=1, spike_gain=2.0), signal(256, 13, 0.5), SMALL),
        "one frame against 4 pieces": (signal(256, 5, 0.7, spikes=1), signal(9001, 6, 0.5), SMALL),
        "n_fft 4096": (signal(3 * 4096 + 5, 7, 0.9, spikes=4), signal(3 * 4096 + 5, 8, 0.5), big),                   # d = 2, p = 6146: one frame per piece
        "mono": (signal(5000, 9, 0.9, channels=0, spikes=3), signal(7000, 10, 0.5, channels=0), SMALL),
        "nothing to limit": (signal(7000, 11, 0.5), signal(7000, 11, 0.5), SMALL),
    }


CASES = _cases()


def oracle(name):
    """computed once per case, shared, read-only"""
    if name not in _ORACLE:
        t, r, cfg = CASES[name]
        _ORACLE[name] = ro.remaster(t, r, ro.Config(**cfg))
    return _ORACLE[name]


def ours(dev, name, **kw):
    from audiolab_amd import master
    t, r, cfg = CASES[name]
    return master.remaster_arrays((on(dev, t), SR), (on(dev, r), SR), master.MasterConfig(**cfg), ctx=dev, want_stages=True, **kw)


def vec(dev, a):
    return on(dev, np.ascontiguousarray(a, dtype=np.float64))


def check(got, want, label, bound=STAGE):
    got = host(got) if isinstance(got, torch.Tensor) else np.asarray(got)
    assert got.dtype == np.float64 and got.shape == want.shape, label
    err, peak = float(np.max(np.abs(got - want))), float(np.max(np.abs(want)))
    print(f"{label}: max|ours - want| = {err:.3e} = {err / peak if peak else 0.0:.3e} of the peak (bound {bound:.1e})")
    assert np.all(np.isfinite(got)) and err <= bound * peak, label
    return err / peak if peak else 0.0


def test_the_masks_are_decided_with_room():
    seen = 0
    for name in CASES:
        w = oracle(name)
        for r, avg in ((w["tgt_r"], w["tgt_avg"]), (w["ref_r"], w["ref_avg"])):
            if len(r) > 1:
                seen += 1
                margin = float(np.min(np.abs(r - avg)) / avg)
                print(f"{name}: {len(r)} pieces, nearest to the average by {margin:.3e}")
                assert margin > 1e-6
    assert seen >= 5


# ---- stages -------------------------------------------------------------------------------------------------------------------------------
def test_mid_side_left_right_peak(dev):
    from audiolab_amd import master
    x = signal(1234, 20, 0.8)
    lr = vec(dev, x.T)
    assert master.peak(dev, lr) == float(np.max(np.abs(x)))
    assert master.peak(dev, lr[1].contiguous()) == float(np.max(np.abs(x[:, 1])))
    div = 0.37
    mid, side = ro.mid_side(x / div)
    ms = master.mid_side(dev, lr, div)
    assert np.array_equal(host(ms), np.stack([mid, side]))
    check(master.left_right(dev, ms, 1.7), np.stack([mid * 1.7 + side * 1.7, mid * 1.7 - side * 1.7]), "left / right")


@pytest.mark.parametrize("n", [10007, 12000, 2999, 256])
def test_piece_sums(dev, n):
    from audiolab_amd import master
    mid = signal(n, 21, 2.5, channels=0)                                     # above 1, so that the clip matters
    d, p = ro.geometry(n, 3000)
    assert master.geometry(n, 3000) == (d, p)
    check(master.piece_sumsq(dev, vec(dev, mid), d, p), ro.piece_sumsq(mid, 3000), f"{d} pieces of {p}")
    want = ro.piece_sumsq(np.clip(mid * 0.9, -1.0, 1.0), 3000)
    assert np.max(np.abs(mid * 0.9)) > 1.0
    check(master.piece_sumsq(dev, vec(dev, mid), d, p, 0.9, clip=True), want, f"{d} pieces of {p}, clipped")
    idx, rms = master.loudest(want, p)
    mask, want_rms, _, _ = ro.loudest(want, p)
    assert np.array_equal(idx, np.nonzero(mask)[0]) and rms == want_rms and (d > 1 or list(idx) == [0])


@pytest.mark.parametrize("n,n_fft,P,pieces", [(10007, 256, 3000, [0, 2, 3]), (12000, 256, 3000, [1]), (256, 256, 3000, [0]),
                                              (3 * 4096 + 5, 4096, 3 * 4096 + 5, [0, 1]), (2 * 1024 + 100, 1024, 3000, [0]),
                                              (8192 * 2, 8192, 8192 * 3, [0])])
def test_average_spectrum(dev, n, n_fft, P, pieces):
    from audiolab_amd import master
    x = signal(n, 22, 0.8)
    mid, side = ro.mid_side(x)
    d, p = ro.geometry(n, P)
    mask = np.zeros(d, dtype=bool)
    mask[pieces] = True
    k0 = 1.37
    want = np.stack([ro.average_spectrum(mid * k0, P, mask, n_fft), ro.average_spectrum(side * k0, P, mask, n_fft)])
    got = master.average_spectrum(dev, vec(dev, np.stack([mid, side])), p, pieces, n_fft, k0)
    check(got, want, f"n {n}, n_fft {n_fft}, pieces {pieces} of {d}")


# n_fir = 256: block exponent 9, 257 new samples per block; 255 taps (odd): 258
@pytest.mark.parametrize("n,taps,log2_block,per", [(100, 256, 9, 0), (257, 256, 9, 0), (1000, 256, 9, 2), (1000, 256, 9, 0), (999, 255, 9, 3),
                                                   (5000, 256, 0, 0), (3 * 4096 + 5, 4096, 13, 1)])
def test_convolve_same(dev, n, taps, log2_block, per):
    from audiolab_amd import master
    rng = np.random.default_rng(23)
    x = signal(n, 23, 0.8).T
    fir = rng.standard_normal((2, taps)) * np.hanning(taps)
    want = np.stack([ro.convolve_same(x[c], fir[c]) for c in range(2)]) * 1.3
    got = master.convolve_same(dev, vec(dev, x), vec(dev, fir), 1.3, log2_block, per)
    check(got, want, f"n {n}, {taps} taps, block 2^{log2_block}, {per} blocks per batch")


@pytest.mark.parametrize("n,w", [(89, 45), (1000, 45), (9000, 4095), (20000, 4096), (300, 1)])
def test_sliding_maxima_bit_for_bit(dev, n, w):
    from audiolab_amd import master
    g = np.abs(signal(n, 24, 1.0, channels=0)) ** 3
    x = vec(dev, g)
    assert np.array_equal(host(master.slide_max(dev, x, w, True)), ro.slide_max_centred(g, w))
    assert np.array_equal(host(master.slide_max(dev, x, w, False)), ro.slide_max_trailing(g, w))


def _filters():
    cfg = ro.Config()
    _, ba, aa = ro.attack_coefficients(cfg)
    _, hold, release = ro.hold_release_coefficients(cfg)
    return {"attack": (ba, aa), "hold": hold, "release": release, "two taps, negative pole": ([0.3, -0.2], [1.0, 0.6])}


# (5000, 1): 5000 chunk ends, more than one chunk of the carry pass, which is scanned in its turn
@pytest.mark.parametrize("n,chunk", [(200, 64), (7, 0), (7, 3), (40000, 0), (8193, 4096), (1, 0), (5000, 1)])
def test_first_order_iir(dev, n, chunk):
    from scipy import signal as ss
    from audiolab_amd import master
    x = np.abs(signal(n, 25, 1.0, channels=0))
    for name, (b, a) in _filters().items():
        for zi in (0.0, 0.4):
            want = ss.lfilter(b, a, x, zi=[zi])[0]
            check(master.iir(dev, vec(dev, x), b, a, zi, False, chunk), want, f"{name}, n {n}, chunk {chunk}, zi {zi}")
            back = ss.lfilter(b, a, x[::-1], zi=[zi])[0][::-1]
            check(master.iir(dev, vec(dev, x), b, a, zi, True, chunk), back, f"{name} backwards, n {n}, chunk {chunk}, zi {zi}")


@pytest.mark.parametrize("n,chunk", [(200, 64), (7, 0), (40000, 0), (1000, 1000)])
def test_filtfilt(dev, n, chunk):
    from scipy import signal as ss
    from audiolab_amd import master
    x = np.abs(signal(n, 26, 1.0, channels=0))
    for name, (b, a) in _filters().items():
        check(master.filtfilt(dev, vec(dev, x), b, a, chunk), ss.filtfilt(b, a, x), f"filtfilt {name}, n {n}, chunk {chunk}")


@pytest.mark.parametrize("name", ["4 pieces with a tail of 3 against 5", "n_fft 4096"])
def test_limiter_stages(dev, name):
    """the oracle's pre-limiter signal through our limiter, curve by curve, then each filter alone on the oracle's own input"""
    from audiolab_amd import master
    w = oracle(name)
    lim = w["limiter"]
    assert lim["ran"]
    cfg = master.MasterConfig(**CASES[name][2])
    lr = vec(dev, w["pre_limiter"].T)
    g, over = master.rectify(dev, lr, cfg.threshold)
    assert over
    check(g, lim["g"], "g")
    wa, ba, aa = ro.attack_coefficients(ro.Config())
    wh, hold, release = ro.hold_release_coefficients(ro.Config())
    assert np.array_equal(host(master.slide_max(dev, vec(dev, lim["g"]), wa, True)), lim["s_a"])
    assert np.array_equal(host(master.slide_max(dev, vec(dev, lim["g"]), wh, False)), lim["s_h"])
    check(master.filtfilt(dev, vec(dev, lim["s_a"]), ba, aa), lim["g_a"], "g_a")
    check(master.iir(dev, vec(dev, lim["s_h"]), *hold), lim["h"], "h")
    check(master.iir(dev, vec(dev, lim["rel_in"]), *release), lim["rel"], "rel")
    stages = {}
    out, gain, ran, peak = master.limit(dev, lr, cfg, stages=stages)
    assert ran and peak == float(np.max(np.abs(host(out))))
    check(gain, lim["gain"], "gain")
    check(out, lim["out"].T, "limited")
    assert peak <= cfg.threshold * (1 + 1e-12)


def test_limiter_bypass(dev):
    from audiolab_amd import master
    cfg = master.MasterConfig(**SMALL)
    x = signal(3000, 27, 0.5).T
    x *= cfg.threshold * (1.0 + 5e-6) / np.max(np.abs(x))                    # numpy.isclose(rect, 1) still holds at 5e-6
    lr = vec(dev, x)
    g, over = master.rectify(dev, lr, cfg.threshold)
    assert not over and np.all(np.isclose(ro.rectify(x.T, cfg.threshold), 1.0))
    out, gain, ran, peak = master.limit(dev, lr, cfg)
    assert out is lr and gain is None and not ran and np.array_equal(host(out), x)
    x[1, 1234] = -cfg.threshold * (1.0 + 2e-5)
    assert master.rectify(dev, vec(dev, x), cfg.threshold)[1] and not np.all(np.isclose(ro.rectify(x.T, cfg.threshold), 1.0))


def test_pcm24_bit_for_bit(dev):
    from audiolab_amd import master
    x = signal(4001, 28, 1.0).T
    x[0, :8] = [1.5, -1.5, 0.5 / 8388607.0, 1.5 / 8388607.0, 2.5 / 8388607.0, -0.5 / 8388607.0, 1.0, -1.0]   # the clip and ties to even
    div = 0.83
    res, pcm = master.pcm24(dev, vec(dev, x), div)
    assert np.array_equal(host(res), x / div)
    assert host(pcm).tobytes() == ro.pcm24((x / div).T)
    assert host(pcm)[:3].tolist() == [255, 255, 127] and host(pcm)[6:9].tolist() == [1, 0, 128]     # +/- 8388607, little-endian


# ---- the chain ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_end_to_end(dev, name):
    """Plumbing: coefficients, piece geometry, stage order.  Measured on the emulated kernels, ours against the oracle relative to the
    peak of the result, over CASES in order: 7.9e-16, 1.0e-15, 1.9e-14, 2.3e-15, 6.1e-16, 7.8e-16.  The bound END_TO_END is 16 times the
    largest, 3.0e-13, below 1e-10.  The one figure above 3e-15 belongs to the target of a single frame: its spectrum is one |rfft|, not
    an average, with bins down to 3e-5 of the peak, and the quotient A_ref / A_tgt of step 5 divides by them -- the mid FIR already
    differs by 1.5e-14 there, everything after it carries that."""
    got, want = ours(dev, name), oracle(name)
    st = got.stages
    assert got.limited == want["ran"] == (name != "nothing to limit")
    assert abs(got.k0 - want["k0"]) <= 1e-12 * want["k0"]
    assert len(got.coefficients) == 4 and all(abs(a - b) <= 1e-12 * b for a, b in zip(got.coefficients, want["coefficients"]))
    check(st["tgt_sumsq"], want["tgt_sumsq"], "target's piece sums")
    check(st["ref_sumsq"], want["ref_sumsq"], "reference's piece sums")
    check(st["tgt_spectrum"], np.stack([want["spectra"]["tgt_mid"], want["spectra"]["tgt_side"]]), "target's spectra", END_TO_END)
    check(st["ref_spectrum"], np.stack([want["spectra"]["ref_mid"], want["spectra"]["ref_side"]]), "reference's spectra", END_TO_END)
    check(got.fir_mid, want["fir_mid"], "mid FIR", END_TO_END)
    if name == "mono":
        # both side spectra are exactly zero in the oracle, M = 0 / min_value = 0; ours are the rounding of one complex transform shared
        # with mid (1e-17), which the division by min_value = 1e-6 raises to 1e-11: a filter of noise, applied to a channel of zeros
        assert not np.any(want["fir_side"]) and np.max(np.abs(got.fir_side)) <= 1e-9 and not np.any(host(st["conv"])[1])
    else:
        check(got.fir_side, want["fir_side"], "side FIR", END_TO_END)
    check(st["conv"], want["conv"], "mid / side after the FIR", END_TO_END)
    check(st["pre_limiter"], want["pre_limiter"].T, "before the limiter", END_TO_END)
    check(st["gain"], want["gain"], "gain", END_TO_END)
    check(got.result, want["result"].T, "result", END_TO_END)
    res = host(got.result)
    peak = float(np.max(np.abs(res)))
    assert peak <= THRESHOLD * (1 + 1e-12)
    if got.limited:
        assert peak >= THRESHOLD * (1 - 1e-12)
    assert got.pcm24_bytes() == ro.pcm24(res.T)
    assert tuple(got.pcm24.shape) == (6 * res.shape[1],) and got.sample_rate == SR


def test_a_silent_target(dev):
    from audiolab_amd import master
    got = master.remaster_arrays((on(dev, np.zeros((3000, 2))), SR), (on(dev, signal(3000, 30, 0.5)), SR), master.MasterConfig(**SMALL), ctx=dev)
    assert not got.limited and np.all(np.isfinite(host(got.result))) and not np.any(host(got.result)) and not np.any(host(got.pcm24))
    assert np.isfinite(got.k0) and np.all(np.isfinite(got.coefficients)) and np.all(np.isfinite(got.fir_mid))


def test_a_48_khz_reference(dev):
    from scipy.signal import resample
    from audiolab_amd import master
    t, r48 = signal(6000, 31, 0.9, spikes=3), signal(7200, 32, 0.5)
    r = np.stack([resample(r48[:, c], int(7200 * SR / 48000)) for c in range(2)], axis=1)
    want = ro.remaster(t, r, ro.Config(**SMALL))
    got = master.remaster_arrays((on(dev, t), SR), (on(dev, r48), 48000), master.MasterConfig(**SMALL), ctx=dev)
    assert got.limited and want["ran"]
    check(got.result, want["result"].T, "result with a resampled reference", END_TO_END)


LAUNCHES = ("ms_peak_partial_kernel", "ms_midside_kernel", "pack_rows_kernel", "ms_piece_partial_kernel", "ms_slide_max_kernel",
            "ms_iir_local_kernel", "ms_odd_ext_kernel", "ola_gather_kernel", "ms_spectrum_kernel", "ms_rectify_kernel", "ms_pcm24_kernel")


def test_errors_come_before_any_launch(dev):
    from audiolab_amd import master
    from audiolab_amd._lib import AlsepError
    cfg = master.MasterConfig(**SMALL)
    ok = on(dev, signal(3000, 33, 0.5))
    dev.launch_counts_reset()
    for bad_t, bad_r, c in ((on(dev, signal(255, 34)), ok, cfg), (ok, on(dev, signal(255, 34)), cfg), (ok, on(dev, np.zeros((3000, 3))), cfg),
                            (ok, ok, master.MasterConfig(n_fft=256, P=3000, max_length_s=0.05)), (ok, on(dev, signal(3000 * 64, 35)), cfg)):
        with pytest.raises(ValueError):
            master.remaster_arrays((bad_t, SR), (bad_r, SR), c, ctx=dev)
    with pytest.raises(ValueError):
        master.remaster_arrays((ok, 0), (ok, SR), cfg, ctx=dev)
    for kw in (dict(n_fft=300), dict(n_fft=128), dict(n_fft=16384), dict(n_fft=4096, P=3000), dict(attack=200.0), dict(threshold=0.0)):
        with pytest.raises(ValueError):
            master.MasterConfig(**kw)
    x = vec(dev, np.abs(signal(88, 36, channels=0)))
    with pytest.raises(AlsepError, match="2 w - 1"):
        master.slide_max(dev, x, 45, True)
    with pytest.raises(AlsepError, match="2 w - 1"):
        master.slide_max(dev, x, 45, False)
    with pytest.raises(AlsepError):
        master.slide_max(dev, x, 4097, True)
    with pytest.raises(AlsepError, match="padding"):
        master.filtfilt(dev, vec(dev, np.ones(6)), [0.1], [1.0, -0.9])
    with pytest.raises(AlsepError):
        master.iir(dev, x, [0.1], [1.0, -0.9], chunk=8193)
    with pytest.raises(AlsepError):
        master.iir(dev, x, [0.1], [1.0, -1.5])
    with pytest.raises(AlsepError):
        master.convolve_same(dev, vec(dev, np.ones((1, 100))), vec(dev, np.ones((1, 256))), log2_block=8)
    with pytest.raises(AlsepError):
        master.average_spectrum(dev, vec(dev, np.ones((2, 3000))), 1000, [3], 256)       # piece 3 of 3
    with pytest.raises(AlsepError):
        master.average_spectrum(dev, vec(dev, np.ones((2, 3000))), 200, [0], 256)        # a piece shorter than a frame
    assert [dev.launch_count(k) for k in LAUNCHES] == [0] * len(LAUNCHES)


def test_chunk_and_batch_do_not_matter(dev):
    name = "4 pieces with a tail of 3 against 5"
    whole = ours(dev, name)
    assert whole.limited
    for kw in (dict(chunk=64), dict(chunk=1000), dict(blocks_per_batch=1), dict(blocks_per_batch=3)):
        other = ours(dev, name, **kw)
        check(other.result, host(whole.result), f"{kw}")
        check(other.stages["gain"], host(whole.stages["gain"]), f"gain, {kw}")


@pytest.mark.parametrize("channels", [1, 2])
def test_wavio_24_bit(tmp_path, channels):
    from audiolab_amd import wavio
    x = signal(1001, 37, 1.2, channels=2)[:, :channels].T
    path = str(tmp_path / "a.wav")
    wavio.write_wav(path, x, 48000, subtype="PCM_24")
    assert wavio.read_wav_info(path) == (channels, 48000, 24, False)
    grid = np.clip(np.rint(x * 8388607.0), -8388607, 8388607)
    back, rate = wavio.read_wav_interleaved(path)
    assert rate == 48000 and np.array_equal(back.reshape(-1, channels).T * 8388608.0, grid)
    ints = np.array([[-(1 << 23), (1 << 23) - 1, 0, -1, 1 << 24]], dtype=np.int64)   # integers are the samples themselves, clipped to the range
    wavio.write_wav(path, ints, 44100, subtype="PCM_24")
    assert np.array_equal(wavio.read_wav_interleaved(path)[0] * 8388608.0, [-(1 << 23), (1 << 23) - 1, 0, -1, (1 << 23) - 1])
    wavio.write_wav(path, ints.astype(np.int32)[:, :4], 44100, subtype="PCM_24")
    assert np.array_equal(wavio.read_wav_interleaved(path)[0] * 8388608.0, [-(1 << 23), (1 << 23) - 1, 0, -1])
    with pytest.raises(ValueError):                                          # a type that cannot hold the 24-bit grid: samples of another width
        wavio.write_wav(path, np.array([[1, 2]], dtype=np.int16), 44100, subtype="PCM_24")


def test_remaster_file(dev, tmp_path):
    from audiolab_amd import master, wavio
    t, r = signal(5000, 38, 0.6, spikes=2), signal(4000, 39, 0.4, channels=0)
    tp, rp, op = (str(tmp_path / f) for f in ("t.wav", "r.wav", "o.wav"))
    wavio.write_wav(tp, t.T, SR, subtype="PCM_16")
    wavio.write_wav(rp, r, SR, subtype="FLOAT")
    cfg = master.MasterConfig(**SMALL)
    res = master.remaster_file(tp, rp, op, cfg, ctx=dev)
    assert wavio.read_wav_info(op) == (2, SR, 24, False)
    t16 = np.clip(np.rint(t * 32768.0), -32768, 32767) / 32768.0
    ref = master.remaster_arrays((on(dev, t16), SR), (on(dev, r.astype(np.float32).astype(np.float64)), SR), cfg, ctx=dev)
    assert res.pcm24_bytes() == ref.pcm24_bytes()
    back, _ = wavio.read_wav_interleaved(op)
    assert np.array_equal(back.reshape(-1, 2).T * 8388608.0, np.rint(host(res.result) * 8388607.0))
