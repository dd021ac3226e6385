"""The pitch shifter (audiolab_amd/pitch.py -> csrc/pitch.h ``alsep_pitch_shift``) on the emulated kernels (-m "not gpu") and on the GPU
(-m gpu), same bodies, against tests/pitch_oracle.py: the specification in numpy float64.  The reference shifts with ffmpeg's rubberband
filter, which is not available: parity with it is unpinned, the oracle is the project's own.

Tolerance: max|ours - oracle| <= 2^-24 max(1, max|oracle|), every sample.  The rounding to float32 costs at most half an ulp, <= 2^-25
below 1; the rest is left to the float64 chain (transforms, atan2, sincos, the Bessel series: ~1e-13 here).  A single-precision
transform does not pass, on purpose.  The peak and owner decisions are discontinuous; on the noisy inputs used here a 1e-13 relative
perturbation of the input moves the oracle's output by <= 3.3e-14, so they are stable.

The shortest signal, N = 1, is shifted by -24 and -13 semitones only: with an analysis hop above n_fft / 2 (r < 1/2) the sample lies in
frame 0 alone.  At a smaller hop a later frame holds nothing but that one sample; its magnitude spectrum is flat, every comparison
of the peak search is a tie in exact arithmetic and is decided by the last bit of the transform, in the oracle as in the kernels --
the specification fixes no value there, so there is nothing to compare (shape and finiteness are still checked at +7)."""
import numpy as np
import pytest
import torch

from tests import pitch_oracle as po
from tests.conftest import host, on

ULP = 2.0 ** -24
SR = 8000
_ORACLE = {}
_OURS = {}


def signal(channels: int, n: int, seed: int = 5, sr: int = SR) -> np.ndarray:
    """0.1 N(0, 1) noise plus two sines"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / sr
    x = 0.1 * rng.standard_normal((channels, n)) + 0.3 * np.sin(2 * np.pi * 440.0 * t) + 0.2 * np.sin(2 * np.pi * 613.7 * t + 1.0)
    return x.astype(np.float32)


def oracle(key, x, s, n_fft):
    """computed once per case, shared, never modified"""
    k = (key, s, n_fft)
    if k not in _ORACLE:
        _ORACLE[k] = po.shift(x, s, n_fft)
        _ORACLE[k].setflags(write=False)
    return _ORACLE[k]


def ours(dev, key, x, s, n_fft, frames_per_batch=0):
    from audiolab_amd import pitch
    k = (dev.device.type, key, s, n_fft, frames_per_batch)
    if k not in _OURS:
        out = pitch.shift_pitch_array(on(dev, x), s, n_fft=n_fft, frames_per_batch=frames_per_batch, ctx=dev)
        assert out.dtype == torch.float32 and out.device.type == dev.device.type and tuple(out.shape) == np.atleast_2d(x).shape
        _OURS[k] = host(out)
    return _OURS[k]


def check(got, want, label):
    err = float(np.max(np.abs(got.astype(np.float64) - want)))
    bound = ULP * max(1.0, float(np.max(np.abs(want))))
    print(f"{label}: max|ours - oracle| = {err:.3e} (bound {bound:.3e}, peak {np.max(np.abs(want)):.3f})")
    assert np.all(np.isfinite(got)) and err <= bound


# n_fft 256: Stockham passes 8, 8, 4; 512: 8, 8, 8; 1024: 8, 8, 8, 2 -- every radix of the float64 transform (4096 is 8 x 4, 8192 ends in 2)
SHAPES = [((1, 3001), 256), ((2, 6000), 256), ((1, 3001), 512), ((1, 3001), 1024)]


@pytest.mark.parametrize("s", [7, -7, 24, -24, 1])
@pytest.mark.parametrize("shape,n_fft", SHAPES)
def test_against_the_oracle_every_sample(dev, shape, n_fft, s):
    x = signal(*shape)
    check(ours(dev, shape, x, s, n_fft), oracle(shape, x, s, n_fft), f"{shape} n_fft {n_fft} s {s:+d} [{dev.device.type}]")


def test_the_largest_frame(dev):
    """n_fft 8192: 4097 bins, the fifth bin per thread of the recurrence and its two LDS rows of 65 552 bytes; a transform ending in radix 2"""
    x = signal(1, 9001, seed=7)
    check(ours(dev, "n8192", x, 7, 8192, frames_per_batch=4), oracle("n8192", x, 7, 8192), f"n_fft 8192 [{dev.device.type}]")


@pytest.mark.parametrize("s", [7, -24])
def test_shorter_than_a_frame(dev, s):
    x = signal(1, 50, seed=6)
    check(ours(dev, "n50", x, s, 256), oracle("n50", x, s, 256), f"N = 50, s {s:+d} [{dev.device.type}]")


def test_one_sample(dev):
    x = np.array([[0.37]], dtype=np.float32)
    for s in (-24, -13):
        check(ours(dev, "n1", x, s, 256), oracle("n1", x, s, 256), f"N = 1, s {s:+d} [{dev.device.type}]")
    got = ours(dev, "n1", x, 7, 256)                                         # flat spectrum in frame 1: see the module docstring
    assert got.shape == (1, 1) and np.all(np.isfinite(got))


def test_silence_stays_silence(dev):
    x = np.zeros((2, 700), dtype=np.float32)
    for s in (5, -5):
        got = ours(dev, "zeros", x, s, 256)
        assert got.shape == (2, 700) and not np.any(got)
        check(got, oracle("zeros", x, s, 256), f"zeros, s {s:+d} [{dev.device.type}]")


@pytest.mark.parametrize("s", [24, -24])
def test_batching_changes_no_bit(dev, s):
    from audiolab_amd import pitch
    shape = (2, 6000)
    x = signal(*shape)
    whole = ours(dev, shape, x, s, 256).view(np.uint32)
    for fpb in (4, 7):
        assert np.array_equal(ours(dev, shape, x, s, 256, frames_per_batch=fpb).view(np.uint32), whole), f"frames_per_batch {fpb}"
    again = host(pitch.shift_pitch_array(on(dev, x), s, n_fft=256, frames_per_batch=7, ctx=dev))
    assert np.array_equal(again.view(np.uint32), whole)


def _peak_hz(seg: np.ndarray) -> float:
    """spectral peak of a Hann-weighted segment, parabolic interpolation on the log magnitude of a zero-padded transform"""
    nfft = 1 << 16
    m = np.abs(np.fft.rfft(seg * np.hanning(len(seg)), nfft))
    k = int(np.argmax(m))
    a, b, c = np.log(m[k - 1]), np.log(m[k]), np.log(m[k + 1])
    return (k + 0.5 * (a - c) / (a - 2 * b + c)) * SR / nfft


@pytest.mark.parametrize("s", [1, 4, 12, -5, -12, -24])
@pytest.mark.parametrize("f", [440.0, 613.7])
def test_a_sine_keeps_its_level_and_moves_by_the_ratio(dev, f, s):
    x = (0.5 * np.sin(2 * np.pi * f * np.arange(6000) / SR)).astype(np.float32)[None]
    got = ours(dev, ("sine", f), x, s, 256)[0].astype(np.float64)
    seg_in, seg_out = x[0, 1000:5000].astype(np.float64), got[1000:5000]
    hz, want_hz = _peak_hz(seg_out), f * 2.0 ** (s / 12.0)
    rms = np.sqrt(np.mean(seg_out ** 2)) / np.sqrt(np.mean(seg_in ** 2))
    print(f"{f} Hz, s {s:+d} [{dev.device.type}]: peak {hz:.3f} Hz (want {want_hz:.3f}), rms ratio {rms:.5f}")
    assert abs(hz - want_hz) <= 1.0
    assert abs(rms - 1.0) <= 0.005


def test_zero_semitones_returns_the_input(dev):
    from audiolab_amd import pitch
    x = signal(2, 300)
    out = pitch.shift_pitch_array(on(dev, x), 0, ctx=dev)
    assert out.dtype == torch.float32 and np.array_equal(host(out), x)
    assert tuple(pitch.shift_pitch_array(x[0], 0, ctx=dev).shape) == (1, 300)           # [N], host array
    audio = (x.T, SR)
    assert pitch.shift_pitch(audio, 0) is audio                                          # util/audio_track.py:626-627


def test_errors(dev):
    from audiolab_amd import _lib, pitch
    from audiolab_amd._lib import AlsepError
    x = signal(2, 600)
    for s in (25, -24.5, float("nan")):
        with pytest.raises(ValueError):
            pitch.shift_pitch_array(on(dev, x), s, n_fft=256, ctx=dev)
    for n_fft in (100, 16384):
        with pytest.raises(AlsepError):
            pitch.shift_pitch_array(on(dev, x), 3, n_fft=n_fft, ctx=dev)
    with pytest.raises(AlsepError):
        pitch.shift_pitch_array(on(dev, x), 3, n_fft=256, frames_per_batch=3, ctx=dev)
    with pytest.raises(AlsepError):
        pitch.shift_pitch_array(np.zeros((2, 3, 4), dtype=np.float32), 3, n_fft=256, ctx=dev)
    # the C entry points themselves
    lib, r = dev.lib, 2.0 ** (3 / 12.0)
    assert lib.alsep_pitch_shift_frames(600, 256, r) == int(np.ceil(600 / (64 / r))) + 1 == po.frame_count(600, 256, r)
    assert lib.alsep_pitch_shift_frames(600, 100, r) == -1 and lib.alsep_pitch_shift_frames(0, 256, r) == -1
    assert lib.alsep_pitch_shift_workspace_bytes(2, 256, 3, r) == -1 and lib.alsep_pitch_shift_workspace_bytes(2, 16384, 8, r) == -1
    assert lib.alsep_pitch_shift_workspace_bytes(2, 256, 8, 4.5) == -1 and lib.alsep_pitch_shift_workspace_bytes(0, 256, 8, r) == -1
    need = int(lib.alsep_pitch_shift_workspace_bytes(2, 256, 8, r))
    assert need > 0
    d, out = on(dev, x), torch.empty((2, 600), dtype=torch.float32, device=dev.device)
    ws = torch.empty((need,), dtype=torch.uint8, device=dev.device)

    def call(dst, ws_bytes, ratio=r, n_fft=256, fpb=8, n=600):
        return lib.alsep_pitch_shift(dev.handle, _lib.ptr(d), 2, n, 600, ratio, n_fft, fpb, _lib.ptr(dst), 600, _lib.ptr(ws), ws_bytes)
    assert call(out, need) == 0
    assert np.array_equal(host(out), ours(dev, "err", x, 3, 256, frames_per_batch=8))
    assert call(out, need - 1) == -1 and call(d, need) == -1
    assert call(out, need, ratio=4.01) == -1 and call(out, need, ratio=0.2) == -1 and call(out, need, n=0) == -1
    assert call(out, need, n_fft=100) == -1 and call(out, need, n_fft=16384) == -1 and call(out, need, fpb=3) == -1


def test_host_form_keeps_dtype_and_layout(dev):
    """shift_pitch((samples, sr), s): soundfile layout in and out (util/audio_track.py:643-666, :689-694)"""
    from audiolab_amd import pitch
    x = signal(2, 700, seed=8)
    pcm = np.clip(np.rint(x.T.astype(np.float64) * 32768), -32768, 32767).astype(np.int16)         # [N, 2]
    got, sr = pitch.shift_pitch((pcm, 44100), 3, ctx=dev)
    assert sr == 44100 and got.dtype == np.int16 and got.shape == (700, 2)
    want = host(pitch.shift_pitch_array(on(dev, np.ascontiguousarray((pcm.astype(np.float64) / 32768).T.astype(np.float32))), 3, ctx=dev))
    assert np.array_equal(got, np.clip(np.rint(want.T.astype(np.float64) * 32768), -32768, 32767).astype(np.int16))
    mono64, sr = pitch.shift_pitch((x[0].astype(np.float64), SR), -2, ctx=dev)
    assert sr == SR and mono64.dtype == np.float64 and mono64.shape == (700,)
    assert np.array_equal(mono64, host(pitch.shift_pitch_array(on(dev, x[:1]), -2, ctx=dev))[0].astype(np.float64))
    with pytest.raises(TypeError):
        pitch.shift_pitch((np.zeros((100, 2), dtype=np.uint8), SR), 3, ctx=dev)


@pytest.mark.gpu
@pytest.mark.parametrize("s,frames_per_batch", [(3, 256), (-4, 160)])
def test_long_track_in_several_batches(gpu_ctx, s, frames_per_batch):
    """20 s of stereo at 44.1 kHz, n_fft 4096, at least four batches; 64 seeded positions per channel -- the first and the last hundred
    samples and positions next to the batch seams among them -- against the oracle at the bound of the module docstring"""
    from audiolab_amd import pitch
    sr, n, n_fft = 44100, 20 * 44100, 4096
    x = signal(2, n, seed=9, sr=sr)
    r = po.ratio(s)
    frames = po.frame_count(n, n_fft, r)
    assert frames == gpu_ctx.lib.alsep_pitch_shift_frames(n, n_fft, r) and -(-frames // frames_per_batch) >= 4
    rng = np.random.default_rng(31)
    seams = [int(b * frames_per_batch * (n_fft // 4) / r) for b in range(1, frames // frames_per_batch + 1)]
    near = np.concatenate([[m - 700, m - 1, m, m + 1, m + 700] for m in seams])
    pos = np.unique(np.clip(np.concatenate([rng.integers(0, 100, 6), rng.integers(n - 100, n, 6), [0, n - 1], near]), 0, n - 1))
    pos = np.sort(np.concatenate([pos, rng.choice(np.setdiff1d(np.arange(n), pos), 64 - len(pos), replace=False)]))
    assert len(pos) == 64
    out = pitch.shift_pitch_array(torch.from_numpy(x).cuda(), s, n_fft=n_fft, frames_per_batch=frames_per_batch, ctx=gpu_ctx)
    got = out[:, torch.from_numpy(pos).cuda()].cpu().numpy()
    want = np.stack([po.shift_channel(ch, s, n_fft, positions=pos) for ch in x])
    check(got, want, f"20 s stereo, s {s:+d}, {frames} frames in batches of {frames_per_batch}")
