"""Reference-track mastering on the GPU: what the reference's Remaster plugin gets from ``matchering.process(target, reference,
[pcm24(out)])`` (wrappers/remaster.py:67-76), restated from the published Matchering 2.0 design in float64 on the device (csrc/master.h).
Parity unpinned -- Matchering itself is not available to compare with; the specification is tests/remaster_oracle.py, built from scipy's
own ``stft``, ``fftconvolve``, ``filtfilt``, ``lfilter``, ``butter``, ``maximum_filter1d`` and ``interp1d``, and DESIGN section 4e.

Steps: the reference is brought up to the threshold; both tracks go to mid / side; each is cut into ``d`` equal pieces of at most
``P`` samples and the RMS of the pieces at or above the average (the "loudest") is its level; the target is scaled to the reference's
level; per mid / side channel the ratio of the two averaged magnitude spectra of the loudest pieces, smoothed on a logarithmic grid
(LOWESS), becomes a linear-phase FIR of ``n_fft`` taps that is applied to the whole track; the level is corrected
``rms_correction_steps`` times on the clipped mid channel; a look-ahead limiter (sliding maxima, a zero-phase attack filter, hold and
release filters) brings the peaks under the threshold; the result is normalised to the threshold and quantised to 24 bits.

The device does everything that touches the track.  The host sees ``d <= 61`` sums of squares per level, two spectra of ``n_fft / 2 + 1``
bins, and designs the FIR from them (numpy / scipy on a few thousand points).

Departures from Matchering, declared: a rate other than ``sample_rate`` is resampled with ``alsep_resample_fft_f64`` (scipy.signal.resample's
method; Matchering uses resampy); LOWESS runs without ``delta`` skipping (Matchering passes ``delta=0.001``); previews and results other than
``pcm24`` are not produced.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import _lib, wavio
from ._lib import AlsepError, Context


@dataclass
class MasterConfig:
    """Matchering's defaults.  ``P``: the piece size in samples (None: ``int(max_piece_s * sample_rate)``).  Times in milliseconds."""
    sample_rate: int = 44100
    max_length_s: float = 900.0
    max_piece_s: float = 15.0
    threshold: float = (2 ** 15 - 61) / 2 ** 15
    min_value: float = 1e-6
    n_fft: int = 4096
    lin_log_oversampling: int = 4
    rms_correction_steps: int = 4
    lowess_frac: float = 0.0375
    attack: float = 1.0
    hold: float = 1.0
    release: float = 3000.0
    attack_filter_coefficient: float = -2.0
    hold_filter_coefficient: float = 7.0
    release_filter_coefficient: float = 800.0
    P: Optional[int] = None

    def __post_init__(self):
        if self.P is None:
            self.P = int(self.max_piece_s * self.sample_rate)
        if self.n_fft < 256 or self.n_fft > 8192 or self.n_fft & (self.n_fft - 1):
            raise ValueError(f"remaster: n_fft {self.n_fft}; a power of two from 256 to 8192")
        if self.sample_rate < 1 or self.P < self.n_fft:
            raise ValueError(f"remaster: pieces of {self.P} samples at {self.sample_rate} Hz; a piece holds at least one frame of {self.n_fft}")
        if not (0.0 < self.threshold <= 1.0 and self.min_value > 0.0 and self.rms_correction_steps >= 0 and self.lin_log_oversampling >= 1):
            raise ValueError("remaster: threshold in (0, 1], min_value > 0, rms_correction_steps >= 0, lin_log_oversampling >= 1")
        for name in ("attack", "hold"):
            if 2 * odd(ms_to_samples(getattr(self, name), self.sample_rate)) - 1 > 8191:
                raise ValueError(f"remaster: {name} of {getattr(self, name)} ms is a window of more than 8191 samples")
        if not (self.release > 0.0 and 0.0 < self.hold_filter_coefficient < self.sample_rate / 2
                and 0.0 < self.release_filter_coefficient / self.release < self.sample_rate / 2):
            raise ValueError("remaster: the hold and release filters need cutoffs between 0 and half the sample rate")


def odd(v: int) -> int:
    return v + 1 if v % 2 == 0 else v


def ms_to_samples(t: float, sample_rate: int) -> int:
    return int(sample_rate * t / 1000.0)


def geometry(n: int, P: int) -> Tuple[int, int]:
    """-> (d pieces, p samples each); the n - d p samples at the end take no part in the analysis"""
    d = int(n / P) + 1
    return d, int(n / d)


def loudest(sumsq: np.ndarray, p: int) -> Tuple[np.ndarray, float]:
    """per-piece sums of squares -> (indices of the pieces whose RMS is at or above the average, the RMS over those)"""
    r = np.sqrt(np.asarray(sumsq, dtype=np.float64) / p)
    avg = np.sqrt(np.mean(r ** 2))
    mask = r >= avg
    return np.nonzero(mask)[0].astype(np.int32), float(np.sqrt(np.mean(r[mask] ** 2)))


# ---- thin wrappers of the entry points: device tensors in, device tensors out --------------------------------------------------------
def _workspace(ctx: Context) -> torch.Tensor:
    ws = getattr(ctx, "_master_ws", None)
    if ws is None or ws.device != ctx.device:
        ws = ctx.empty((int(ctx.lib.alsep_master_workspace_bytes()),), torch.uint8)
        ctx._master_ws = ws
    return ws


def _rows(x: torch.Tensor, rows: int, what: str) -> int:
    if x.dtype != torch.float64 or x.dim() != 2 or int(x.shape[0]) != rows or not x.is_contiguous():
        raise ValueError(f"remaster: {what} is a contiguous float64 [{rows}, n] tensor")
    return int(x.shape[1])


def _vector(x: torch.Tensor, what: str) -> int:
    if x.dtype != torch.float64 or x.dim() != 1 or not x.is_contiguous() or int(x.shape[0]) < 1:
        raise ValueError(f"remaster: {what} is a contiguous float64 [n] tensor")
    return int(x.shape[0])


def mid_side(ctx: Context, lr: torch.Tensor, divisor: float = 1.0) -> torch.Tensor:
    n = _rows(lr, 2, "the signal")
    ms = ctx.empty((2, n), torch.float64)
    ctx.check(ctx.lib.alsep_master_midside(ctx.handle, _lib.ptr(lr), n, n, float(divisor), _lib.ptr(ms), n), "alsep_master_midside")
    return ms


def left_right(ctx: Context, ms: torch.Tensor, scale: float = 1.0) -> torch.Tensor:
    n = _rows(ms, 2, "mid / side")
    lr = ctx.empty((2, n), torch.float64)
    ctx.check(ctx.lib.alsep_master_leftright(ctx.handle, _lib.ptr(ms), n, n, float(scale), _lib.ptr(lr), n), "alsep_master_leftright")
    return lr


def piece_sumsq(ctx: Context, x: torch.Tensor, d: int, p: int, scale: float = 1.0, clip: bool = False) -> np.ndarray:
    """the sums of squares of the d pieces of p samples of the float64 [n] tensor x (of clip(scale x, -1, 1) with ``clip``) -> host [d]"""
    n = _vector(x, "the channel")
    if d < 1 or d > 64 or p < 1 or d * p > n:
        raise ValueError(f"remaster: {d} pieces of {p} samples in {n}")
    ws = _workspace(ctx)
    out = ctx.empty((d,), torch.float64)
    ctx.check(ctx.lib.alsep_master_piece_sumsq(ctx.handle, _lib.ptr(x), n, d, p, float(scale), 1 if clip else 0, _lib.ptr(out), _lib.ptr(ws),
                                               ws.numel()), "alsep_master_piece_sumsq")
    return out.cpu().numpy()


def peak(ctx: Context, x: torch.Tensor) -> float:
    """max|x| of a float64 [2, n] (or [n]) tensor"""
    rows, n = (1, _vector(x, "the signal")) if x.dim() == 1 else (2, _rows(x, 2, "the signal"))
    ws = _workspace(ctx)
    out = ctx.empty((1,), torch.float64)
    ctx.check(ctx.lib.alsep_master_peak(ctx.handle, _lib.ptr(x), rows, n, n, _lib.ptr(out), _lib.ptr(ws), ws.numel()), "alsep_master_peak")
    return float(out.cpu()[0])


def _twiddle(ctx: Context, n_fft: int) -> torch.Tensor:
    """exp(-2 pi i m / n_fft), float64 (re, im), computed on the host, exact at the multiples of a quarter turn"""
    cache = ctx.__dict__.setdefault("_master_twiddle", {})
    if n_fft not in cache or cache[n_fft].device != ctx.device:
        ang = 2.0 * np.pi * np.arange(n_fft, dtype=np.float64) / n_fft
        tw = np.stack([np.cos(ang), -np.sin(ang)], axis=1)
        tw[0], tw[n_fft // 4], tw[n_fft // 2], tw[3 * n_fft // 4] = (1.0, 0.0), (0.0, -1.0), (-1.0, 0.0), (0.0, 1.0)
        cache[n_fft] = torch.from_numpy(np.ascontiguousarray(tw)).to(ctx.device)
    return cache[n_fft]


def average_spectrum(ctx: Context, ms: torch.Tensor, p: int, pieces, n_fft: int, scale: float = 1.0) -> torch.Tensor:
    """float64 [2, n_fft / 2 + 1]: the mean over the whole frames of the listed pieces of |rfft| scale / n_fft, for mid and for side"""
    n = _rows(ms, 2, "mid / side")
    pieces = np.ascontiguousarray(pieces, dtype=np.int32)
    if pieces.ndim != 1 or not 1 <= len(pieces) <= 64:
        raise ValueError(f"remaster: a list of 1 .. 64 pieces, got {pieces.shape}")
    ws = _workspace(ctx)
    out = ctx.empty((2, n_fft // 2 + 1), torch.float64)
    ctx.check(ctx.lib.alsep_master_spectrum(ctx.handle, _lib.ptr(ms), n, n, int(p), pieces.ctypes.data_as(C.POINTER(C.c_int32)), len(pieces),
                                            int(n_fft), float(scale), _lib.ptr(_twiddle(ctx, n_fft)), _lib.ptr(out), _lib.ptr(ws), ws.numel()),
              "alsep_master_spectrum")
    return out


def convolve_same(ctx: Context, x: torch.Tensor, fir: torch.Tensor, scale: float = 1.0, log2_block: int = 0,
                  blocks_per_batch: int = 0) -> torch.Tensor:
    """``scale * scipy.signal.fftconvolve(x[c], fir[c], "same")`` per row: x float64 [C, n], fir float64 [C, taps].  ``log2_block``: the
    overlap-save block exponent (0: 8 times the filter, at least 2^10); ``blocks_per_batch``: blocks transformed side by side (0: up to
    256 MiB of workspace); neither changes the result beyond rounding."""
    if x.dtype != torch.float64 or fir.dtype != torch.float64 or x.dim() != 2 or fir.dim() != 2 or x.shape[0] != fir.shape[0]:
        raise ValueError("remaster: the convolution takes float64 [C, n] and [C, taps] tensors")
    if not (x.is_contiguous() and fir.is_contiguous()) or blocks_per_batch < 0 or log2_block < 0:
        raise ValueError("remaster: contiguous tensors, non-negative block settings")
    lib = ctx.lib
    ch, n, taps = int(x.shape[0]), int(x.shape[1]), int(fir.shape[1])
    need = int(lib.alsep_reverb_apply_block_log2(taps, 0))
    if log2_block == 0 and need >= 0:
        log2_block = min(max(need + 3, 10), 21)
    k = int(lib.alsep_reverb_apply_block_log2(taps, log2_block))
    if k < 0:
        raise AlsepError(f"remaster: no overlap-save block for a filter of {taps} taps with exponent {log2_block}")
    step = (1 << k) - taps + 1
    n_blocks = -(-(n + (taps - 1) // 2) // step)
    per = blocks_per_batch if blocks_per_batch > 0 else max(1, min(n_blocks, (256 << 20) // (32 << k)))
    ws_bytes = int(lib.alsep_master_convolve_workspace_bytes(taps, k, min(per, n_blocks)))
    ws = ctx.empty((ws_bytes,), torch.uint8)
    out = ctx.empty((ch, n), torch.float64)
    ctx.check(lib.alsep_master_convolve_same(ctx.handle, _lib.ptr(x), ch, n, n, _lib.ptr(fir), taps, float(scale), k, _lib.ptr(out), n,
                                             _lib.ptr(ws), ws_bytes), "alsep_master_convolve_same")
    return out


def slide_max(ctx: Context, x: torch.Tensor, w: int, centred: bool) -> torch.Tensor:
    """centred: ``scipy.ndimage.maximum_filter1d(x, size=2 w - 1)``; else ``out[i] = max x[max(0, i - w + 1) .. i]``"""
    n = _vector(x, "the curve")
    out = ctx.empty((n,), torch.float64)
    ctx.check(ctx.lib.alsep_master_slide_max(ctx.handle, _lib.ptr(x), n, int(w), 1 if centred else 0, _lib.ptr(out)), "alsep_master_slide_max")
    return out


def _first_order(b, a) -> Tuple[float, float, float]:
    b, a = np.atleast_1d(np.asarray(b, dtype=np.float64)), np.atleast_1d(np.asarray(a, dtype=np.float64))
    if len(a) != 2 or len(b) not in (1, 2) or a[0] == 0.0:
        raise ValueError("remaster: a first-order filter has b of one or two and a of two coefficients")
    return float(b[0] / a[0]), float(b[1] / a[0]) if len(b) == 2 else 0.0, float(a[1] / a[0])


def iir(ctx: Context, x: torch.Tensor, b, a, zi: float = 0.0, reverse: bool = False, chunk: int = 0) -> torch.Tensor:
    """``scipy.signal.lfilter(b, a, x, zi=[zi])`` for a first-order filter; ``reverse``: over ``x[::-1]``, stored back in x's order.
    ``chunk``: samples per workgroup of the scan (0: the library's default)."""
    n = _vector(x, "the curve")
    b0, b1, a1 = _first_order(b, a)
    need = int(ctx.lib.alsep_master_iir_workspace_bytes(n, int(chunk)))
    if need < 0:
        raise AlsepError(f"remaster: no scan of {n} samples in chunks of {chunk}")
    ws, y = ctx.empty((need,), torch.uint8), ctx.empty((n,), torch.float64)
    ctx.check(ctx.lib.alsep_master_iir(ctx.handle, _lib.ptr(x), n, b0, b1, a1, float(zi), 1 if reverse else 0, int(chunk), _lib.ptr(y), _lib.ptr(ws),
                                       need), "alsep_master_iir")
    return y


def filtfilt(ctx: Context, x: torch.Tensor, b, a, chunk: int = 0) -> torch.Tensor:
    """``scipy.signal.filtfilt(b, a, x)`` for a first-order filter, scipy's defaults"""
    n = _vector(x, "the curve")
    b0, b1, a1 = _first_order(b, a)
    if 1.0 + a1 == 0.0:
        raise ValueError("remaster: the filter has a pole at 1; lfilter_zi does not exist")
    zi = b1 - a1 * (b0 + b1) / (1.0 + a1)                                    # scipy.signal.lfilter_zi for one state
    need = int(ctx.lib.alsep_master_filtfilt_workspace_bytes(n, int(chunk)))
    if need < 0:
        raise AlsepError(f"remaster: no scan of {n} samples in chunks of {chunk}")
    ws, y = ctx.empty((need,), torch.uint8), ctx.empty((n,), torch.float64)
    ctx.check(ctx.lib.alsep_master_filtfilt(ctx.handle, _lib.ptr(x), n, b0, b1, a1, zi, int(chunk), _lib.ptr(y), _lib.ptr(ws), need),
              "alsep_master_filtfilt")
    return y


def rectify(ctx: Context, lr: torch.Tensor, threshold: float) -> Tuple[torch.Tensor, bool]:
    """-> (g = 1 - 1 / rect, whether anything rises above the threshold)"""
    n = _rows(lr, 2, "the signal")
    g, over = ctx.empty((n,), torch.float64), ctx.empty((1,), torch.int32)
    ctx.check(ctx.lib.alsep_master_rectify(ctx.handle, _lib.ptr(lr), n, n, float(threshold), _lib.ptr(g), _lib.ptr(over)), "alsep_master_rectify")
    return g, bool(int(over.cpu()[0]))


def limit(ctx: Context, lr: torch.Tensor, config: MasterConfig, chunk: int = 0, stages: Optional[Dict] = None):
    """the limiter of step 9 on a float64 [2, n] tensor -> (limited signal, gain curve or None, whether it ran, max|out| or None).  When nothing
    rises above the threshold the input itself is returned.  ``stages``: a dict that receives every intermediate curve."""
    from scipy import signal
    sr = config.sample_rate
    n = _rows(lr, 2, "the signal")
    wa, wh = odd(ms_to_samples(config.attack, sr)), odd(ms_to_samples(config.hold, sr))
    if n < 2 * max(wa, wh) - 1 or n < 7:
        raise ValueError(f"remaster: {n} samples are fewer than the limiter's window of {2 * max(wa, wh) - 1}")
    g, over = rectify(ctx, lr, config.threshold)
    if not over:
        return lr, None, False, None
    lib = ctx.lib
    c = float(np.exp(config.attack_filter_coefficient / wa))
    s_a = slide_max(ctx, g, wa, True)
    g_a = filtfilt(ctx, s_a, [1.0 - c], [1.0, -c], chunk)
    s_h = slide_max(ctx, g, wh, False)
    bh, ah = signal.butter(1, config.hold_filter_coefficient, fs=sr)
    br, ar = signal.butter(1, config.release_filter_coefficient / config.release, fs=sr)
    h = iir(ctx, s_h, bh, ah, 0.0, False, chunk)
    rel_in = ctx.empty((n,), torch.float64)
    ctx.check(lib.alsep_master_maximum(ctx.handle, _lib.ptr(s_h), _lib.ptr(h), n, _lib.ptr(rel_in)), "alsep_master_maximum")
    rel = iir(ctx, rel_in, br, ar, 0.0, False, chunk)
    ws = _workspace(ctx)
    out, gain, pk = ctx.empty((2, n), torch.float64), ctx.empty((n,), torch.float64), ctx.empty((1,), torch.float64)
    ctx.check(lib.alsep_master_limit_apply(ctx.handle, _lib.ptr(lr), n, n, _lib.ptr(s_h), _lib.ptr(g_a), _lib.ptr(h), _lib.ptr(rel), _lib.ptr(out), n,
                                           _lib.ptr(gain), _lib.ptr(pk), _lib.ptr(ws), ws.numel()), "alsep_master_limit_apply")
    if stages is not None:
        stages.update(g=g, s_a=s_a, g_a=g_a, s_h=s_h, h=h, rel_in=rel_in, rel=rel)
    return out, gain, True, float(pk.cpu()[0])


def pcm24(ctx: Context, lr: torch.Tensor, divisor: float = 1.0) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (lr / divisor, its 24-bit PCM: uint8 [6 n], L R interleaved, little-endian)"""
    n = _rows(lr, 2, "the signal")
    res, pcm = ctx.empty((2, n), torch.float64), ctx.empty((6 * n,), torch.uint8)
    ctx.check(ctx.lib.alsep_master_pcm24(ctx.handle, _lib.ptr(lr), n, n, float(divisor), _lib.ptr(res), n, _lib.ptr(pcm)), "alsep_master_pcm24")
    return res, pcm


# ---- the matching FIR: host arithmetic on n_fft / 2 + 1 bins ----------------------------------------------------------------------------
def _lowess_weights(offsets: np.ndarray) -> np.ndarray:
    """offsets [m, k]: the neighbours' distances from the point of the fit, in grid steps -> c [m, k] with fit = sum_j c_j y_j: the
    tricube-weighted linear fit is linear in y, my + slope (0 - mx) = sum_j (w_j / sw - mx w_j (x_j - mx) / sxx) y_j"""
    x = offsets.astype(np.float64)
    radius = np.max(np.abs(x), axis=1, keepdims=True)
    w = (1.0 - np.clip(np.abs(x) / radius, 0.0, 1.0) ** 3) ** 3
    sw = np.sum(w, axis=1, keepdims=True)
    mx = np.sum(w * x, axis=1, keepdims=True) / sw
    sxx = np.sum(w * (x - mx) ** 2, axis=1, keepdims=True)
    lin = np.where(sxx > 0.0, -mx * w * (x - mx) / np.where(sxx > 0.0, sxx, 1.0), 0.0)
    return w / sw + lin


def lowess(y: np.ndarray, frac: float) -> np.ndarray:
    """LOWESS without robustness iterations or skipping on x = linspace(0, 1, N): at every point a tricube-weighted linear fit over its
    k = max(2, int(frac N + 1e-10)) nearest neighbours.  On the uniform grid those are the k points from max(0, min(i - k // 2, N - k)),
    the fit depends on the neighbours' offsets alone, and it is linear in y: every interior point applies the same k coefficients (one
    correlation), the k points near the two ends have a row of coefficients each."""
    y = np.asarray(y, dtype=np.float64)
    N = len(y)
    k = min(N, max(2, int(frac * N + 1e-10)))
    half = k // 2
    j = np.arange(k)
    out = np.empty(N)
    inner = _lowess_weights((j - half)[None, :])[0]
    out[half:N - k + half + 1] = np.correlate(y, inner, "valid")            # windows from lo = 0 .. N - k, fitted at lo + half
    head = np.arange(half)                                                   # lo = 0
    out[:half] = _lowess_weights(j[None, :] - head[:, None]) @ y[:k]
    tail = np.arange(N - k + half + 1, N)                                    # lo = N - k
    out[N - k + half + 1:] = _lowess_weights((N - k + j)[None, :] - tail[:, None]) @ y[N - k:]
    return out


def matching_fir(a_target: np.ndarray, a_reference: np.ndarray, config: MasterConfig) -> np.ndarray:
    """the two averaged spectra of one channel -> the n_fft taps of step 5"""
    from scipy import interpolate, signal
    n_fft, sr = config.n_fft, config.sample_rate
    m = np.asarray(a_reference, dtype=np.float64) / np.maximum(config.min_value, np.asarray(a_target, dtype=np.float64))
    grid_lin = 0.5 * sr * np.linspace(0.0, 1.0, n_fft // 2 + 1)
    grid_log = 0.5 * sr * np.logspace(np.log10(4.0 / n_fft), 0.0, (n_fft // 2) * config.lin_log_oversampling + 1)
    on_log = interpolate.interp1d(grid_lin, m, "cubic")(grid_log)
    smooth = lowess(on_log, config.lowess_frac)
    back = interpolate.interp1d(grid_log, smooth, "cubic", fill_value="extrapolate")(grid_lin)
    back[0] = 0.0
    back[1] = m[1]
    return np.fft.ifftshift(np.fft.irfft(back)) * signal.windows.hann(n_fft)


# ---- the chain ------------------------------------------------------------------------------------------------------------------------------
@dataclass
class RemasterResult:
    """``result``: float64 [2, n] on the device; ``pcm24``: its 24-bit PCM, uint8 [6 n] on the device (``pcm24_bytes()`` for the host);
    ``fir_mid`` / ``fir_side``: host float64 [n_fft]; ``stages`` (with ``want_stages``): ``tgt_sumsq`` / ``ref_sumsq`` (host), ``tgt_spectrum`` /
    ``ref_spectrum`` [2, n_fft / 2 + 1], ``conv`` (mid / side after step 6, [2, n]), ``pre_limiter`` [2, n], ``gain`` [n] and the limiter's curves."""
    result: torch.Tensor
    pcm24: torch.Tensor
    k0: float
    coefficients: List[float]
    fir_mid: np.ndarray
    fir_side: np.ndarray
    limited: bool
    sample_rate: int
    stages: Dict = field(default_factory=dict)

    def pcm24_bytes(self) -> bytes:
        return self.pcm24.cpu().numpy().tobytes()


def _as_stereo(x, what: str) -> torch.Tensor:
    """[n] or [n, 2], host or device -> float64 [n, 2] tensor (where it is)"""
    t = torch.as_tensor(x)
    if t.dim() == 1:
        t = torch.stack([t, t], dim=1)
    if t.dim() != 2 or int(t.shape[1]) != 2:
        raise ValueError(f"remaster: the {what} is an [n] or [n, 2] signal, got {tuple(t.shape)}")
    return t.to(torch.float64)


def _check_resample(n: int, what: str) -> None:
    length = n if n & (n - 1) == 0 else 1 << (2 * n - 2).bit_length()
    if length > 1 << 27 or n > 1 << 27:
        raise AlsepError(f"remaster: resampling the {what} of {n} samples needs a transform of {length} points, above the limit of 2^27")


def _to_device_rows(ctx: Context, t: torch.Tensor, rate: int, config: MasterConfig) -> torch.Tensor:
    """[n, 2] at ``rate`` -> contiguous float64 [2, n'] on the device at the configured rate"""
    x = t.to(ctx.device).t().contiguous()
    if rate == config.sample_rate:
        return x
    n_in = int(x.shape[1])
    n_out = int(n_in * config.sample_rate / rate)
    lib = ctx.lib
    need = int(lib.alsep_resample_fft_f64_workspace_bytes(n_in, n_out))
    if need < 0:
        raise AlsepError(f"remaster: no workspace to resample {n_in} samples to {n_out}")
    ws, y = ctx.empty((need,), torch.uint8), ctx.empty((2, n_out), torch.float64)
    ctx.check(lib.alsep_resample_fft_f64(ctx.handle, _lib.ptr(x), n_in, _lib.ptr(y), n_out, 2, n_in, n_out, _lib.ptr(ws), need), "alsep_resample_fft_f64")
    return y


def remaster_arrays(target, reference, config: Optional[MasterConfig] = None, ctx: Optional[Context] = None, want_stages: bool = False,
                    chunk: int = 0, blocks_per_batch: int = 0) -> RemasterResult:
    """``target``, ``reference``: ``(samples, rate)`` with samples ``[n]`` (mono, duplicated) or ``[n, 2]``, numpy or tensor, host or device.
    ValueError, before anything is launched, when a track (at the configured rate) is shorter than ``n_fft`` samples or longer than
    ``max_length_s``.  ``chunk`` / ``blocks_per_batch``: the scan's chunk length and the convolution's batch (0: the defaults)."""
    config = config if config is not None else MasterConfig()
    ctx = ctx if ctx is not None else _lib.default_context(None)
    sr = config.sample_rate
    tracks = []
    for (samples, rate), what in ((target, "target"), (reference, "reference")):
        rate = int(rate)
        if rate < 1:
            raise ValueError(f"remaster: the {what}'s rate is {rate}")
        t = _as_stereo(samples, what)
        n_in = int(t.shape[0])
        n = n_in if rate == sr else int(n_in * sr / rate)
        if n < config.n_fft:
            raise ValueError(f"remaster: the {what} has {n} samples at {sr} Hz; the analysis needs at least {config.n_fft}")
        if n > config.max_length_s * sr:
            raise ValueError(f"remaster: the {what} has {n} samples at {sr} Hz, more than {config.max_length_s} s")
        if geometry(n, config.P)[0] > 64:
            raise ValueError(f"remaster: the {what}'s {n} samples in pieces of {config.P} are more than 64 pieces")
        if rate != sr:
            _check_resample(n_in, what)
            _check_resample(n, what)
        tracks.append((t, rate))
    wa, wh = odd(ms_to_samples(config.attack, sr)), odd(ms_to_samples(config.hold, sr))
    n_t = int(tracks[0][0].shape[0]) if tracks[0][1] == sr else int(int(tracks[0][0].shape[0]) * sr / tracks[0][1])
    if n_t < 2 * max(wa, wh) - 1 or n_t < 7:
        raise ValueError(f"remaster: the target's {n_t} samples are fewer than the limiter's window of {2 * max(wa, wh) - 1}")
    stages: Dict = {}

    tgt = _to_device_rows(ctx, tracks[0][0], tracks[0][1], config)
    ref = _to_device_rows(ctx, tracks[1][0], tracks[1][1], config)
    n = int(tgt.shape[1])
    # 1, 2: the reference up to the threshold; mid / side
    ref_peak = peak(ctx, ref)
    ref_div = max(config.min_value, ref_peak / config.threshold) if ref_peak < config.threshold else 1.0
    t_ms, r_ms = mid_side(ctx, tgt), mid_side(ctx, ref, ref_div)
    del tgt, ref
    # 3, 4: levels
    (t_d, t_p), (r_d, r_p) = geometry(n, config.P), geometry(int(r_ms.shape[1]), config.P)
    t_ss, r_ss = piece_sumsq(ctx, t_ms[0], t_d, t_p), piece_sumsq(ctx, r_ms[0], r_d, r_p)
    (t_loud, t_rms), (r_loud, r_rms) = loudest(t_ss, t_p), loudest(r_ss, r_p)
    k0 = r_rms / max(config.min_value, t_rms)
    # 5: the matching FIRs
    t_spec = average_spectrum(ctx, t_ms, t_p, t_loud, config.n_fft, k0)
    r_spec = average_spectrum(ctx, r_ms, r_p, r_loud, config.n_fft, 1.0)
    del r_ms
    t_host, r_host = t_spec.cpu().numpy(), r_spec.cpu().numpy()
    fir_mid, fir_side = matching_fir(t_host[0], r_host[0], config), matching_fir(t_host[1], r_host[1], config)
    fir = torch.from_numpy(np.ascontiguousarray(np.stack([fir_mid, fir_side]))).to(ctx.device)
    # 6: the filter over the whole track, the level match folded into it
    conv = convolve_same(ctx, t_ms, fir, scale=k0, blocks_per_batch=blocks_per_batch)
    del t_ms
    # 7: level correction -- the track is read, never rewritten; the running scale goes into the L / R pass
    scale, coefficients = 1.0, []
    for _ in range(config.rms_correction_steps):
        _, rms_c = loudest(piece_sumsq(ctx, conv[0], t_d, t_p, scale, clip=True), t_p)
        c = r_rms / max(config.min_value, rms_c)
        coefficients.append(c)
        scale *= c
    # 8, 9: back to L / R, the limiter
    lr = left_right(ctx, conv, scale)
    limiter_stages: Optional[Dict] = {} if want_stages else None
    out, gain, ran, out_peak = limit(ctx, lr, config, chunk, limiter_stages)
    # 10: normalise and quantise
    if out_peak is None:
        out_peak = peak(ctx, out)
    div = max(config.min_value, out_peak / config.threshold) if out_peak < config.threshold else 1.0
    result, pcm = pcm24(ctx, out, div)
    if want_stages:
        stages.update(tgt_sumsq=t_ss, ref_sumsq=r_ss, tgt_spectrum=t_spec, ref_spectrum=r_spec, conv=conv, pre_limiter=lr,
                      gain=gain if gain is not None else torch.ones((n,), dtype=torch.float64, device=ctx.device), **(limiter_stages or {}))
    return RemasterResult(result, pcm, k0, coefficients, fir_mid, fir_side, ran, sr, stages)


def read_track(path: str) -> Tuple[np.ndarray, int]:
    """a WAV file -> (float64 [n, channels <= 2] fractions of full scale, rate); more than two channels: the first two"""
    samples, rate = wavio.read_wav_interleaved(path)
    ch = wavio.read_wav_info(path)[0]
    x = samples.reshape(-1, ch)
    return (x[:, 0] if ch == 1 else np.ascontiguousarray(x[:, :2])), int(rate)


def remaster_file(target_path: str, reference_path: str, output_path: str, config: Optional[MasterConfig] = None,
                  ctx: Optional[Context] = None) -> RemasterResult:
    """WAV files in, a 24-bit PCM WAV at the configured rate out"""
    config = config if config is not None else MasterConfig()
    res = remaster_arrays(read_track(target_path), read_track(reference_path), config, ctx)
    raw = res.pcm24.cpu().numpy().reshape(-1, 3).astype(np.int32)
    v = raw[:, 0] | (raw[:, 1] << 8) | (raw[:, 2] << 16)
    v = np.where(v >= 1 << 23, v - (1 << 24), v).reshape(-1, 2).T
    wavio.write_wav(output_path, v, config.sample_rate, subtype="PCM_24")
    return res
