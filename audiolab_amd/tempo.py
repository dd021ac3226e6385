"""Tempo and beat tracking on the GPU: what the reference's Export plugin gets from ``librosa.load`` + ``librosa.beat.beat_track``
(wrappers/export.py:18-40), restated from the published design and run in float64 on the device (csrc/tempo.h):

  a. mel power spectrogram: 22050 Hz, centred frames of 2048 samples every 512 (zero padding), periodic Hann, 128 Slaney mel bands 0 .. 11025 Hz;
  b. spectral flux: decibels floored at 80 below the maximum, rectified frame differences, the median over the bands, 3 leading zeros;
  c. the autocorrelation tempogram (window 344) averaged over the frames; the log-normal tempo prior and the pick run on the host;
  d. the local score: the envelope over its standard deviation, smoothed by a Gaussian of the beat period;
  e. Ellis' dynamic-programming recursion, one wave, sequential;
  f. the last beat, the walk back and the trim on the host, over three arrays of one value per frame.

Parity unpinned: librosa is not available to compare with.  The specification is tests/tempo_oracle.py (numpy / scipy), against which every
stage is pinned (tests/test_tempo.py).  Stand-in: a rate other than 22050 Hz goes through the Fourier-method resampler
``alsep_resample_fft_f64`` (``scipy.signal.resample`` on ``ceil(n 22050 / sr)`` points) where ``librosa.load`` runs soxr_hq.
"""
from __future__ import annotations

import functools
import logging
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import _lib, wavio
from ._lib import AlsepError, Context
from .compare import MAX_TRANSFORM                                         # the float64 transforms of csrc/reverb.hip

logger = logging.getLogger(__name__)

SAMPLE_RATE, N_FFT, HOP, N_MELS = 22050, 2048, 512, 128
BINS = N_FFT // 2 + 1
WIN = int(8.0 * SAMPLE_RATE / HOP)                                           # 344 frames, 8 seconds
MAX_SECONDS = 3600


def _hz_to_mel(f: np.ndarray) -> np.ndarray:
    """the Slaney scale: linear below 1 kHz (200 / 3 Hz per mel), logarithmic above (27 mels per factor of 6.4)"""
    f = np.asarray(f, dtype=np.float64)
    return np.where(f >= 1000.0, 15.0 + 27.0 * np.log(np.maximum(f, 1e-300) / 1000.0) / np.log(6.4), 3.0 * f / 200.0)


def _mel_to_hz(m: np.ndarray) -> np.ndarray:
    m = np.asarray(m, dtype=np.float64)
    return np.where(m >= 15.0, 1000.0 * np.exp(np.log(6.4) * (m - 15.0) / 27.0), 200.0 * m / 3.0)


@functools.lru_cache(maxsize=None)
def mel_bands() -> Tuple[np.ndarray, np.ndarray]:
    """the filterbank as the kernel takes it: int32 ``[128, 3]`` (first bin, bin count, offset into the weights) and the float64 weights of
    every band's non-zero stretch: triangles over neighbouring points of the mel scale, each scaled by 2 / its width in Hz"""
    freqs = np.linspace(0.0, SAMPLE_RATE / 2.0, BINS)
    edges = _mel_to_hz(np.linspace(_hz_to_mel(0.0), _hz_to_mel(SAMPLE_RATE / 2.0), N_MELS + 2))
    bands = np.zeros((N_MELS, 3), dtype=np.int32)
    weights: List[np.ndarray] = []
    at = 0
    for i in range(N_MELS):
        rise = (freqs - edges[i]) / (edges[i + 1] - edges[i])
        fall = (edges[i + 2] - freqs) / (edges[i + 2] - edges[i + 1])
        tri = np.maximum(0.0, np.minimum(rise, fall)) * (2.0 / (edges[i + 2] - edges[i]))
        nz = np.flatnonzero(tri)
        first, count = (int(nz[0]), int(nz[-1] - nz[0] + 1)) if len(nz) else (0, 0)
        bands[i] = (first, count, at)
        weights.append(tri[first:first + count])
        at += count
    return bands, np.concatenate(weights)


def _hann(n: int) -> np.ndarray:
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n, dtype=np.float64) / n)


def _twiddle() -> np.ndarray:
    ang = 2.0 * np.pi * np.arange(N_FFT, dtype=np.float64) / N_FFT
    tw = np.stack([np.cos(ang), -np.sin(ang)], axis=1)
    tw[0], tw[N_FFT // 4], tw[N_FFT // 2], tw[3 * N_FFT // 4] = (1.0, 0.0), (0.0, -1.0), (-1.0, 0.0), (0.0, 1.0)
    return np.ascontiguousarray(tw)


def _dev(ctx: Context, a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)


def mel_power(ctx: Context, y: torch.Tensor) -> torch.Tensor:
    """float64 ``[n]`` device tensor at 22050 Hz -> float64 ``[128, F]``"""
    n = int(y.shape[0])
    F = int(ctx.lib.alsep_tempo_frames(n))
    if F < 0:
        raise ValueError(f"tempo: {n} samples at {SAMPLE_RATE} Hz (1 sample .. {MAX_SECONDS // 60} minutes)")
    bands, weights = mel_bands()
    mel = ctx.empty((N_MELS, F), torch.float64)
    window, twiddle, bands_d, weights_d = (_dev(ctx, a) for a in (_hann(N_FFT), _twiddle(), bands, weights))
    ctx.check(ctx.lib.alsep_tempo_mel(ctx.handle, _lib.ptr(y), n, _lib.ptr(window), _lib.ptr(twiddle), _lib.ptr(bands_d), _lib.ptr(weights_d),
                                      int(weights.shape[0]), _lib.ptr(mel)), "alsep_tempo_mel")
    return mel


def flux(ctx: Context, mel: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """float64 ``[128, F]`` -> (the decibel array, floored at 80 below its maximum, ``[128, F]``; the onset envelope ``[F]``)"""
    F = int(mel.shape[1])
    db, env = ctx.empty((N_MELS, F), torch.float64), ctx.empty((F,), torch.float64)
    need = int(ctx.lib.alsep_tempo_flux_workspace_bytes())
    ws = ctx.empty((need,), torch.uint8)
    ctx.check(ctx.lib.alsep_tempo_flux(ctx.handle, _lib.ptr(mel), F, _lib.ptr(db), _lib.ptr(env), _lib.ptr(ws), need), "alsep_tempo_flux")
    return db, env


def env_stats(ctx: Context, env: torch.Tensor) -> torch.Tensor:
    """-> device ``[3]``: max|env|, mean, standard deviation (ddof = 1)"""
    stats = ctx.empty((3,), torch.float64)
    ctx.check(ctx.lib.alsep_tempo_env_stats(ctx.handle, _lib.ptr(env), int(env.shape[0]), _lib.ptr(stats)), "alsep_tempo_env_stats")
    return stats


def tempogram_mean(ctx: Context, env: torch.Tensor) -> torch.Tensor:
    """-> device ``[344]``: the normalised autocorrelation of the windowed envelope, averaged over the frames"""
    tg = ctx.empty((WIN,), torch.float64)
    need = int(ctx.lib.alsep_tempo_tempogram_workspace_bytes())
    ws, window = ctx.empty((need,), torch.uint8), _dev(ctx, _hann(WIN))
    ctx.check(ctx.lib.alsep_tempo_tempogram(ctx.handle, _lib.ptr(env), int(env.shape[0]), _lib.ptr(window), _lib.ptr(tg), _lib.ptr(ws), need),
              "alsep_tempo_tempogram")
    return tg


def tempo_scores(tg: np.ndarray, start_bpm: float = 120.0) -> Tuple[np.ndarray, np.ndarray]:
    """host: (the tempo of every lag, ``log1p(1e6 tg)`` plus the log-normal prior around ``start_bpm``, one octave wide, -inf at 320 bpm and above)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        bpms = 60.0 * SAMPLE_RATE / (HOP * np.arange(WIN, dtype=np.float64))
        prior = -0.5 * ((np.log2(bpms) - np.log2(start_bpm)) / 1.0) ** 2
    prior[:int(np.argmax(bpms < 320.0))] = -np.inf
    return bpms, np.log1p(1e6 * tg) + prior


def period_of(bpm: float) -> int:
    return int(round(60.0 * (SAMPLE_RATE / HOP) / bpm))


def local_score(ctx: Context, env: torch.Tensor, period: int, stats: Optional[torch.Tensor] = None) -> torch.Tensor:
    window = _dev(ctx, np.exp(-0.5 * (np.arange(-period, period + 1) * 32.0 / period) ** 2))
    stats = stats if stats is not None else env_stats(ctx, env)
    ls = ctx.empty((int(env.shape[0]),), torch.float64)
    ctx.check(ctx.lib.alsep_tempo_local_score(ctx.handle, _lib.ptr(env), int(env.shape[0]), _lib.ptr(stats), _lib.ptr(window), int(period),
                                              _lib.ptr(ls)), "alsep_tempo_local_score")
    return ls


def dp_tables(period: int, tightness: float = 100.0) -> Tuple[np.ndarray, np.ndarray]:
    """the offsets ``-2 period .. -round(period / 2)`` (ties to even) and their transition costs"""
    w = np.arange(-2 * period, -int(round(period / 2)) + 1, dtype=np.int64)
    return w, -tightness * np.log(-w / period) ** 2


def beat_dp(ctx: Context, ls: torch.Tensor, period: int, tightness: float = 100.0) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (cum float64 ``[F]``, back int32 ``[F]``)"""
    w, txwt = dp_tables(period, tightness)
    F = int(ls.shape[0])
    cum, back, costs = ctx.empty((F,), torch.float64), ctx.empty((F,), torch.int32), _dev(ctx, txwt)
    ctx.check(ctx.lib.alsep_tempo_beat_dp(ctx.handle, _lib.ptr(ls), F, _lib.ptr(costs), int(w[0]), int(len(w)), _lib.ptr(cum), _lib.ptr(back)),
              "alsep_tempo_beat_dp")
    return cum, back


def local_maxima(x: np.ndarray) -> np.ndarray:
    """``x[i] > x[i - 1]`` and ``x[i] >= x[i + 1]`` with the ends repeated: the first element never is one"""
    p = np.pad(x, 1, mode="edge")
    return (x > p[:-2]) & (x >= p[2:])


def finish(cum: np.ndarray, back: np.ndarray, ls: np.ndarray, trim: bool = True) -> np.ndarray:
    """host: the last beat (the largest frame whose cum is a local maximum above half the median of the local maxima), the walk along
    ``back`` to -1, and the trim of weak beats at both ends"""
    peaks = local_maxima(cum)
    if not peaks.any():
        return np.zeros(0, dtype=np.int64)
    ok = np.flatnonzero(peaks & (2.0 * cum > np.median(cum[peaks])))
    if len(ok) == 0:
        return np.zeros(0, dtype=np.int64)
    beats = [int(ok.max())]
    while back[beats[-1]] >= 0:
        beats.append(int(back[beats[-1]]))
    beats = np.array(beats[::-1], dtype=np.int64)
    if trim:
        picked, taps = ls[beats], (0.0, 0.5, 1.0, 0.5, 0.0)                   # the 5-point symmetric Hann window, "same"
        wide = np.concatenate([np.zeros(2), picked, np.zeros(2)])
        smooth = sum(t * wide[4 - j:4 - j + len(picked)] for j, t in enumerate(taps))
        keep = np.flatnonzero(smooth > 0.5 * np.sqrt(np.mean(smooth ** 2)))
        beats = beats[keep.min():keep.max() + 1] if len(keep) else beats[:0]
    return beats


@dataclass
class TempoResult:
    """``bpm`` 0.0 and no beats when the onset envelope is all zero.  ``k``: the winning lag, ``period``: frames per beat.  ``stages`` (when
    asked for): the device tensors ``y, mel, db, env, tg, ls, cum, back`` as far as the run got."""
    bpm: float
    beat_frames: np.ndarray
    beat_times: np.ndarray
    k: int = 0
    period: int = 0
    stages: Dict[str, torch.Tensor] = field(default_factory=dict)


def _check_transform(n: int) -> None:
    length = n if n & (n - 1) == 0 else 1 << (2 * n - 2).bit_length()
    if length > MAX_TRANSFORM or n > MAX_TRANSFORM:
        raise AlsepError(f"tempo: resampling {n} samples needs a transform of {length} points, above the limit of 2^27")


def to_22050(ctx: Context, y, sr: int) -> torch.Tensor:
    """mono ``[n]`` or ``[channels, n]`` at ``sr`` -> float64 ``[m]`` on the device at 22050 Hz: channels averaged, then the Fourier-method
    resampler on ``m = ceil(n 22050 / sr)`` points"""
    x = torch.as_tensor(y).to(ctx.device, torch.float64)
    if x.dim() == 2:
        x = x.mean(dim=0)
    if x.dim() != 1 or int(x.shape[0]) < 1:
        raise ValueError("tempo: a track is [n] or [channels, n] with n >= 1")
    n = int(x.shape[0])
    if int(sr) < 1:
        raise ValueError(f"tempo: sample rate {sr}")
    if n > MAX_SECONDS * int(sr):
        raise ValueError(f"tempo: {n / sr / 60.0:.1f} minutes; tracks of up to {MAX_SECONDS // 60} minutes are taken")
    x = x.contiguous()
    if int(sr) == SAMPLE_RATE:
        return x
    m = -(-n * SAMPLE_RATE // int(sr))
    _check_transform(n)
    _check_transform(m)
    need = int(ctx.lib.alsep_resample_fft_f64_workspace_bytes(n, m))
    if need < 0:
        raise AlsepError(f"tempo: no workspace to resample {n} samples to {m}")
    ws, out = ctx.empty((need,), torch.uint8), ctx.empty((m,), torch.float64)
    ctx.check(ctx.lib.alsep_resample_fft_f64(ctx.handle, _lib.ptr(x), n, _lib.ptr(out), m, 1, n, m, _lib.ptr(ws), need), "alsep_resample_fft_f64")
    return out


def beat_track_array(y, sr: int, ctx: Optional[Context] = None, *, start_bpm: float = 120.0, tightness: float = 100.0, trim: bool = True,
                     want_stages: bool = False) -> TempoResult:
    """``y``: mono ``[n]`` or ``[channels, n]`` (array or tensor, host or device) at ``sr`` Hz; channels are averaged first.  ValueError for a
    track of more than 60 minutes; one shorter than a frame is fine, the centring pad covers it."""
    ctx = ctx if ctx is not None else _lib.default_context(None)
    if not (start_bpm > 0.0) or not (tightness > 0.0):
        raise ValueError(f"tempo: start_bpm {start_bpm} and tightness {tightness} must be positive")
    stages: Dict[str, torch.Tensor] = {}
    stages["y"] = y22 = to_22050(ctx, y, sr)
    stages["mel"] = mel = mel_power(ctx, y22)
    stages["db"], stages["env"] = db, env = flux(ctx, mel)
    stats = env_stats(ctx, env)
    empty = TempoResult(0.0, np.zeros(0, dtype=np.int64), np.zeros(0), stages=stages if want_stages else {})
    if not (float(stats[0].item()) > 0.0):                                   # an all-zero envelope: no tempo
        return empty
    stages["tg"] = tg = tempogram_mean(ctx, env)
    bpms, scores = tempo_scores(tg.cpu().numpy(), start_bpm)
    k = int(np.argmax(scores))
    bpm, period = float(bpms[k]), period_of(float(bpms[k]))
    stages["ls"] = ls = local_score(ctx, env, period, stats)
    stages["cum"], stages["back"] = cum, back = beat_dp(ctx, ls, period, tightness)
    beats = finish(cum.cpu().numpy(), back.cpu().numpy(), ls.cpu().numpy(), trim)
    return TempoResult(bpm, beats, beats * HOP / float(SAMPLE_RATE), k, period, stages if want_stages else {})


def detect_bpm(audio_path: str, start_time: float = 0, end_time: float = None, ctx: Optional[Context] = None):
    """the reference's helper (wrappers/export.py:18-40): ``(bpm, beat_times)`` of the file between ``start_time`` and ``end_time`` seconds (cut
    before resampling); any exception is logged and ``(0, [])`` comes back.  The file is read by audiolab_amd.wavio; anything that is not a
    WAV goes through ``ensure_wav`` first."""
    bpm, beat_times = 0, []
    try:
        from .separator.stem_separator import ensure_wav
        wav = ensure_wav(audio_path)
        samples, sr = wavio.read_wav_interleaved(wav)
        channels = wavio.read_wav_info(wav)[0]
        y = samples.reshape(-1, channels).T
        first = int(start_time * sr)
        last = first + int((end_time - start_time) * sr) if end_time else y.shape[1]
        res = beat_track_array(np.ascontiguousarray(y[:, first:last]), sr, ctx)
        bpm, beat_times = res.bpm, [float(t) for t in res.beat_times]
        logger.info(f"Estimated tempo for {audio_path}: {bpm}")
    except Exception as e:
        logger.error(f"Error detecting BPM for {audio_path}: {e}")
    return bpm, beat_times
