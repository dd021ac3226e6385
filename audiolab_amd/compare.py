"""The arithmetic of the reference's Compare plugin (wrappers/compare.py:73-124) on the GPU: both files brought to 44.1 kHz with
``scipy.signal.resample`` (:84), cut to the shorter one (:92-93), RMS-normalised (:96-99), their absolute difference (:102) and the
magnitude spectrograms ``scipy.signal.stft(x, fs=44100, nperseg=2048, noverlap=1024)`` (:110-124) as the decibel arrays the figure shows
(:145, :152).  Float64 on the device throughout (csrc/compare.h, ``alsep_resample_fft_f64`` of csrc/reverb.hip); the two decibel arrays
are float32.  Pinned against scipy itself: tests/compare_oracle.py, tests/test_compare.py.

Kept quirk: the reference resamples ``get_array_of_samples()``, the INTERLEAVED samples, as one signal at the file's frame rate -- a stereo
file is treated as a mono signal of twice the length.  So is it here.

Departures from the reference:
  * a float WAV's samples are taken as they are; pydub would hand them to ffmpeg and read them back on a 32-bit integer grid;
  * when ``int(n * 44100 / frame_rate) == n`` the resampler's transform pair is skipped (scipy's rfft -> irfft round trip is the identity
    to about 1e-16);
  * the decibel arrays are float32 (float64 in the reference), which moves a value of up to 180 dB by at most 8e-6 dB;
  * files are read by audiolab_amd.wavio (WAV only; the wrapper transcodes anything else first).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Tuple, Union

import numpy as np
import torch

from . import _lib, wavio
from ._lib import AlsepError, Context

SAMPLE_RATE = 44100                                                          # :73
N_SEG, HOP, BINS = 2048, 1024, 1025                                          # :110
MAX_TRANSFORM = 1 << 27                                                      # the float64 transforms of csrc/reverb.hip

Track = Union[str, Tuple[np.ndarray, int]]


def _tables(ctx: Context) -> Tuple[torch.Tensor, torch.Tensor]:
    """the periodic Hann window and exp(-2 pi i m / 2048), float64, computed on the host"""
    m = np.arange(N_SEG, dtype=np.float64)
    window = 0.5 - 0.5 * np.cos(2.0 * np.pi * m / N_SEG)
    ang = 2.0 * np.pi * m / N_SEG
    twiddle = np.stack([np.cos(ang), -np.sin(ang)], axis=1)
    # the exact values at the multiples of a quarter turn
    twiddle[0], twiddle[N_SEG // 4], twiddle[N_SEG // 2], twiddle[3 * N_SEG // 4] = (1.0, 0.0), (0.0, -1.0), (-1.0, 0.0), (0.0, 1.0)
    return torch.from_numpy(window).to(ctx.device), torch.from_numpy(np.ascontiguousarray(twiddle)).to(ctx.device)


def load_track(track: Track) -> Tuple[torch.Tensor, int]:
    """a path or ``(samples, frame_rate)`` -> (float64 1-D tensor of the interleaved samples, frame rate)"""
    if isinstance(track, (str, bytes)) or hasattr(track, "__fspath__"):
        samples, rate = wavio.read_wav_interleaved(str(track))
        return torch.from_numpy(samples), int(rate)
    samples, rate = track
    t = torch.as_tensor(samples)
    if t.dim() != 1:
        raise ValueError("compare: a track is a 1-D sequence of interleaved samples")
    if int(rate) < 1:
        raise ValueError(f"compare: frame rate {rate}")
    return t.to(torch.float64), int(rate)


def _check_transform(n: int) -> None:
    """a length the float64 DFT takes: a power of two up to 2^27, or one whose Bluestein length 2^ceil(log2(2 n - 1)) is"""
    if n & (n - 1) == 0:
        length = n
    else:
        length = 1 << (2 * n - 2).bit_length()
    if length > MAX_TRANSFORM or n > MAX_TRANSFORM:
        raise AlsepError(f"compare: resampling {n} samples needs a transform of {length} points, above the limit of 2^27 "
                         f"(about 12 minutes of stereo at 44.1 kHz)")


@dataclass
class CompareResult:
    """``waveforms[i]``, ``differences``: float64 ``[n]`` device tensors; ``spec1_db``, ``diff_db``: float32 ``[1025, F]`` device tensors;
    ``t`` ``[F]`` and ``f`` ``[1025]``: the axes scipy.signal.stft returns, on the host; ``spec1``, ``spec_diff``: S1 and |S1 - S2|
    themselves (float64 ``[1025, F]``) when asked for, else None."""
    waveforms: List[torch.Tensor]
    differences: torch.Tensor
    spec1_db: torch.Tensor
    diff_db: torch.Tensor
    t: np.ndarray
    f: np.ndarray
    ctx: Context
    spec1: Optional[torch.Tensor] = None
    spec_diff: Optional[torch.Tensor] = None

    def minmax(self, x: torch.Tensor, columns: int):
        """``(min, argmin, max, argmax)`` device tensors over ``K = min(columns, n)`` buckets of the float64 ``[n]`` device tensor ``x``, bucket
        ``j`` = samples ``[floor(j n / K), floor((j + 1) n / K))``, the first index on ties"""
        if columns < 1:
            raise ValueError(f"compare: {columns} columns")
        ctx, n = self.ctx, int(x.shape[0])
        k = min(int(columns), n)
        mn, mx = ctx.empty((k,), torch.float64), ctx.empty((k,), torch.float64)
        imn, imx = ctx.empty((k,), torch.int64), ctx.empty((k,), torch.int64)
        ctx.check(ctx.lib.alsep_compare_minmax(ctx.handle, _lib.ptr(x), n, k, _lib.ptr(mn), _lib.ptr(imn), _lib.ptr(mx), _lib.ptr(imx)),
                  "alsep_compare_minmax")
        return mn, imn, mx, imx

    def envelopes(self, columns: int):
        """the three curves of the upper panels -- track 1, track 2, the difference -- at figure resolution: per curve ``(x, y)`` host
        arrays of ``2 K`` points, ``K = min(columns, n)``: each bucket's two extremum samples in index order, real samples at their own x"""
        out = []
        for curve in (self.waveforms[0], self.waveforms[1], self.differences):
            mn, imn, mx, imx = (v.cpu().numpy() for v in self.minmax(curve, columns))
            first = imn <= imx
            x = np.stack([np.where(first, imn, imx), np.where(first, imx, imn)], axis=1).reshape(-1)
            y = np.stack([np.where(first, mn, mx), np.where(first, mx, mn)], axis=1).reshape(-1)
            out.append((x, y))
        return out

    def spectra_reduced(self, columns: int):
        """``(t, spec1_db, diff_db)`` with the frames in ``Kt = min(columns, F)`` buckets (same rule): float32 ``[1025, Kt]`` device tensors
        of the per-bin maximum over each bucket, ``t`` the time of each bucket's first frame"""
        if columns < 1:
            raise ValueError(f"compare: {columns} columns")
        ctx, frames = self.ctx, int(self.spec1_db.shape[1])
        kt = min(int(columns), frames)
        outs = []
        for src in (self.spec1_db, self.diff_db):
            dst = ctx.empty((BINS, kt), torch.float32)
            ctx.check(ctx.lib.alsep_compare_colmax(ctx.handle, _lib.ptr(src), frames, kt, _lib.ptr(dst)), "alsep_compare_colmax")
            outs.append(dst)
        first = (np.arange(kt, dtype=np.int64) * frames) // kt
        return self.t[first], outs[0], outs[1]


def compare_arrays(a: Track, b: Track, ctx: Optional[Context] = None, frames_per_batch: int = 0, want_linear: bool = False) -> CompareResult:
    """``a``, ``b``: ``(interleaved samples, frame_rate)`` -- a 1-D array or tensor, host or device, taken as float64 -- or the path of a WAV
    file, read as float64 fractions of full scale (a float WAV's samples as they are: see the module docstring).  ``frames_per_batch``:
    spectrogram columns per kernel launch (0: the library's default); it changes no bit.  ``want_linear``: also return S1 and |S1 - S2|.
    ValueError when the common length is below 2048 samples (scipy: "noverlap must be less than nperseg"), AlsepError when a track that
    needs resampling is too long for the float64 transform; both before anything is launched."""
    ctx = ctx if ctx is not None else _lib.default_context(None)
    if frames_per_batch < 0:
        raise ValueError(f"compare: {frames_per_batch} frames per batch")
    tracks = [load_track(a), load_track(b)]
    nums = [int(int(x.shape[0]) * SAMPLE_RATE / rate) for x, rate in tracks]                         # :84
    n = min(nums)                                                                                    # :92-93
    if n < N_SEG:
        raise ValueError(f"compare: the common length is {n} samples; the spectrogram needs at least {N_SEG}")
    for (x, _), num in zip(tracks, nums):
        if num != int(x.shape[0]):
            _check_transform(int(x.shape[0]))
            _check_transform(num)
    lib = ctx.lib
    xs = []
    for (x, _), num in zip(tracks, nums):
        x = x.to(ctx.device).contiguous()
        n_in = int(x.shape[0])
        if num != n_in:
            need = int(lib.alsep_resample_fft_f64_workspace_bytes(n_in, num))
            if need < 0:
                raise AlsepError(f"compare: no workspace to resample {n_in} samples to {num}")
            ws = ctx.empty((need,), torch.uint8)
            y = ctx.empty((num,), torch.float64)
            ctx.check(lib.alsep_resample_fft_f64(ctx.handle, _lib.ptr(x), n_in, _lib.ptr(y), num, 1, n_in, num, _lib.ptr(ws), need),
                      "alsep_resample_fft_f64")
            del ws
            x = y
        xs.append(x)
    sumsq = ctx.empty((2,), torch.float64)
    ws_bytes = int(lib.alsep_compare_rms_workspace_bytes())
    ws = ctx.empty((ws_bytes,), torch.uint8)
    for i, x in enumerate(xs):
        ctx.check(lib.alsep_compare_rms(ctx.handle, _lib.ptr(x), n, _lib.ptr(sumsq) + 8 * i, _lib.ptr(ws), ws_bytes), "alsep_compare_rms")
    w0, w1, diff = (ctx.empty((n,), torch.float64) for _ in range(3))
    ctx.check(lib.alsep_compare_wave(ctx.handle, _lib.ptr(xs[0]), _lib.ptr(xs[1]), n, _lib.ptr(sumsq), _lib.ptr(w0), _lib.ptr(w1),
                                     _lib.ptr(diff)), "alsep_compare_wave")
    del xs
    frames = int(lib.alsep_compare_frames(n))
    if frames < 0:
        raise AlsepError(f"compare: {n} samples are more than the spectrogram kernel takes")
    window, twiddle = _tables(ctx)
    spec1_db, diff_db = ctx.empty((BINS, frames), torch.float32), ctx.empty((BINS, frames), torch.float32)
    spec1 = ctx.empty((BINS, frames), torch.float64) if want_linear else None
    spec_diff = ctx.empty((BINS, frames), torch.float64) if want_linear else None
    ctx.check(lib.alsep_compare_spectra(ctx.handle, _lib.ptr(w0), _lib.ptr(w1), n, _lib.ptr(window), _lib.ptr(twiddle), int(frames_per_batch),
                                        _lib.ptr(spec1_db), _lib.ptr(diff_db), _lib.ptr(spec1), _lib.ptr(spec_diff)), "alsep_compare_spectra")
    t = np.arange(frames, dtype=np.float64) * HOP / float(SAMPLE_RATE)
    f = np.arange(BINS, dtype=np.float64) * SAMPLE_RATE / N_SEG
    return CompareResult([w0, w1], diff, spec1_db, diff_db, t, f, ctx, spec1, spec_diff)
