"""Pitch shifting of stems -- the "transpose the song" path of the reference's Merge plugin (wrappers/merge.py:125-127 ->
util/audio_track.py:603-694 ``shift_pitch``), where every stem that is not a cloned voice is shifted by the ``pitch_shift`` Clone applied
to the voice.  The reference shells out to ffmpeg's ``rubberband`` filter.  That library is not part of this build, so bit parity is not
the goal (parity unpinned): this is a deterministic shifter of the project's own, a phase vocoder with identity phase locking followed by
a Kaiser-windowed sinc resampler, in double precision on the device (csrc/pitch.h, ``alsep_pitch_shift``), specified step by step in
tests/pitch_oracle.py and DESIGN section 4c and checked against that float64 restatement to float32 rounding.

``shift_pitch_array`` is the entry point for signals in (or on their way to) device memory; ``shift_pitch`` has the reference's signature
for its ``(ndarray, sample_rate)`` form (:643-666, :689-694): soundfile layout in, the same dtype, layout and rate out, ``pitch_shift == 0``
returns the argument itself (:626-627).

Departures from the reference: no transient handling; the channels are shifted independently (no stereo phase coupling); the quality
is a plain phase-locked vocoder's, not rubberband's; the ``AudioSegment`` and file-path forms of ``shift_pitch`` are not built (the Merge
wrapper hands device tensors over).
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import AlsepError, Context

MAX_SEMITONES = 24                                                           # the slider's range (wrappers/merge.py:54-62); ratio 1/4 .. 4
MAX_WORKSPACE_BYTES = 1 << 30                                                # default batch: as many frames as fit in 1 GiB
MIN_FRAMES_PER_BATCH = 4


def _as_channels(x, ctx: Context) -> torch.Tensor:
    t = torch.as_tensor(x)
    if t.dtype != torch.float32:
        t = t.to(torch.float32)
    if t.dim() == 1:
        t = t[None]
    if t.dim() != 2 or t.shape[0] < 1 or t.shape[1] < 1:
        raise AlsepError("shift_pitch: signals are [channels, samples]")
    return t.to(ctx.device).contiguous()


def shift_pitch_array(x, semitones, *, n_fft: int = 4096, frames_per_batch: int = 0, ctx: Optional[Context] = None) -> torch.Tensor:
    """``x`` shifted by ``semitones`` (|.| <= 24) at unchanged length as a float32 ``[C, N]`` device tensor.  ``x``: float32 ``[C, N]`` or
    ``[N]``, tensor or array, device or host.  ``n_fft``: the vocoder's frame, a power of two from 256 to 8192; ``frames_per_batch``: the
    frames transformed side by side (0: what a 1 GiB workspace holds, at least 4) -- it does not change a bit of the result.
    ``semitones == 0`` returns the input values unchanged."""
    ctx = ctx if ctx is not None else _lib.default_context(None)
    if not abs(semitones) <= MAX_SEMITONES:
        raise ValueError(f"shift_pitch: {semitones} semitones is outside -{MAX_SEMITONES} .. {MAX_SEMITONES}")
    x_t = _as_channels(x, ctx)
    if semitones == 0:
        return x_t.clone() if x_t is x else x_t
    ratio = 2.0 ** (semitones / 12.0)
    c, n = x_t.shape
    frames = int(ctx.lib.alsep_pitch_shift_frames(n, int(n_fft), ratio))
    if frames < 0:
        raise AlsepError(f"shift_pitch: n_fft {n_fft} is not supported (a power of two, 256 .. 8192)")
    if frames_per_batch == 0:
        lo = int(ctx.lib.alsep_pitch_shift_workspace_bytes(c, int(n_fft), MIN_FRAMES_PER_BATCH, ratio))
        per_frame = int(ctx.lib.alsep_pitch_shift_workspace_bytes(c, int(n_fft), MIN_FRAMES_PER_BATCH + 1, ratio)) - lo
        frames_per_batch = MIN_FRAMES_PER_BATCH + max(0, (MAX_WORKSPACE_BYTES - lo) // max(per_frame, 1) - 1)
    elif frames_per_batch < MIN_FRAMES_PER_BATCH:
        raise AlsepError(f"shift_pitch: {frames_per_batch} frames per batch; at least {MIN_FRAMES_PER_BATCH}")
    batch = max(MIN_FRAMES_PER_BATCH, min(int(frames_per_batch), frames))
    need = int(ctx.lib.alsep_pitch_shift_workspace_bytes(c, int(n_fft), batch, ratio))
    if need < 0:
        raise AlsepError(f"shift_pitch: no workspace for {c} channels, n_fft {n_fft}, {batch} frames per batch")
    ws = ctx.empty((need,), torch.uint8)
    out = ctx.empty((c, n), torch.float32)
    ctx.check(ctx.lib.alsep_pitch_shift(ctx.handle, _lib.ptr(x_t), c, n, n, ratio, int(n_fft), batch, _lib.ptr(out), n, _lib.ptr(ws), need),
              "alsep_pitch_shift")
    return out


_INT_BITS = {np.dtype(np.int16): 16, np.dtype(np.int32): 32}


def shift_pitch(audio: Tuple[np.ndarray, int], pitch_shift, ctx: Optional[Context] = None) -> Tuple[np.ndarray, int]:
    """util/audio_track.py:603-694 for ``audio = (samples, sample_rate)``: samples in soundfile layout, ``[N]`` or ``[N, C]``; the same
    dtype, layout and rate come back.  float32 / float64 samples are returned as they are computed (not clipped); int16 / int32 samples
    are shifted as fractions of their full scale and quantised by ``clip(rint(.))`` on their own grid; other dtypes are refused."""
    if pitch_shift == 0:
        return audio                                                         # :626-627
    samples, sr = audio
    samples = np.asarray(samples)
    if samples.ndim not in (1, 2) or samples.size == 0:
        raise ValueError("shift_pitch: samples are [N] or [N, C]")
    dt = samples.dtype
    if dt in _INT_BITS:
        full = float(1 << (_INT_BITS[dt] - 1))
        x = samples.astype(np.float64) / full
    elif dt in (np.dtype(np.float32), np.dtype(np.float64)):
        full, x = None, samples
    else:
        raise TypeError(f"shift_pitch: {dt} samples are not supported (float32, float64, int16, int32)")
    chan_major = np.ascontiguousarray(x.T if x.ndim == 2 else x[None], dtype=np.float32)
    y = shift_pitch_array(chan_major, pitch_shift, ctx=ctx).cpu().numpy()
    y = y.T if samples.ndim == 2 else y[0]
    if full is not None:
        y = np.clip(np.rint(y.astype(np.float64) * full), -full, full - 1)
    return np.ascontiguousarray(y.astype(dt)), sr
