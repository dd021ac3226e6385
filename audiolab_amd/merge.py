"""Stem mixdown with loudness matching -- the arithmetic of the reference's Merge wrapper (wrappers/merge.py:15-45, :146-151) on the GPU.

The reference mixes with pydub: ``merged = stems[0].overlay(stems[1]).overlay(...)``, ``effects.normalize(merged)`` (headroom 0.1 dB), a gain
that brings the result's ``dBFS`` to the source file's, capped so that the peak stays below full scale (``prevent_clipping``), and
``apply_gain``.  pydub is a thin shell over the C module ``audioop``: a saturating integer add per stem (``add``), the unsigned peak (``max``),
a truncated integer RMS (``rms``) and a ``floor`` of the clipped double product (``mul``).  The same integer arithmetic runs here in three
passes of libalsep.so (csrc/mixdown.h) over an int32 mix that stays in device memory: ``alsep_mix_sum`` (several stems per launch, each read
once), ``alsep_mix_power`` (peak and the EXACT integer sum of squares of the normalised mix, which is not written) and ``alsep_mix_finish``.
The ``audioop`` arithmetic is pinned bit for bit by tests/golden/merge.npz (scripts/make_golden_merge.py runs the stdlib module); pydub's control
flow around it is restated from its published source and is UNPINNED (pydub is not a dependency of this build).

Host maths, in Python floats (pydub's ``normalize(headroom=0.1)`` and ``normalize_segment`` :15-45), M = 2^(bits-1)::

    db_to_float(d) = 10 ** (d / 20)          ratio_to_db(r) = 20 * math.log10(r)
    f1   = db_to_float(ratio_to_db(M * db_to_float(-0.1) / peak))        # peak == 0: a silent mix comes back as zeros, no gain
    rms  = int(math.sqrt(S / count))                                     # S exact, count = C * N; audioop.rms truncates
    dBFS = ratio_to_db(rms / M), -inf if rms == 0
    gain = target_dBFS - current_dBFS
    if prevent_clipping: gain = min(gain, -20 * math.log10(peak1 / M))   # peak1 = max|y1|
    f2   = db_to_float(gain)                                             # target -inf -> f2 = 0 -> zeros

Departures from the reference: lengths are sample-exact (pydub slices by milliseconds); float samples reach the integer grid by
``clip(rint(x 2^(b-1)))`` on the stem's own width b (the reference's conversion goes through ffmpeg); stems with differing sample rates are
an error (pydub would ``audioop.ratecv`` them).
"""
from __future__ import annotations

import math
from dataclasses import asdict, dataclass
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib, wavio
from ._lib import AlsepError, Context

HEADROOM_DB = 0.1                                                            # pydub.effects.normalize's default


@dataclass
class MixRecord:
    """what the host computed between the passes"""
    peak: int                  # max|mix| before any gain, on the grid of ``bits``
    f1: float                  # normalize's factor
    rms: int                   # audioop.rms of the normalised mix
    current_dBFS: float
    target_dBFS: float
    gain_dB: float
    f2: float
    bits: int = 32

    def as_dict(self) -> dict:
        return asdict(self)


def db_to_float(db: float) -> float:
    try:
        return 10 ** (float(db) / 20)
    except OverflowError:
        return math.inf


def ratio_to_db(ratio: float) -> float:
    return 20 * math.log10(ratio) if ratio > 0 else -math.inf


def normalize_factor(peak: int, bits: int) -> float:
    """pydub.effects.normalize(headroom=0.1): the factor apply_gain hands to audioop.mul"""
    return db_to_float(ratio_to_db((1 << (bits - 1)) * db_to_float(-HEADROOM_DB) / peak))


def rms_of(sum_squares: int, count: int) -> int:
    return int(math.sqrt(sum_squares / count))


def match_gain(target_dbfs: float, rms: int, peak1: int, bits: int, prevent_clipping: bool) -> Tuple[float, float, float]:
    """-> (current dBFS, gain in dB, f2) of normalize_segment (:19-45)"""
    full = 1 << (bits - 1)
    current = ratio_to_db(rms / full)
    gain = -math.inf if target_dbfs == -math.inf else target_dbfs - current
    if prevent_clipping:
        allowed = -20 * math.log10(peak1 / full) if peak1 else math.inf
        gain = min(gain, allowed)
    return current, gain, db_to_float(gain)


# ---- the three passes ---------------------------------------------------------------------------------------------------------------
def _rows(t: torch.Tensor, what: str) -> Tuple[int, int, int, int]:
    """-> (data pointer, channels, samples, row stride) of a [C, N] tensor whose rows are dense"""
    if t.device.type != _lib.DEVICE_TYPE:
        raise AlsepError(f"{what}: tensor on {t.device}, expected a {_lib.DEVICE_TYPE} tensor")
    if t.dim() != 2 or t.shape[1] < 1 or t.shape[0] < 1 or t.stride(1) != 1:
        raise AlsepError(f"{what}: expected [channels, samples] with dense rows")
    return t.data_ptr(), t.shape[0], t.shape[1], max(t.stride(0), t.shape[1])


def empty_mix(ctx: Context, channels: int, n: int, dtype=torch.int32) -> torch.Tensor:
    """[channels, n] view of a buffer whose rows start on 16-byte boundaries (the kernels then use 16-byte loads and stores)"""
    return ctx.empty((channels, (n + 3) // 4 * 4), dtype)[:, :n]


def mix_sum(ctx: Context, stems: Sequence[torch.Tensor], widths: Sequence[int], bits: int, max_per_launch: int = 0,
            acc: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, int]:
    """stems float32 [C_k, N_k] on the device, each with its source width -> (int32 mix [C, N_0], max|mix|); audioop.add stem by stem.
    ``acc``: an int32 [C, N_0] buffer to mix into (default: a fresh one with 16-byte aligned rows)."""
    if not stems or len(stems) != len(widths):
        raise AlsepError("mix_sum: one width per stem, at least one stem")
    per = _lib.MIX_MAX_STEMS if max_per_launch <= 0 else min(int(max_per_launch), _lib.MIX_MAX_STEMS)
    c, n = max(s.shape[0] for s in stems), stems[0].shape[1]
    if acc is None:
        acc = empty_mix(ctx, c, n)
    elif acc.dtype != torch.int32 or tuple(acc.shape) != (c, n):
        raise AlsepError(f"mix_sum: the mix is int32 [{c}, {n}]")
    peak = ctx.empty((1,), torch.int32)
    acc_p, _, _, acc_ld = _rows(acc, "mix_sum")
    for first in range(0, len(stems), per):
        group = stems[first:first + per]
        arr = (_lib.MixStem * len(group))()
        for j, s in enumerate(group):
            if s.dtype != torch.float32:
                raise AlsepError("mix_sum: stems are float32")
            p, ck, nk, ld = _rows(s, f"mix_sum: stem {first + j}")
            if ck not in (1, c):
                raise AlsepError(f"mix_sum: stem {first + j} has {ck} channels, the mix {c}")
            arr[j] = _lib.MixStem(p, nk, ld, ck, int(widths[first + j]))
        ctx.check(ctx.lib.alsep_mix_sum(ctx.handle, acc_p if first else None, acc_ld, arr, len(group), c, n, bits, acc_p, acc_ld, _lib.ptr(peak)),
                  "alsep_mix_sum")
    return acc, int(peak.item()) & 0xFFFFFFFF


def mix_power(ctx: Context, acc: torch.Tensor, bits: int, f1: float) -> Tuple[int, int]:
    """-> (max|y1|, sum y1^2 as an exact Python integer) for y1 = audioop.mul(acc, f1), which is not written"""
    p, c, n, ld = _rows(acc, "mix_power")
    need = int(ctx.lib.alsep_mix_power_workspace_bytes(c, n))
    ws = ctx.empty((need // 8,), torch.int64)
    out = ctx.empty((3,), torch.int64)
    ctx.check(ctx.lib.alsep_mix_power(ctx.handle, p, c, n, ld, bits, float(f1), _lib.ptr(ws), need, _lib.ptr(out)), "alsep_mix_power")
    pk, hi, lo = (int(v) & 0xFFFFFFFFFFFFFFFF for v in out.tolist())
    return pk, (hi << 32) + lo


def mix_finish(ctx: Context, acc: torch.Tensor, bits: int, f1: float, f2: float, want_float: bool = False):
    """audioop.mul(audioop.mul(acc, f1), f2) -> int32 [C, N] (and float32 y2 / M with ``want_float``)"""
    p, c, n, ld = _rows(acc, "mix_finish")
    out_i = empty_mix(ctx, c, n)
    out_f = empty_mix(ctx, c, n, torch.float32) if want_float else None
    ip, _, _, ild = _rows(out_i, "mix_finish")
    fp, fld = (None, 0) if out_f is None else (_rows(out_f, "mix_finish")[0], _rows(out_f, "mix_finish")[3])
    ctx.check(ctx.lib.alsep_mix_finish(ctx.handle, p, c, n, ld, bits, float(f1), float(f2), ip, ild, fp, fld), "alsep_mix_finish")
    return (out_i, out_f) if want_float else out_i


# ---- mixdown ------------------------------------------------------------------------------------------------------------------------
def _as_stem(ctx: Context, x) -> torch.Tensor:
    t = torch.as_tensor(x, dtype=torch.float32)
    if t.dim() == 1:
        t = t[None]
    if t.dim() != 2 or t.shape[1] < 1:
        raise AlsepError("mixdown: stems are [channels, samples]")
    return t.to(ctx.device).contiguous()


def grid_of(width: int) -> int:
    """the sample width pydub holds a file of ``width`` bits in, as far as this build goes: 16, or 32 for everything wider"""
    return 16 if width <= 16 else 32


def source_dbfs(source, ctx: Optional[Context] = None, bits: int = 32) -> float:
    """``AudioSegment.from_file(src).dBFS`` (:18-19) of a float32 [C, N] signal on the grid of its own width"""
    ctx = ctx if ctx is not None else _lib.default_context(None)
    g = grid_of(bits)
    acc, _ = mix_sum(ctx, [_as_stem(ctx, source)], [g], g)
    _, s = mix_power(ctx, acc, g, 1.0)
    return ratio_to_db(rms_of(s, acc.shape[0] * acc.shape[1]) / (1 << (g - 1)))


def mixdown_array(stems, source, prevent_clipping: bool = True, bits: Optional[int] = None, src_bits: Optional[Sequence[int]] = None,
                  max_per_launch: int = 0, ctx: Optional[Context] = None) -> Tuple[torch.Tensor, MixRecord]:
    """Mix ``stems`` (float32 [C_k, N_k], device or host; the first one sets the length, a 1-channel stem feeds every channel) and match the
    loudness of ``source``: a float32 [C, N] signal, a ``(signal, width)`` pair when the source is a 16-bit file, or the target dBFS itself.
    ``src_bits``: the source width of every stem (default: ``bits``, or 32); ``bits``: the width of the mix, by default 16 iff every stem's
    width is <= 16, else 32.  ``max_per_launch`` stems per summing launch (0: as many as one holds); the result does not depend on it.
    -> (integer mix on the grid of ``bits``, int32 [C, N] on the device, rows 16-byte aligned; MixRecord)."""
    ctx = ctx if ctx is not None else _lib.default_context(None)
    stems = [_as_stem(ctx, s) for s in stems]
    if not stems:
        raise AlsepError("mixdown: no stems")
    if src_bits is None:
        src_bits = [bits if bits is not None else 32] * len(stems)
    src_bits = [int(b) for b in src_bits]
    if len(src_bits) != len(stems):
        raise AlsepError("mixdown: one source width per stem")
    if bits is None:
        bits = 16 if all(b <= 16 for b in src_bits) else 32
    if bits not in (16, 32) or any(b > bits or b < 2 for b in src_bits):
        raise AlsepError(f"mixdown: a mix of width {bits} cannot hold stems of widths {src_bits}")
    if isinstance(source, (int, float)):
        target = float(source)
    elif isinstance(source, tuple):
        target = source_dbfs(source[0], ctx, int(source[1]))
    else:
        target = source_dbfs(source, ctx)
    acc, peak = mix_sum(ctx, stems, src_bits, bits, max_per_launch)
    if peak == 0:
        return acc, MixRecord(0, 1.0, 0, -math.inf, target, 0.0, 1.0, bits)
    f1 = normalize_factor(peak, bits)
    peak1, s = mix_power(ctx, acc, bits, f1)
    rms = rms_of(s, acc.shape[0] * acc.shape[1])
    current, gain, f2 = match_gain(target, rms, peak1, bits, prevent_clipping)
    out = mix_finish(ctx, acc, bits, f1, f2)
    return out, MixRecord(peak, f1, rms, current, target, gain, f2, bits)


StemInput = Union[str, Tuple[torch.Tensor, int, int]]


def merge_files(paths: Sequence[StemInput], src_file: str, out_path: str, prevent_clipping: bool = True, bits: Optional[int] = None,
                max_per_launch: int = 0, ctx: Optional[Context] = None) -> MixRecord:
    """``paths``: WAV files, or ``(device signal [C, N], sample rate, width)`` for a stem that is already in device memory; ``src_file``: the
    WAV whose loudness the mix is brought to.  Writes ``out_path`` as PCM_16 or PCM_32 according to the width of the mix."""
    ctx = ctx if ctx is not None else _lib.default_context(None)
    stems: List[torch.Tensor] = []
    widths: List[int] = []
    rates: List[int] = []
    for p in paths:
        if isinstance(p, str):
            audio, sr = wavio.read_wav(p)
            _, _, width, _ = wavio.read_wav_info(p)
            stems.append(torch.from_numpy(audio).to(ctx.device))
        else:
            t, sr, width = p
            stems.append(t)
        widths.append(grid_of(width))
        rates.append(int(sr))
    if len(set(rates)) > 1:
        raise ValueError(f"merge: the stems have different sample rates {sorted(set(rates))}; resampling them (audioop.ratecv in pydub) is not "
                         f"built")
    src_audio, _ = wavio.read_wav(src_file)
    src_width = wavio.read_wav_info(src_file)[2]
    mix, rec = mixdown_array(stems, (torch.from_numpy(src_audio).to(ctx.device), src_width), prevent_clipping=prevent_clipping, bits=bits,
                             src_bits=[min(w, bits) for w in widths] if bits else widths, max_per_launch=max_per_launch, ctx=ctx)
    samples = mix.cpu().numpy()
    wavio.write_wav(out_path, samples.astype(np.int16) if rec.bits == 16 else samples, rates[0], subtype="PCM_16" if rec.bits == 16 else "PCM_32")
    return rec
