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

Stems of differing sample rates.  ``AudioSegment.overlay`` first brings both segments to the larger frame rate (``_sync`` ->
``set_frame_rate`` -> ``audioop.ratecv(data, width, channels, rate, new_rate, None)``: linear interpolation on 32-bit values, truncated toward
zero), before the sample widths meet.  With R the running rate of the mix: a stem below R is resampled on its own width's grid and then
shifted up; a stem above R has the running mix -- the saturated sum so far -- resampled on the grid of the widest stem in it, the mix takes
the new length and R becomes the stem's rate; the file is written at the final R.  ``alsep_mix_sum_rates`` (the fourth pass of
csrc/mixdown.h) does the interpolation inside the sum; every rise of R is a launch boundary (``plan_rates``).  The ``ratecv`` arithmetic is
pinned by tests/golden/merge_rates.npz (scripts/make_golden_merge_rates.py).  ``merge_files(mixed_rates="ratecv")`` switches it on; the
default, ``"error"``, raises as before.

Departures from the reference: lengths are sample-exact (pydub slices by milliseconds); float samples reach the integer grid by
``clip(rint(x 2^(b-1)))`` on the stem's own width b (the reference's conversion goes through ffmpeg); the width of the mix is fixed from the
start (pydub widens it when a wider stem arrives); ``ratecv``'s filter weights and state, which pydub never passes, are not built.
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
    rate: int = 0              # the sample rate of the mix: the largest one given (0: no rates were given)

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


# ---- stems of differing sample rates ----------------------------------------------------------------------------------------------------
RATE_MAX = 1 << 20                                                           # of a rate divided by the pair's gcd


def ratecv_length(n: int, in_rate: int, out_rate: int) -> int:
    """samples ``audioop.ratecv`` returns for ``n`` input samples: floor((n - 1) outr / inr) + 1 on the reduced pair"""
    n, in_rate, out_rate = int(n), int(in_rate), int(out_rate)
    if n < 1 or in_rate < 1 or out_rate < 1:
        raise AlsepError(f"ratecv: {n} samples from rate {in_rate} to {out_rate}")
    g = math.gcd(in_rate, out_rate)
    inr, outr = in_rate // g, out_rate // g
    if inr > RATE_MAX or outr > RATE_MAX:
        raise AlsepError(f"ratecv: the rates {in_rate} -> {out_rate} reduce to {inr} -> {outr}, above {RATE_MAX}")
    return (n - 1) * outr // inr + 1


@dataclass
class RateLaunch:
    """one launch of the resampling sum pass"""
    mix: Optional[Tuple[int, int]]                       # None: no mix yet; (R, R): the mix as it is; (R, R'): the mix resampled
    mix_width: int                                       # the grid the mix is resampled on: the widest stem in it
    stems: List[Tuple[int, Optional[Tuple[int, int]]]]   # (index of the stem, its rate pair or None)
    rate: int                                            # the running rate R after this launch
    length: Optional[int] = None                         # samples per row of the mix after this launch (when the first length was given)


def plan_rates(rates: Sequence[int], widths: Sequence[int], max_per_launch: int = 0, n: Optional[int] = None) -> List[RateLaunch]:
    """Host only.  The launches that mix stems of the given rates and source widths in pydub's order: the running rate R starts as the first
    stem's; a stem below R carries the pair (its rate, R); a stem above R starts a new launch whose first operand is the mix carrying
    (R, its rate) -- every earlier add has to be complete before the mix is resampled -- and R becomes its rate.  No launch holds more
    than ``max_per_launch`` stems (0: as many as one holds), nor more than ALSEP_MIX_MAX_STEMS operands with the mix."""
    rates, widths = [int(r) for r in rates], [int(w) for w in widths]
    if not rates or len(rates) != len(widths):
        raise AlsepError("plan_rates: one rate and one width per stem, at least one stem")
    if any(r < 1 for r in rates):
        raise AlsepError(f"plan_rates: sample rates are positive, got {rates}")
    per = _lib.MIX_MAX_STEMS if max_per_launch <= 0 else min(int(max_per_launch), _lib.MIX_MAX_STEMS)
    rate, length = rates[0], n
    launches: List[RateLaunch] = []
    cur = RateLaunch(None, 0, [], rate, length)
    for k, r in enumerate(rates):
        if r > rate:
            if cur.stems or cur.mix is not None:
                launches.append(cur)
            length = None if length is None else ratecv_length(length, rate, r)
            cur = RateLaunch((rate, r), max(widths[:k]), [], r, length)
            rate = r
        elif len(cur.stems) >= min(per, _lib.MIX_MAX_STEMS - (cur.mix is not None)):
            launches.append(cur)
            cur = RateLaunch((rate, rate), max(widths[:k]), [], rate, length)
        cur.stems.append((k, (r, rate) if r < rate else None))
    launches.append(cur)
    return launches


def _mix_sum_rates(ctx: Context, operands, channels: int, n_out: int, bits: int, acc: torch.Tensor, peak: torch.Tensor) -> None:
    arr = (_lib.MixOperand * len(operands))(*operands)
    p, _, _, ld = _rows(acc, "mix_sum_rates")
    ctx.check(ctx.lib.alsep_mix_sum_rates(ctx.handle, arr, len(operands), channels, n_out, bits, p, ld, _lib.ptr(peak)), "alsep_mix_sum_rates")


def mix_sum_rates(ctx: Context, stems: Sequence[torch.Tensor], widths: Sequence[int], rates: Sequence[int], bits: int,
                  max_per_launch: int = 0) -> Tuple[torch.Tensor, int, int]:
    """``mix_sum`` for stems of differing sample rates -> (int32 mix [C, N] at the largest rate, max|mix|, that rate)"""
    if not stems or len(stems) != len(widths) or len(stems) != len(rates):
        raise AlsepError("mix_sum_rates: one width and one rate per stem, at least one stem")
    c = max(s.shape[0] for s in stems)
    peak = ctx.empty((1,), torch.int32)
    acc = None
    for launch in plan_rates(rates, widths, max_per_launch, stems[0].shape[1]):
        operands = []
        if launch.mix is not None:
            p, _, n, ld = _rows(acc, "mix_sum_rates")
            resampled = launch.mix[0] != launch.mix[1]
            operands.append(_lib.MixOperand(p, n, ld, launch.mix[0], launch.mix[1], c, launch.mix_width if resampled else bits, 1))
            if resampled:                                                    # a resampled mix must not be acc itself
                old, acc = acc, empty_mix(ctx, c, launch.length)             # noqa: F841 (the operand, alive until the launch is queued)
        else:
            acc = empty_mix(ctx, c, launch.length)
        for k, pair in launch.stems:
            s = stems[k]
            if s.dtype != torch.float32:
                raise AlsepError("mix_sum_rates: stems are float32")
            p, ck, nk, ld = _rows(s, f"mix_sum_rates: stem {k}")
            if ck not in (1, c):
                raise AlsepError(f"mix_sum_rates: stem {k} has {ck} channels, the mix {c}")
            operands.append(_lib.MixOperand(p, nk, ld, pair[0] if pair else 0, pair[1] if pair else 0, ck, int(widths[k]), 0))
        _mix_sum_rates(ctx, operands, c, launch.length, bits, acc, peak)
        rate = launch.rate
    return acc, int(peak.item()) & 0xFFFFFFFF, rate


def ratecv_array(x, in_rate: int, out_rate: int, width: int, ctx: Optional[Context] = None) -> torch.Tensor:
    """``audioop.ratecv(x, width // 8, channels, in_rate, out_rate, None)`` -> int32 [C, K] on the grid of ``width`` (16 or 32), K =
    ``ratecv_length``.  ``x`` [C, N]: float32, quantised on that grid first, or int32 samples already on it."""
    ctx = ctx if ctx is not None else _lib.default_context(None)
    t = torch.as_tensor(x)
    is_int = t.dtype == torch.int32
    if not is_int:
        t = t.to(torch.float32)
    if t.dim() == 1:
        t = t[None]
    t = t.to(ctx.device).contiguous()
    p, c, n, ld = _rows(t, "ratecv_array")
    if width not in (16, 32):
        raise AlsepError(f"ratecv_array: width {width}, expected 16 or 32")
    k = ratecv_length(n, in_rate, out_rate)
    out, peak = empty_mix(ctx, c, k), ctx.empty((1,), torch.int32)
    _mix_sum_rates(ctx, [_lib.MixOperand(p, n, ld, int(in_rate), int(out_rate), c, int(width), 1 if is_int else 0)], c, k, int(width), out, peak)
    return out


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
                  max_per_launch: int = 0, ctx: Optional[Context] = None, rates: Optional[Sequence[int]] = None) -> Tuple[torch.Tensor, MixRecord]:
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
    rate = 0
    if rates is not None:
        rates = [int(r) for r in rates]
        if len(rates) != len(stems):
            raise AlsepError("mixdown: one sample rate per stem")
        rate = max(rates)
    if rates is not None and len(set(rates)) > 1:
        acc, peak, rate = mix_sum_rates(ctx, stems, src_bits, rates, bits, max_per_launch)
    else:
        acc, peak = mix_sum(ctx, stems, src_bits, bits, max_per_launch)
    if peak == 0:
        return acc, MixRecord(0, 1.0, 0, -math.inf, target, 0.0, 1.0, bits, rate)
    f1 = normalize_factor(peak, bits)
    peak1, s = mix_power(ctx, acc, bits, f1)
    rms = rms_of(s, acc.shape[0] * acc.shape[1])
    current, gain, f2 = match_gain(target, rms, peak1, bits, prevent_clipping)
    out = mix_finish(ctx, acc, bits, f1, f2)
    return out, MixRecord(peak, f1, rms, current, target, gain, f2, bits, rate)


StemInput = Union[str, Tuple[torch.Tensor, int, int]]


def merge_files(paths: Sequence[StemInput], src_file: str, out_path: str, prevent_clipping: bool = True, bits: Optional[int] = None,
                max_per_launch: int = 0, ctx: Optional[Context] = None, mixed_rates: str = "error") -> MixRecord:
    """``paths``: WAV files, or ``(device signal [C, N], sample rate, width)`` for a stem that is already in device memory; ``src_file``: the
    WAV whose loudness the mix is brought to.  Writes ``out_path`` as PCM_16 or PCM_32 according to the width of the mix.  ``mixed_rates``:
    what to do with stems of differing sample rates -- ``"error"``: ValueError; ``"ratecv"``: resample as pydub's overlay does and write the
    file at the largest rate."""
    if mixed_rates not in ("error", "ratecv"):
        raise ValueError(f"merge: mixed_rates is 'error' or 'ratecv', not {mixed_rates!r}")
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
    if len(set(rates)) > 1 and mixed_rates == "error":
        raise ValueError(f"merge: the stems have different sample rates {sorted(set(rates))}; mixed_rates='ratecv' resamples them as pydub "
                         f"does (audioop.ratecv)")
    src_audio, _ = wavio.read_wav(src_file)
    src_width = wavio.read_wav_info(src_file)[2]
    mix, rec = mixdown_array(stems, (torch.from_numpy(src_audio).to(ctx.device), src_width), prevent_clipping=prevent_clipping, bits=bits,
                             src_bits=[min(w, bits) for w in widths] if bits else widths, max_per_launch=max_per_launch, ctx=ctx,
                             rates=rates if len(set(rates)) > 1 else None)
    samples = mix.cpu().numpy()
    wavio.write_wav(out_path, samples.astype(np.int16) if rec.bits == 16 else samples, rec.rate or rates[0], subtype="PCM_16" if rec.bits == 16 else "PCM_32")
    return rec
