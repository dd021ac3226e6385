"""Stems of differing sample rates for the mixdown (``audiolab_amd.merge``: ``ratecv_array``, ``mixdown_array(rates=...)``), shared by
scripts/make_golden_merge_rates.py -- which runs the stdlib module ``audioop`` on them and writes tests/golden/merge_rates.npz -- and by
tests/test_merge_rates*.py.  TEST INFRASTRUCTURE, beside tests/merge_cases.py, whose signals, quantiser and numpy restatements it uses.

``np_ratecv`` is the closed form of ``audioop.ratecv(data, width, channels, in_rate, out_rate, None)`` (weightA = 1, weightB = 0, no state):
linear interpolation on samples shifted to 32 bits, truncated toward zero.  ``reference_mix_rates`` walks pydub's overlay chain --
``_sync`` brings both segments to the larger channel count (``tostereo``), then to the larger frame rate (``ratecv``), then to the larger
sample width (``lin2lin``) -- in this project's model of the mix (an integer container on the grid of ``bits``, fixed from the start; the
running mix is resampled on the grid of the widest stem in it), with the ``audioop`` routines passed in: the generator passes the C module,
the CPU-only test the numpy restatements (``NUMPY_RATE_OPS``).  pydub's control flow is restated from its published source and unpinned.

Fixture layout.  ``ratecv`` outputs of at most ``FULL_BELOW`` input samples are stored whole; of the longer inputs the SHA-256 of the
little-endian int32 [C, K] result and K are stored (the 24-fold rise alone would otherwise outweigh every other fixture): equality of the
digest is equality of every sample."""
from __future__ import annotations

import hashlib
import math
import os
import zlib

import numpy as np

from tests.merge_cases import NUMPY_OPS, SOURCE_SAMPLES, _signal, dbfs, db_to_float, quantise, ratio_to_db, rms_margin

# ---- ratecv alone ---------------------------------------------------------------------------------------------------------------------
PAIRS = [(44100, 48000), (48000, 44100), (40000, 44100), (22050, 44100), (44100, 22050), (8000, 192000), (192000, 8000), (44100, 44101),
         (1048573, 1048576)]
WIDTHS = (16, 32)
CHANNELS = (1, 2)
LENGTHS = (1, 2, 3, 5, 147, 1000, 4099)
FULL_BELOW = 147


def ratecv_key(pair, width: int, channels: int, n: int) -> str:
    return f"rcv_{pair[0]}_{pair[1]}_{width}_{channels}_{n}"


def ratecv_input(pair, width: int, channels: int, n: int) -> np.ndarray:
    """float32 [channels, n] in [-1, 1]: full-range noise with the extremes of the grid planted side by side (-1.0 quantises to INT_MIN of
    the width, +1.0 clips to INT_MAX), so that products of magnitude 2^31 meet and a negative quotient has to be truncated, not floored"""
    rng = np.random.default_rng(zlib.crc32(ratecv_key(pair, width, channels, n).encode()))
    x = rng.uniform(-1.0, 1.0, size=(channels, n)).astype(np.float32)
    runs = ([1.0, -1.0], [-1.0, -1.0, 1.0], [-1.0, 1.0, 1.0, -1.0, -1.0])     # the last one is placed last and stays whole
    for c in range(channels):
        for run in runs:
            if n >= len(run):
                p = int(rng.integers(0, n - len(run) + 1))
                x[c, p:p + len(run)] = run
    if n <= 3:
        x[:, 0] = -1.0 if width == 16 else 1.0                               # the first output is trunc(x[0] ...): one extreme each
    return x


def ratecv_length(n: int, in_rate: int, out_rate: int) -> int:
    g = math.gcd(in_rate, out_rate)
    return (n - 1) * (out_rate // g) // (in_rate // g) + 1


def np_ratecv(u: np.ndarray, width: int, in_rate: int, out_rate: int) -> np.ndarray:
    """audioop.ratecv(u, width // 8, channels, in_rate, out_rate, None) on int64 [C, N] samples of the grid of ``width`` -> int64 [C, K].
    Output k: j = ceil(k inr / outr), d = j outr - k inr, trunc((x[j-1] d + x[j] (outr - d)) / outr) >> (32 - width) with x = u << (32 -
    width) and x[-1] = 0.  The C routine divides in doubles; the numerator is an integer below 2^31 outr, exact in a double, and a correctly
    rounded quotient cannot reach the next integer while outr < 2^21, so the integer division here truncates alike."""
    g = math.gcd(in_rate, out_rate)
    inr, outr = in_rate // g, out_rate // g
    n = u.shape[1]
    k = np.arange((n - 1) * outr // inr + 1, dtype=np.int64)
    j = -((-k * inr) // outr)
    d = j * outr - k * inr
    sh = 32 - width
    x = u.astype(np.int64) << sh
    cur = x[:, j]
    prev = np.where(j > 0, x[:, np.maximum(j - 1, 0)], 0)
    num = prev * d + cur * (outr - d)
    return (np.sign(num) * (np.abs(num) // outr)) >> sh


def digest(a: np.ndarray) -> np.ndarray:
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).astype("<i4").tobytes()).digest(), dtype=np.uint8)


# ---- chains ---------------------------------------------------------------------------------------------------------------------------
# name -> stems [(channels, samples, gain, source width or 0 = the width of the mix, sample rate)], widths of the mix, seed
CHAINS = {
    # (a) the mix is resampled, then a later stem below the new rate
    "rise_then_lower": dict(stems=[(2, 3001, 0.2, 0, 44100), (2, 3300, 0.25, 0, 48000), (2, 2800, 0.15, 0, 44100)], bits=(16, 32), seed=101),
    # (b) two hot stems saturate the mix, which is then resampled
    "hot_rise": dict(stems=[(2, 1025, "square", 0, 44100)] * 2 + [(2, 1200, 0.2, 0, 48000)], bits=(16, 32), seed=102),
    # (c) a 16-bit mono stem below the rate: resampled on the 16-bit grid, then fed to both channels of a 32-bit mix
    "narrow_mono_lower": dict(stems=[(2, 2003, 0.2, 32, 48000), (1, 1700, 0.3, 16, 40000)], bits=(32,), seed=103),
    # (d) two rises
    "two_rises": dict(stems=[(2, 1001, 0.2, 0, 22050), (2, 2100, 0.2, 0, 44100), (2, 2000, 0.2, 0, 48000)], bits=(16, 32), seed=104),
    # (e) stems that end before and after the mix (1088 samples once resampled), as they are and resampled
    "ragged_ends": dict(stems=[(2, 1000, 0.2, 0, 44100), (2, 500, 0.2, 0, 48000), (2, 3000, 0.2, 0, 48000), (2, 700, 0.2, 0, 40000),
                               (1, 2000, 0.2, 0, 32000)], bits=(16, 32), seed=105),
    # (f) nine stems, the rise at the fifth, lower rates after it, one mono
    "nine_rise_at_5": dict(stems=[(2, 2049, 0.1, 0, 44100)] * 4 + [(2, 2300, 0.1, 0, 48000), (2, 1500, 0.1, 0, 44100), (1, 2231, 0.1, 0, 48000),
                                  (2, 2500, 0.1, 0, 40000), (2, 2231, 0.1, 0, 48000)], bits=(16, 32), seed=106),
    # a saturated mix of 16-bit stems in a 32-bit container is resampled on the 16-bit grid (2^31 - 1 >> 16), a 32-bit stem follows
    "narrow_mix_rises": dict(stems=[(2, 1025, "square", 16, 44100)] * 2 + [(2, 1300, 0.2, 32, 48000)], bits=(32,), seed=107),
}
CHAIN_VARIANTS = [(name, bits) for name, case in CHAINS.items() for bits in case["bits"]]
SOURCE_GAIN = 0.1


def make_chain(name: str, bits: int):
    """-> (stems: float32 [C_k, N_k] arrays, their source widths, their sample rates, source float32 [2, SOURCE_SAMPLES])"""
    case = CHAINS[name]
    rng = np.random.default_rng(case["seed"])
    stems = [_signal(rng, c, n, g) for c, n, g, _, _ in case["stems"]]
    widths = [w if w else bits for _, _, _, w, _ in case["stems"]]
    rates = [r for _, _, _, _, r in case["stems"]]
    return stems, widths, rates, _signal(rng, 2, SOURCE_SAMPLES, SOURCE_GAIN)


def np_lin2lin(a, width, new_width):
    """audioop.lin2lin: the top bytes when narrowing (an arithmetic shift), zeros below when widening"""
    a = a.astype(np.int64)
    return a >> (width - new_width) if new_width < width else a << (new_width - width)


NUMPY_RATE_OPS = dict(NUMPY_OPS, ratecv=np_ratecv, lin2lin=np_lin2lin, tostereo=lambda a, width: np.concatenate([a, a], axis=0))


def reference_mix_rates(stems, widths, rates, bits: int, source, prevent_clipping: bool, ops) -> dict:
    """-> rate, acc, y2 (int64 [C, N] at the final rate), peak, f1, peak1, rms, current_dBFS, target_dBFS, gain_dB, f2, margins"""
    full = 1 << (bits - 1)
    channels = max(s.shape[0] for s in stems)
    rate, w_run, acc = rates[0], widths[0], None
    for k, (s, w, r) in enumerate(zip(stems, widths, rates)):
        seg = quantise(s, w, w)                                              # the stem on its own grid
        if seg.shape[0] < channels:
            assert seg.shape[0] == 1 and channels == 2
            seg = ops["tostereo"](seg, w)
        if acc is not None and r > rate:                                     # the running mix goes to the stem's rate, on the grid of the widest stem in it
            acc = ops["lin2lin"](ops["ratecv"](ops["lin2lin"](acc, bits, w_run), w_run, rate, r), w_run, bits)
            rate = r
        elif r < rate:
            seg = ops["ratecv"](seg, w, r, rate)
        seg = ops["lin2lin"](seg, w, bits)
        if acc is None:
            acc = seg.astype(np.int64)
        else:
            m = min(acc.shape[1], seg.shape[1])
            acc[:, :m] = ops["add"](np.ascontiguousarray(acc[:, :m]), np.ascontiguousarray(seg[:, :m]), bits)
        w_run = max(w_run, w)
    src = quantise(source, bits, bits)
    out = dict(rate=rate, acc=acc, margins=[rms_margin(src)], target_dBFS=dbfs(src, bits, ops), peak=ops["max"](acc, bits))
    assert out["peak"] > 0
    f1 = db_to_float(ratio_to_db(full * db_to_float(-0.1) / out["peak"]))
    y1 = ops["mul"](acc, f1, bits)
    out["margins"].append(rms_margin(y1))
    rms, peak1 = ops["rms"](y1, bits), ops["max"](y1, bits)
    current = ratio_to_db(rms / full)
    gain = out["target_dBFS"] - current
    if prevent_clipping:
        gain = min(gain, -20 * math.log10(peak1 / full))
    f2 = db_to_float(gain)
    out.update(y2=ops["mul"](y1, f2, bits), f1=f1, peak1=peak1, rms=rms, current_dBFS=current, gain_dB=gain, f2=f2)
    return out


# ---- the fixture ----------------------------------------------------------------------------------------------------------------------
_GOLDEN = {}


def _golden(golden_dir: str) -> dict:
    if not _GOLDEN:
        with np.load(os.path.join(golden_dir, "merge_rates.npz")) as z:
            _GOLDEN.update({k: z[k] for k in z.files})
    return _GOLDEN


def ratecv_fixture(golden_dir: str, pair, width: int, channels: int, n: int):
    """-> (the int64 [C, K] result or None, its SHA-256, K)"""
    g, key = _golden(golden_dir), ratecv_key(pair, width, channels, n)
    if key in g:
        full = g[key].astype(np.int64)
        return full, digest(full), full.shape[1]
    return None, g[key + "_sha"], int(g[key + "_len"])


def chain_fixture(golden_dir: str, name: str, bits: int) -> dict:
    g, key = _golden(golden_dir), f"chain_{name}_{bits}"
    peak, peak1, rms, rate = (int(v) for v in g[f"{key}_ints"])
    f1, f2, current, target, gain = (float(v) for v in g[f"{key}_floats"])
    return dict(acc=g[f"{key}_acc"].astype(np.int64), y2=g[f"{key}_y2"].astype(np.int64), peak=peak, peak1=peak1, rms=rms, rate=rate, f1=f1,
                f2=f2, current=current, target=target, gain=gain)
