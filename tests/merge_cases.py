"""Deterministic stem sets for the mixdown (``audiolab_amd.merge``), shared by scripts/make_golden_merge.py -- which runs the stdlib module
``audioop`` (what pydub calls underneath) on them and writes tests/golden/merge.npz -- and by tests/test_merge*.py.  TEST INFRASTRUCTURE.

``reference_mix`` is the pipeline of the reference's wrappers/merge.py:15-45,146-151 as pydub runs it (overlay -> normalize -> dBFS match ->
apply_gain), on integer arrays, with the four ``audioop`` routines passed in: the generator passes the C module, the CPU-only test the numpy
restatements below (``NUMPY_OPS``), which reproduce the fixture exactly and so keep it auditable where ``audioop`` is absent (the module
leaves the standard library with Python 3.13).  The host formulas are those of audiolab_amd/merge.py's docstring, restated here on purpose."""
from __future__ import annotations

import math
import os

import numpy as np

# name -> stems [(channels, samples, gain, source width or 0 = the width of the mix)], source gain (a gain of "square": a +-0.9 square wave of random signs),
#         widths of the mix the case runs at, prevent_clipping, seed
CASES = {
    "three_ragged": dict(stems=[(2, 6001, 0.2, 0), (2, 4000, 0.25, 0), (2, 12002, 0.15, 0)], source=0.1, bits=(16, 32), seed=1),
    "one_stem": dict(stems=[(2, 1500, 0.2, 0)], source=0.1, bits=(16, 32), seed=2),
    "single_sample": dict(stems=[(2, 1, 0.2, 0), (2, 1, 0.2, 0), (2, 5, 0.2, 0)], source=0.1, bits=(16, 32), seed=3),
    "odd_63": dict(stems=[(2, 63, 0.2, 0), (2, 63, 0.2, 0), (2, 61, 0.2, 0)], source=0.1, bits=(16, 32), seed=4),
    "nine_stems": dict(stems=[(2, 4097, 0.1, 0)] * 4 + [(2, 3000, 0.1, 0), (1, 4097, 0.1, 0)] + [(2, 5000, 0.1, 0)] * 3, source=0.1,
                       bits=(16, 32), seed=5),
    "hot": dict(stems=[(2, 1025, "square", 0)] * 3, source=0.1, bits=(16, 32), seed=6),
    "mono_into_stereo": dict(stems=[(2, 1001, 0.2, 0), (1, 1200, 0.2, 0), (2, 900, 0.2, 0)], source=0.1, bits=(16, 32), seed=7),
    "mono_first": dict(stems=[(1, 1001, 0.2, 0), (2, 1200, 0.2, 0)], source=0.1, bits=(16, 32), seed=17),
    "rereverb16": dict(stems=[(2, 2000, 0.2, 32), (2, 2000, 0.2, 32), (2, 2000, 0.2, 16)], source=0.1, bits=(32,), seed=18),
    "all16": dict(stems=[(2, 1003, 0.2, 16), (2, 1003, 0.2, 16), (1, 1003, 0.2, 16)], source=0.1, source_width=16, bits=(16,), seed=9),
    "quiet_source": dict(stems=[(2, 2048, 0.2, 0), (2, 2048, 0.2, 0)], source=0.0267, bits=(16, 32), seed=10),
    "loud_source": dict(stems=[(2, 2048, 0.2, 0), (2, 2048, 0.2, 0)], source=0.8, bits=(16, 32), seed=11),
    "loud_source_free": dict(stems=[(2, 2048, 0.2, 0), (2, 2048, 0.2, 0)], source=0.8, bits=(16, 32), seed=11, prevent_clipping=False),
    "silent_mix": dict(stems=[(2, 515, 0.0, 0), (2, 515, 0.0, 0)], source=0.1, bits=(16, 32), seed=12),
    "silent_source": dict(stems=[(2, 515, 0.2, 0), (2, 515, 0.2, 0)], source=0.0, bits=(16, 32), seed=13),
    "nonfinite": dict(stems=[(2, 777, 0.2, 0), (2, 777, 0.2, 0)], source=0.1, bits=(16, 32), seed=14, nonfinite=True),
}
SOURCE_SAMPLES = 3001
VARIANTS = [(name, bits) for name, case in CASES.items() for bits in case["bits"]]


def _signal(rng, channels: int, n: int, gain) -> np.ndarray:
    """float32 [channels, n]: decaying noise bursts, or a +-0.9 square wave of random signs"""
    if gain == "square":
        return (0.9 * rng.choice([-1.0, 1.0], size=(channels, n))).astype(np.float32)
    t = np.arange(n) / 1000.0
    x = gain * rng.standard_normal((channels, n)) * np.exp(-((t * 3.0) % 1.0) * 2.0)
    return np.clip(x, -1.0, 1.0).astype(np.float32)


def make_case(name: str, bits: int):
    """-> (stems: float32 [C_k, N_k] arrays, their source widths, source float32 [2, SOURCE_SAMPLES], source width, prevent_clipping)"""
    case = CASES[name]
    rng = np.random.default_rng(case["seed"])
    stems = [_signal(rng, c, n, g) for c, n, g, _ in case["stems"]]
    widths = [w if w else bits for _, _, _, w in case["stems"]]
    source = _signal(rng, 2, SOURCE_SAMPLES, case["source"])
    if case.get("nonfinite"):
        stems[0][0, 5], stems[0][1, 9], stems[1][0, 9], stems[1][1, 700] = np.nan, np.inf, -np.inf, np.nan
        stems[1][0, 5] = 0.125                                               # meets the NaN of stem 0: counts as 0 + 0.125
        stems[1][1, 9] = stems[0][0, 9] = 0.0                                # the infinities meet silence: the clip values themselves
    return stems, widths, source, case.get("source_width", bits), case.get("prevent_clipping", True)


# ---- the arithmetic -----------------------------------------------------------------------------------------------------------------
def quantise(x: np.ndarray, width: int, bits: int) -> np.ndarray:
    """q_width(x) << (bits - width): clip(rint(double(x) 2^(width-1))), ties to even, NaN -> 0 (int64)"""
    full = float(1 << (width - 1))
    with np.errstate(invalid="ignore"):
        v = np.rint(x.astype(np.float64) * full)
    v = np.where(np.isnan(v), 0.0, np.clip(v, -full, full - 1.0))
    return v.astype(np.int64) << (bits - width)


def exact_sum_squares(y: np.ndarray) -> int:
    sq = y.astype(np.int64) * y.astype(np.int64)                            # |y| <= 2^31
    return (int(np.sum(sq >> 32, dtype=np.uint64)) << 32) + int(np.sum(sq & 0xFFFFFFFF, dtype=np.uint64))


def np_add(a, b, bits):
    """audioop.add: saturating"""
    full = 1 << (bits - 1)
    return np.clip(a.astype(np.int64) + b.astype(np.int64), -full, full - 1)


def np_mul(a, factor, bits):
    """audioop.mul: floor of the clipped double product (fbound)"""
    full = float(1 << (bits - 1))
    return np.floor(np.clip(a.astype(np.float64) * float(factor), -full, full - 1.0)).astype(np.int64)


def np_max(a, bits):
    """audioop.max: the largest absolute value, unsigned (|-2^31| = 2^31)"""
    return int(np.max(np.abs(a.astype(np.int64)))) if a.size else 0


def np_rms(a, bits):
    """audioop.rms: sqrt(sum of squares / count) truncated.  The C routine sums the squares in a double, sample after sample; this one
    sums exactly.  Both truncate alike wherever the root lies 1e-3 or more from an integer, which the generator asserts per fixture."""
    return int(math.sqrt(exact_sum_squares(a) / a.size)) if a.size else 0


NUMPY_OPS = dict(add=np_add, mul=np_mul, max=np_max, rms=np_rms)


def db_to_float(db):
    return 10 ** (db / 20)


def ratio_to_db(ratio):
    return 20 * math.log10(ratio)


def rms_margin(y: np.ndarray) -> float:
    """distance of sqrt(S / count) from the nearest integer, S the exact sum of squares (inf for S = 0: an all-zero signal has rms 0
    however its squares are summed)"""
    s = exact_sum_squares(y)
    r = math.sqrt(s / y.size)
    return abs(r - round(r)) if s else math.inf


def dbfs(y: np.ndarray, bits: int, ops) -> float:
    rms = ops["rms"](y, bits)
    return ratio_to_db(rms / (1 << (bits - 1))) if rms else -math.inf


def reference_mix(stems, widths, bits: int, source, source_width: int, prevent_clipping: bool, ops) -> dict:
    """-> acc, y2 (int64 [C, N]), peak, f1, peak1, rms, current_dBFS, target_dBFS, gain_dB, f2, margins (of every rms taken)"""
    full = 1 << (bits - 1)
    channels, n = max(s.shape[0] for s in stems), stems[0].shape[1]
    acc = np.zeros((channels, n), dtype=np.int64)
    for k, (s, w) in enumerate(zip(stems, widths)):
        m = min(n, s.shape[1])
        seg = np.ascontiguousarray(np.broadcast_to(quantise(s[:, :m], w, bits), (channels, m)))
        acc[:, :m] = seg if k == 0 else ops["add"](np.ascontiguousarray(acc[:, :m]), seg, bits)
    src_bits = 16 if source_width <= 16 else 32
    src = quantise(source, src_bits, src_bits)
    out = dict(acc=acc, margins=[rms_margin(src)], target_dBFS=dbfs(src, src_bits, ops), peak=ops["max"](acc, bits))
    if out["peak"] == 0:                                                     # normalize returns the segment; zeros stay zeros
        out.update(y2=acc.copy(), f1=1.0, peak1=0, rms=0, current_dBFS=-math.inf, gain_dB=0.0, f2=1.0)
        return out
    f1 = db_to_float(ratio_to_db(full * db_to_float(-0.1) / out["peak"]))
    y1 = ops["mul"](acc, f1, bits)
    out["margins"].append(rms_margin(y1))
    rms, peak1 = ops["rms"](y1, bits), ops["max"](y1, bits)
    current = ratio_to_db(rms / full) if rms else -math.inf
    gain = -math.inf if out["target_dBFS"] == -math.inf else out["target_dBFS"] - current
    if prevent_clipping:
        gain = min(gain, -20 * math.log10(peak1 / full))
    f2 = db_to_float(gain)
    out.update(y2=ops["mul"](y1, f2, bits), f1=f1, peak1=peak1, rms=rms, current_dBFS=current, gain_dB=gain, f2=f2)
    return out


_GOLDEN = {}


def fixture_of(golden_dir: str, name: str, bits: int) -> dict:
    """tests/golden/merge.npz for one case at one width: acc, y2 (int64), peak, peak1, rms, f1, f2, current, target, gain"""
    if not _GOLDEN:
        with np.load(os.path.join(golden_dir, "merge.npz")) as z:
            _GOLDEN.update({k: z[k] for k in z.files})
    key = f"{name}_{bits}"
    peak, peak1, rms = (int(v) for v in _GOLDEN[f"{key}_ints"])
    f1, f2, current, target, gain = (float(v) for v in _GOLDEN[f"{key}_floats"])
    return dict(acc=_GOLDEN[f"{key}_acc"].astype(np.int64), y2=_GOLDEN[f"{key}_y2"].astype(np.int64), peak=peak, peak1=peak1, rms=rms, f1=f1,
                f2=f2, current=current, target=target, gain=gain)
