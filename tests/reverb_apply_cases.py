"""Deterministic (dry, impulse response, pre-delay) cases for the convolution reverb (``audiolab_amd.reverb.apply_reverb``), shared by
scripts/make_golden_reverb_apply.py -- which runs the reference's ``apply_reverb`` (handlers/reverb.py:179-209) on them and writes
tests/golden/reverb_apply.npz -- and by tests/test_reverb_apply.py.  TEST INFRASTRUCTURE.  The dry arrays are what the reference's
``read_audio`` returns (:22-36): float32, ``[N, C]`` for multi-channel files, ``[N]`` for mono ones.

Block counts at the default block length F = max(2^ceil(log2(2 L)), 1024), S = F - L + 1 new samples per block."""
from __future__ import annotations

import numpy as np

WET_GAIN = 0.7                                                               # handlers/reverb.py:205

# name -> (sample rate, samples, channels (0 = a 1-D mono array), IR taps L, pre-delay seconds, dry gain, seed)
CASES = {
    "tiny_stereo": (8000, 6001, 2, 300, 0.0, 0.25, 1),                       # 9 blocks of 1024, ragged last block
    "mono_delay": (16000, 20000, 0, 1200, 0.01, 0.25, 2),                    # zero imaginary half, shift of 160 samples
    "ir_longer": (44100, 48000, 2, 88200, 0.037, 0.25, 3),                   # IR longer than the track, the 2 s cap at 44.1 kHz: one 2^18 block
    "clip_stereo": (8000, 9000, 2, 500, 0.002, 1.2, 4),                      # the clip is active on both sides
    "three_ch": (8000, 5000, 3, 257, 0.001, 0.25, 5),                        # odd channel count, odd L
    "delay_past_end": (8000, 4000, 2, 300, 0.75, 0.25, 6),                   # pre-delay >= n: clip(dry) exactly
    "block_multiple": (8000, 4 * (1024 - 300 + 1), 2, 300, 0.0, 0.25, 7),    # the track ends exactly on a block boundary
    "unit_ir": (8000, 3000, 2, 1, 0.0, 0.25, 8),                             # L = 1, S = F
}

# cases whose fixture holds the first HEAD samples plus N_PROBE seeded positions instead of the whole signal
SAMPLED = ("ir_longer",)
HEAD, N_PROBE = 4096, 4096


def make_case(name: str):
    """-> (dry float32 [N, C] or [N], ir float64 [L], pre_delay seconds, sr): dry = gain * (decaying noise bursts + a tone per channel)
    clipped to +-1, as oracle/reverb_cases.make_case builds its dry signal; ir = exponentially decaying noise with a unit direct path,
    normalised to unit energy."""
    sr, n, ch, taps, pre_delay, gain, seed = CASES[name]
    rng = np.random.default_rng(seed)
    c = max(ch, 1)
    t = np.arange(n) / sr
    dry = np.zeros((n, c))
    for k in range(c):
        bursts = rng.standard_normal(n) * (np.exp(-((t * 3.0 + 0.37 * k) % 1.0) * 6.0))
        dry[:, k] = gain * (bursts + 0.4 * np.sin(2 * np.pi * (220.0 + 110.0 * k) * t) * np.exp(-t * 1.5))
    dry32 = np.clip(dry, -1.0, 1.0).astype(np.float32)
    ir = rng.standard_normal(taps) * np.exp(-np.arange(taps) / (taps / 6.9))
    ir[0] = 1.0
    ir /= np.sqrt(np.sum(ir ** 2))
    return (dry32[:, 0].copy() if ch == 0 else dry32), ir, pre_delay, sr


def positions(name: str) -> np.ndarray:
    """the sample indices the fixture holds for ``name`` (every channel at the same ones)"""
    n = CASES[name][1]
    if name not in SAMPLED:
        return np.arange(n)
    probes = np.random.default_rng(CASES[name][6] + 100).integers(HEAD, n, size=N_PROBE)
    return np.concatenate([np.arange(HEAD), np.sort(probes)])


def chan_major(x: np.ndarray) -> np.ndarray:
    """the reference's [N, C] / [N] arrays -> this build's [C, N]"""
    return np.ascontiguousarray(x.T if x.ndim == 2 else x[None])


def exact_final(dry: np.ndarray, ir: np.ndarray, pre: int, pos: np.ndarray, gain: float = WET_GAIN) -> np.ndarray:
    """clip(dry + gain * wet) at ``pos`` with the convolution as long-double dot products (64-bit mantissa: ~1e-19 per term) -> float64
    [len(pos), C] (or [len(pos)] for 1-D input).  ``gain`` is the double constant the reference multiplies by."""
    x = chan_major(dry).astype(np.longdouble)
    h = ir.astype(np.longdouble)
    n = x.shape[1]
    if len(pos) == n and pre < n:                                            # the whole signal: one long-double convolution per channel
        wet = np.zeros_like(x)
        for c in range(x.shape[0]):
            wet[c, pre:] = np.convolve(x[c], h)[: n - pre]
        wet = wet[:, pos]
    else:
        wet = np.zeros((x.shape[0], len(pos)), dtype=np.longdouble)
        hr = h[::-1]
        for i, o in enumerate(pos):
            t = int(o) - pre                                                 # wet[o] = conv[t] = sum_j h[j] x[t - j]
            if t < 0:
                continue
            m = min(t + 1, len(h))
            wet[:, i] = x[:, t - m + 1: t + 1] @ hr[len(h) - m:]
    final = np.clip(x[:, pos] + np.longdouble(gain) * wet, -1.0, 1.0).astype(np.float64)
    return final[0] if dry.ndim == 1 else np.ascontiguousarray(final.T)
