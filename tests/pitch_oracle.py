"""The phase-locked vocoder pitch shifter of audiolab_amd/pitch.py restated in numpy float64, independently of the kernels
(csrc/pitch.h): the specification, step by step.  Not a restatement of any reference code: the reference shells out to ffmpeg's
rubberband filter, which is not available -- parity with it is unpinned.

  r = 2^(s/12); n = n_fft; hs = n/4; K = n/2 + 1; w = periodic Hann
  1. analysis   ha = hs / r; U = ceil(N / ha) + 1; a_u = floor(u ha); frame u = x[a_u - n/2 .. a_u + n/2) w (zeros outside [0, N));
                D = rfft(frame); mag = |D|; pa = atan2(im, re), atan2(0, 0) = 0
  2. peaks      k is a peak iff mag[k] > mag[k-1], mag[k] > mag[k-2], mag[k] >= mag[k+1], mag[k] >= mag[k+2] (bins outside count as -1);
                own[k] = the nearest peak, the lower one on equal distance; no peak: own[k] = k
  3. phases     ps_0 = pa_0; inc[k] = (om_k + wrap(pa_u[k] - pa_{u-1}[k] - om_k da) / da) hs, om_k = 2 pi k / n, da = a_u - a_{u-1};
                ps_u[k] = wrap(ps_{u-1}[own[k]] + inc[own[k]] + pa_u[k] - pa_u[own[k]]); wrap(d) = d - 2 pi round(d / 2 pi), ties to even
  4. synthesis  y_u = irfft(mag_u exp(i ps_u)); z = overlap-add of w y_u at hop hs over the envelope of w^2 (1 where it is <= 1e-10),
                Lz = (U - 1) hs + n/2 samples, sample 0 = the centre of frame 0
  5. resampling out[m] = sum_i z[i] g(m r - i), |m r - i| <= half; g(t) = c sinc(c t) I0(beta sqrt(1 - (t / half)^2)) / I0(beta),
                c = roll min(1, 1/r), half = Z / c
"""
import math

import numpy as np

ZEROS = 64
BETA = 14.769656459379492
ROLLOFF = 0.9475937167399596
TWO_PI = 2.0 * math.pi


def ratio(semitones) -> float:
    return 2.0 ** (semitones / 12.0)


def wrap(d):
    return d - TWO_PI * np.round(d / TWO_PI)


def hann(n: int) -> np.ndarray:
    return 0.5 - 0.5 * np.cos(TWO_PI * np.arange(n) / n)


def frame_count(n_samples: int, n_fft: int, r: float) -> int:
    return int(math.ceil(n_samples / ((n_fft // 4) / r))) + 1


def owners(mag: np.ndarray) -> np.ndarray:
    """own[k] for one frame's magnitudes"""
    K = len(mag)
    p = np.concatenate([[-1.0, -1.0], mag, [-1.0, -1.0]])
    c = p[2:-2]
    peak = (c > p[1:-3]) & (c > p[:-4]) & (c >= p[3:-1]) & (c >= p[4:])
    idx = np.nonzero(peak)[0]
    k = np.arange(K)
    if len(idx) == 0:
        return k
    pos = np.searchsorted(idx, k, side="right")                              # peaks <= k
    lo = idx[np.clip(pos - 1, 0, len(idx) - 1)]
    hi = idx[np.clip(pos, 0, len(idx) - 1)]
    lo_ok, hi_ok = pos > 0, pos < len(idx)
    take_lo = lo_ok & (~hi_ok | (k - lo <= hi - k))
    return np.where(take_lo, lo, hi)


def stretch(x: np.ndarray, r: float, n_fft: int):
    """steps 1-4 for one channel -> z (float64, Lz samples)"""
    n, hs, K = n_fft, n_fft // 4, n_fft // 2 + 1
    N = len(x)
    ha = hs / r
    U = int(math.ceil(N / ha)) + 1
    a = [int(math.floor(u * ha)) for u in range(U)]
    w = hann(n)
    om = TWO_PI * np.arange(K) / n
    xp = np.concatenate([np.zeros(n // 2), x.astype(np.float64), np.zeros(a[-1] + n)])
    Lz = (U - 1) * hs + n // 2
    z = np.zeros(Lz + n)                                                     # index i + n/2
    env = np.zeros(Lz + n)
    w2 = w * w
    ps_prev = pa_prev = None
    for u in range(U):
        D = np.fft.rfft(xp[a[u]: a[u] + n] * w)
        mag = np.abs(D)
        pa = np.where((D.real == 0) & (D.imag == 0), 0.0, np.arctan2(D.imag, D.real))
        if u == 0:
            ps = pa
        else:
            da = a[u] - a[u - 1]
            own = owners(mag)
            inc = (om + wrap(pa - pa_prev - om * da) / da) * hs
            ps = wrap(ps_prev[own] + (inc[own] + pa - pa[own]))
        y = np.fft.irfft(mag * (np.cos(ps) + 1j * np.sin(ps)), n)
        z[u * hs: u * hs + n] += w * y
        env[u * hs: u * hs + n] += w2
        ps_prev, pa_prev = ps, pa
    z, env = z[n // 2: n // 2 + Lz], env[n // 2: n // 2 + Lz]
    return z / np.where(env > 1e-10, env, 1.0)


def kaiser_sinc(t: np.ndarray, c: float, half: float) -> np.ndarray:
    q = 1.0 - (t / half) ** 2
    return np.where(q >= 0, c * np.sinc(c * t) * np.i0(BETA * np.sqrt(np.maximum(q, 0.0))) / np.i0(BETA), 0.0)


def resample_at(z: np.ndarray, r: float, positions: np.ndarray) -> np.ndarray:
    """step 5 at the given output positions only"""
    c = ROLLOFF * min(1.0, 1.0 / r)
    half = ZEROS / c
    m = np.asarray(positions, dtype=np.int64)
    t0 = m * r
    first = np.ceil(t0 - half).astype(np.int64)
    out = np.zeros(len(m))
    for j in range(int(2 * half) + 2):
        i = first + j
        t = t0 - i
        ok = (i >= 0) & (i < len(z)) & (np.abs(t) <= half)
        out += np.where(ok, z[np.clip(i, 0, len(z) - 1)] * kaiser_sinc(t, c, half), 0.0)
    return out


def shift_channel(x: np.ndarray, semitones, n_fft: int = 4096, positions=None) -> np.ndarray:
    r = ratio(semitones)
    z = stretch(np.asarray(x), r, n_fft)
    return resample_at(z, r, np.arange(len(x)) if positions is None else positions)


def shift(x: np.ndarray, semitones, n_fft: int = 4096) -> np.ndarray:
    """float32 [C, N] -> float64 [C, N] (the kernels' result is this rounded once to float32)"""
    x = np.atleast_2d(x)
    return np.stack([shift_channel(ch, semitones, n_fft) for ch in x])
