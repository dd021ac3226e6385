"""The specification of audiolab_amd.compare in numpy / scipy float64, written from the description of the Compare plugin's figure: what each
of its four panels shows.  ``scipy.signal.resample`` and ``scipy.signal.stft`` are called themselves, so the GPU chain is pinned against the
libraries the plugin runs on, not against a restatement of them.

A track is ``(interleaved samples, frame_rate)``; the interleaved sequence is one signal (a stereo file counts as a mono signal of twice the
length -- the plugin's behaviour)."""
import numpy as np
from scipy.signal import resample, stft

RATE = 44100
N_SEG, OVERLAP = 2048, 1024


def common_rate(samples: np.ndarray, frame_rate: int) -> np.ndarray:
    """the track at 44.1 kHz: the Fourier-method resampler on ``int(n * 44100 / frame_rate)`` points"""
    x = np.asarray(samples, dtype=np.float64)
    return resample(x, int(len(x) * RATE / frame_rate))


def compare(a, b) -> dict:
    tracks = [common_rate(*a), common_rate(*b)]
    n = min(len(w) for w in tracks)
    tracks = [w[:n].copy() for w in tracks]
    for w in tracks:                                                         # unit RMS, unless the track is (all but) silent
        level = np.sqrt(np.mean(w ** 2))
        if level > 1e-9:
            w /= level
    diff = np.abs(tracks[0] - tracks[1])
    f, t, z1 = stft(tracks[0], fs=RATE, nperseg=N_SEG, noverlap=OVERLAP)
    _, _, z2 = stft(tracks[1], fs=RATE, nperseg=N_SEG, noverlap=OVERLAP)
    s1, s2 = np.abs(z1), np.abs(z2)
    sd = np.abs(s1 - s2)
    out = {"waveforms": tracks, "differences": diff, "f": f, "t": t, "spec1": s1, "spec_diff": sd,
           "spec1_db": 20.0 * np.log10(s1 + 1e-9), "diff_db": 20.0 * np.log10(sd + 1e-9)}
    for v in (tracks[0], tracks[1], diff, s1, sd, out["spec1_db"], out["diff_db"]):
        v.setflags(write=False)
    return out
