#!/usr/bin/env python
"""Writes tests/golden/merge.npz: the mixdown of every case of tests/merge_cases.py as the stdlib C module ``audioop`` computes it --
the module pydub calls for AudioSegment.overlay (``add``), .max (``max``), .rms / .dBFS (``rms``) and .apply_gain (``mul``), i.e. for
everything the reference's wrappers/merge.py:15-45,146-151 does to samples.  pydub's own control flow (overlay's cropping to the first
segment, normalize's headroom of 0.1 dB, the dBFS formula) is restated in tests/merge_cases.reference_mix from its published source;
only the ``audioop`` arithmetic is pinned here.  Needs Python <= 3.12 (``audioop`` leaves the standard library with 3.13).

Per case and width of the mix: acc and y2 (int16 / int32 [C, N]), peak, peak1, rms as integers, f1, f2 and the dB values as raw float64.
Asserted per case and per power computation: sqrt(S / count) lies at least 1e-3 from an integer, so that audioop's sequentially rounded
double sum and an exact integer sum truncate to the same rms.  Reseed a case that fails it."""
import audioop
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.merge_cases import CASES, NUMPY_OPS, VARIANTS, make_case, reference_mix  # noqa: E402


def _bytes(a, bits):
    return np.ascontiguousarray(a).astype("<i2" if bits == 16 else "<i4").tobytes()


def _array(b, bits, shape):
    return np.frombuffer(b, dtype="<i2" if bits == 16 else "<i4").astype(np.int64).reshape(shape)


AUDIOOP_OPS = dict(
    add=lambda a, b, bits: _array(audioop.add(_bytes(a, bits), _bytes(b, bits), bits // 8), bits, a.shape),
    mul=lambda a, f, bits: _array(audioop.mul(_bytes(a, bits), bits // 8, f), bits, a.shape),
    max=lambda a, bits: audioop.max(_bytes(a, bits), bits // 8),
    rms=lambda a, bits: audioop.rms(_bytes(a, bits), bits // 8),
)


def main():
    out = {}
    for name, bits in VARIANTS:
        stems, widths, source, source_width, prevent = make_case(name, bits)
        r = reference_mix(stems, widths, bits, source, source_width, prevent, AUDIOOP_OPS)
        assert min(r["margins"]) >= 1e-3, f"{name}/{bits}: sqrt(S / count) within {min(r['margins']):.2e} of an integer -- reseed the case"
        check = reference_mix(stems, widths, bits, source, source_width, prevent, NUMPY_OPS)
        assert all(np.array_equal(r[k], check[k]) for k in ("acc", "y2")) and all(r[k] == check[k] for k in ("peak", "peak1", "rms", "f1", "f2"))
        store = np.int16 if bits == 16 else np.int32
        key = f"{name}_{bits}"
        out[f"{key}_acc"], out[f"{key}_y2"] = r["acc"].astype(store), r["y2"].astype(store)
        out[f"{key}_ints"] = np.array([r["peak"], r["peak1"], r["rms"]], dtype=np.int64)
        out[f"{key}_floats"] = np.array([r["f1"], r["f2"], r["current_dBFS"], r["target_dBFS"], r["gain_dB"]], dtype=np.float64)
        full = 1 << (bits - 1)
        sat = (int(np.sum(r["acc"] == -full)), int(np.sum(r["acc"] == full - 1)))
        print(f"{key:24s} C,N={r['acc'].shape} peak={r['peak']} f1={r['f1']:.6f} rms={r['rms']} target={r['target_dBFS']:.3f} dB "
              f"gain={r['gain_dB']:.3f} dB f2={r['f2']:.6f} saturated(-/+)={sat} margin={min(r['margins']):.3f}")
    path = os.path.join(ROOT, "tests", "golden", "merge.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes, {len(CASES)} cases, {len(VARIANTS)} fixtures")


if __name__ == "__main__":
    main()
