#!/usr/bin/env python
"""Writes tests/golden/merge_rates.npz: what the stdlib C module ``audioop`` computes on the cases of tests/merge_rate_cases.py -- ``ratecv``
alone on every (rate pair, width, channel count, length), and the overlay chains of stems of differing sample rates with ``tostereo``,
``ratecv``, ``lin2lin`` and ``add`` in pydub's order, then ``max`` / ``mul`` / ``rms`` as in scripts/make_golden_merge.py.  pydub's own
control flow is restated in tests/merge_rate_cases.reference_mix_rates from its published source; only the ``audioop`` arithmetic is pinned
here.  Needs Python <= 3.12 (``audioop`` leaves the standard library with 3.13).

Asserted per case: the numpy restatements (``np_ratecv``, the numpy chain) equal the C module sample for sample, and sqrt(S / count) lies
at least 1e-3 from an integer wherever an rms is taken (the margin rule of make_golden_merge.py).  Reseed a case that fails it."""
import audioop
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.merge_cases import quantise  # noqa: E402
from tests.merge_rate_cases import (CHAIN_VARIANTS, CHANNELS, FULL_BELOW, LENGTHS, NUMPY_RATE_OPS, PAIRS, WIDTHS, digest, make_chain,  # noqa: E402
                                    np_ratecv, ratecv_input, ratecv_key, ratecv_length, reference_mix_rates)
from scripts.make_golden_merge import AUDIOOP_OPS, _array, _bytes  # noqa: E402


def _frames(a, bits):
    """[C, N] -> interleaved frames"""
    return _bytes(np.ascontiguousarray(a.T), bits)


def _rows(b, bits, channels):
    return np.ascontiguousarray(_array(b, bits, (-1, channels)).T)


def c_ratecv(a, width, in_rate, out_rate):
    return _rows(audioop.ratecv(_frames(a, width), width // 8, a.shape[0], in_rate, out_rate, None)[0], width, a.shape[0])


def c_lin2lin(a, width, new_width):
    return _rows(audioop.lin2lin(_frames(a, width), width // 8, new_width // 8), new_width, a.shape[0])


def c_tostereo(a, width):
    return _rows(audioop.tostereo(_frames(a, width), width // 8, 1, 1), width, 2)


AUDIOOP_RATE_OPS = dict(AUDIOOP_OPS, ratecv=c_ratecv, lin2lin=c_lin2lin, tostereo=c_tostereo)


def main():
    out = {}
    count = 0
    for pair in PAIRS:
        for width in WIDTHS:
            for channels in CHANNELS:
                for n in LENGTHS:
                    u = quantise(ratecv_input(pair, width, channels, n), width, width)
                    lo, hi = -(1 << (width - 1)), (1 << (width - 1)) - 1
                    if n >= 5:
                        assert any(u[0, i] == lo and u[0, i + 1] == hi for i in range(n - 1)), "the extremes are neighbours"
                    r = c_ratecv(u, width, *pair)
                    assert r.shape == (channels, ratecv_length(n, *pair)) and np.array_equal(r, np_ratecv(u, width, *pair)), (pair, width, channels, n)
                    key = ratecv_key(pair, width, channels, n)
                    if n <= FULL_BELOW:
                        out[key] = r.astype(np.int16 if width == 16 else np.int32)
                    else:
                        out[key + "_sha"], out[key + "_len"] = digest(r), np.int64(r.shape[1])
                    count += 1
    print(f"ratecv: {count} cases equal to the closed form")
    for name, bits in CHAIN_VARIANTS:
        stems, widths, rates, source = make_chain(name, bits)
        r = reference_mix_rates(stems, widths, rates, bits, source, True, AUDIOOP_RATE_OPS)
        assert min(r["margins"]) >= 1e-3, f"{name}/{bits}: sqrt(S / count) within {min(r['margins']):.2e} of an integer -- reseed the case"
        check = reference_mix_rates(stems, widths, rates, bits, source, True, NUMPY_RATE_OPS)
        assert all(np.array_equal(r[k], check[k]) for k in ("acc", "y2")) and all(r[k] == check[k] for k in ("rate", "peak", "peak1", "rms", "f1", "f2"))
        store = np.int16 if bits == 16 else np.int32
        key = f"chain_{name}_{bits}"
        out[f"{key}_acc"], out[f"{key}_y2"] = r["acc"].astype(store), r["y2"].astype(store)
        out[f"{key}_ints"] = np.array([r["peak"], r["peak1"], r["rms"], r["rate"]], dtype=np.int64)
        out[f"{key}_floats"] = np.array([r["f1"], r["f2"], r["current_dBFS"], r["target_dBFS"], r["gain_dB"]], dtype=np.float64)
        full = 1 << (bits - 1)
        sat = (int(np.sum(r["acc"] == -full)), int(np.sum(r["acc"] == full - 1)))
        print(f"{key:28s} C,N={r['acc'].shape} rate={r['rate']} peak={r['peak']} f1={r['f1']:.6f} rms={r['rms']} gain={r['gain_dB']:.3f} dB "
              f"f2={r['f2']:.6f} saturated(-/+)={sat} margin={min(r['margins']):.3f}")
    path = os.path.join(ROOT, "tests", "golden", "merge_rates.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
