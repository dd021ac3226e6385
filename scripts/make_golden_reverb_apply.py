#!/usr/bin/env python3
"""Generate tests/golden/reverb_apply.npz by RUNNING THE REFERENCE's ``apply_reverb`` (handlers/reverb.py:179-209).

    python scripts/make_golden_reverb_apply.py --reference <AudioLab checkout>      (or AUDIOLAB_REFERENCE=<checkout>)

The reference never travels: only the reference's OUTPUTS on the seeded cases of tests/reverb_apply_cases.py are stored.  Third-party
imports the function does not need are stubbed (pydub, soundfile, audio_separator) as oracle/make_golden_reverb.py does; ``read_audio``
and ``load_params_from_file`` are replaced to hand over the case, ``sf.write`` to capture ``final_signal``; everything between them is
the reference's code (scipy's ``fftconvolve``, ``np.pad``, the 0.7 gain, ``np.clip``).

Per case (at tests.reverb_apply_cases.positions: the whole signal, or the first 4096 samples + 4096 seeded positions for "ir_longer"):
  <name>_ref      the reference's float64 ``final_signal``, [positions, C] or [positions]
  <name>_exact_q  int16: (exact - reference) in units of 2^-36, exact = the same formula with the convolution as long-double dot
                  products.  The reference transforms the float32 dry signal in single precision, so it sits 3e-8 .. 2e-7 from the
                  exact value; that distance fits 16 bits at a step of 2^-36 = 1.5e-11 (rounding <= 7.3e-12, four orders below the
                  2^-24 the tests allow), which keeps the file under 1 MB where two float64 copies would not be.
  <name>_ref_err  max|reference - exact| before that rounding
  <name>_pre      the pre-delay in samples the reference derived, int(pre_delay * sr) (:187)
"""
from __future__ import annotations

import argparse
import importlib.util
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "reverb_apply.npz")
sys.path.insert(0, ROOT)

from tests.reverb_apply_cases import CASES, exact_final, make_case, positions  # noqa: E402

Q_STEP = 2.0 ** -36


def _stub(name: str, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    m.__path__ = []
    sys.modules[name] = m
    return m


def load_ref_reverb(ref_root: str):
    class _Dummy:
        def __init__(self, *a, **k):
            pass
    _stub("soundfile")
    _stub("audio_separator")
    _stub("audio_separator.separator", Separator=_Dummy)
    _stub("pydub", AudioSegment=_Dummy)
    _stub("handlers")
    _stub("handlers.config", output_path=".")
    spec = importlib.util.spec_from_file_location("ref_reverb", os.path.join(ref_root, "handlers", "reverb.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("AUDIOLAB_REFERENCE"), help="root of the AudioLab checkout")
    args = ap.parse_args()
    if not args.reference:
        ap.error("pass --reference or set AUDIOLAB_REFERENCE")
    ref = load_ref_reverb(args.reference)
    out = {}
    for name in CASES:
        dry, ir, pre_delay, sr = make_case(name)
        captured = {}
        ref.read_audio = lambda path: (dry.copy(), sr)
        ref.load_params_from_file = lambda path: {"sample_rate": sr, "pre_delay": pre_delay, "impulse_response": ir.tolist()}
        ref.sf.write = lambda path, data, rate: captured.update(final=np.array(data), sr=rate)
        assert ref.apply_reverb("dry", "params", "out.wav") == "out.wav"
        final = captured["final"]
        assert final.dtype == np.float64 and final.shape == dry.shape and captured["sr"] == sr
        pre = int(pre_delay * sr)
        pos = positions(name)
        got = final[pos]
        exact = exact_final(dry, ir, pre, pos)
        diff = exact - got
        ref_err = float(np.max(np.abs(diff)))
        q = np.rint(diff / Q_STEP)
        assert np.max(np.abs(q)) < 32768, "the reference is further from the exact value than int16 steps of 2^-36 hold"
        out[f"{name}_ref"] = got
        out[f"{name}_exact_q"] = q.astype(np.int16)
        out[f"{name}_ref_err"] = np.array([ref_err])
        out[f"{name}_pre"] = np.array([pre])
        clipped = float(np.mean(np.abs(got) >= 1.0))
        print(f"{name}: {got.shape} pre {pre} ref_err {ref_err:.3e} clipped {clipped:.3%}")
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
