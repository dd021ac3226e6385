#!/usr/bin/env python3
"""The Remaster chain (``audiolab_amd.master.remaster_arrays`` / ``remaster_file``) at the size a user runs: a 5-minute stereo target and a
5-minute stereo reference at 44.1 kHz, seeded.

Prints: ``remaster_arrays`` from device-resident samples (device events around the whole call: warm-up first, then ``--runs`` repetitions
with their spread); the share of the host-side FIR design in it (wall clock around ``matching_fir``); ``remaster_file``, file to file; the
scipy restatement (tests/remaster_oracle.py) on this host's CPU; and ASSERTS that the GPU result and the oracle's agree within the
end-to-end bound of tests/test_remaster.py, after checking on the oracle that the loudest-piece masks are decided with room.

``--once`` runs one warmed-up call and nothing else: the per-kernel table comes from a profiler run of its own,
``rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/bench_remaster.py --once``."""
import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from audiolab_amd import _lib, master, wavio  # noqa: E402


def song(frames: int, seed: int, gain: float, hits: float) -> np.ndarray:
    """[frames, 2] float64: noise and two tones under a slow loudness curve (verse / chorus), plus a decaying 2 Hz pulse train of
    height ``hits`` that sets the crest factor"""
    rng = np.random.default_rng(seed)
    t = np.arange(frames) / 44100.0
    loud = 0.55 + 0.45 * np.sign(np.sin(2 * np.pi * t / 47.0 + seed)) * (0.6 + 0.4 * np.sin(2 * np.pi * t / 13.0))
    env = np.exp(-((t * 2.0) % 1.0) * 12.0)
    rows = []
    for c in range(2):
        x = 0.08 * rng.standard_normal(frames) + 0.25 * np.sin(2 * np.pi * 220.0 * t + c) + 0.15 * np.sin(2 * np.pi * 3613.7 * t + 0.5 * c)
        rows.append(gain * (loud * x + hits * env * np.sin(2 * np.pi * 90.0 * t + 0.3 * c)))
    return np.stack(rows, axis=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=300.0)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--once", action="store_true", help="one warmed-up call, for a profiler run")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_remaster: needs a GPU (cuda:0)")
    ctx = _lib.Context("cuda:0")
    cfg = master.MasterConfig()
    n = int(args.seconds * 44100)
    target, reference = song(n, 0, 0.5, 2.5), song(n, 1, 0.7, 0.05)          # the target's crest factor is the higher: the limiter has work
    dt, dr = torch.from_numpy(target).cuda(), torch.from_numpy(reference).cuda()

    def call():
        return master.remaster_arrays((dt, 44100), (dr, 44100), cfg, ctx=ctx)

    for _ in range(max(args.warmup, 1)):
        res = call()
    torch.cuda.synchronize()
    if args.once:
        call()
        torch.cuda.synchronize()
        return
    print(f"Remaster of a stereo target against a stereo reference, {args.seconds:g} s each at 44.1 kHz ({n} samples); {args.warmup} warm-up, "
          f"{args.runs} runs", flush=True)
    host_s = []
    design = master.matching_fir

    def timed_design(*a, **k):
        t0 = time.perf_counter()
        out = design(*a, **k)
        host_s[-1] += time.perf_counter() - t0
        return out
    master.matching_fir = timed_design
    totals = []
    for _ in range(args.runs):
        host_s.append(0.0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        res = call()
        e1.record()
        torch.cuda.synchronize()
        totals.append(e0.elapsed_time(e1))
    master.matching_fir = design
    med, fir = statistics.median(totals), 1e3 * statistics.median(host_s)
    print(f"remaster_arrays: median {med:.1f} ms (min {min(totals):.1f}, max {max(totals):.1f}); the host's FIR design (two channels: "
          f"interpolation, LOWESS, interpolation, irfft) {fir:.1f} ms of it = {100.0 * fir / med:.0f} %; limiter ran: {res.limited}; "
          f"k0 {res.k0:.4f}, corrections {', '.join(f'{c:.4f}' for c in res.coefficients)}", flush=True)
    with tempfile.TemporaryDirectory() as tmp:
        pt, pr, po = (os.path.join(tmp, f) for f in ("target.wav", "reference.wav", "out.wav"))
        wavio.write_wav(pt, np.clip(target.T, -1.0, 1.0), 44100, subtype="PCM_16")
        wavio.write_wav(pr, np.clip(reference.T, -1.0, 1.0), 44100, subtype="PCM_16")
        t0 = time.perf_counter()
        master.remaster_file(pt, pr, po, cfg, ctx=ctx)
        torch.cuda.synchronize()
        print(f"remaster_file, 16-bit WAV to 24-bit WAV: {time.perf_counter() - t0:.2f} s", flush=True)
    if not args.no_cpu_baseline:
        from tests import remaster_oracle as ro
        from tests.test_remaster import END_TO_END
        t0 = time.perf_counter()
        want = ro.remaster(target, reference, ro.Config())
        scipy_s = time.perf_counter() - t0
        margins = [float(np.min(np.abs(r - avg)) / avg) for r, avg in ((want["tgt_r"], want["tgt_avg"]), (want["ref_r"], want["ref_avg"]))]
        assert min(margins) > 1e-6, f"a piece's RMS lies within 1e-6 of the average ({margins}): the mask is not decided"
        got = res.result.cpu().numpy()
        err, peak = float(np.max(np.abs(got - want["result"].T))), float(np.max(np.abs(want["result"])))
        same = res.pcm24_bytes() == want["pcm24"]
        print(f"scipy restatement on this host's CPU: {scipy_s:.1f} s = {1e3 * scipy_s / med:.0f} times remaster_arrays; max|GPU - scipy| = {err:.3e} = "
              f"{err / peak:.3e} of the peak (bound {END_TO_END:.1e}); pieces nearest to the average by {min(margins):.1e}; "
              f"24-bit samples {'identical' if same else 'differ'}", flush=True)
        assert res.limited == want["ran"] and err <= END_TO_END * peak, "the GPU result and the oracle's differ by more than the end-to-end bound"


if __name__ == "__main__":
    main()
