#!/usr/bin/env python3
"""The pitch shifter (``audiolab_amd.pitch.shift_pitch_array`` -> ``alsep_pitch_shift``) at the size a user runs: one 5-minute stereo stem
at 44.1 kHz, n_fft 4096, at +2, -3, +12 and -12 semitones.

Prints, per shift: the frames and batches, the total per call (device events around the call: warm-up calls first, then the median of
``--runs`` timed calls) and the four stages -- analysis, recurrence, synthesis, resampling -- each from a profiled call of its own
(the library's event brackets, one category per call; median of ``--runs``).  The parent commit has nothing to compare with: the numbers
are recorded, no threshold is set.  The only baseline there is, labelled as such: the numpy oracle of tests/pitch_oracle.py on a 20 s
excerpt of one channel on this host, with a spot check of the GPU result against it."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from audiolab_amd import _lib, pitch  # noqa: E402

STAGES = (("analysis", _lib.PROF_PITCH_ANALYSIS), ("recurrence", _lib.PROF_PITCH_RECURRENCE), ("synthesis", _lib.PROF_PITCH_SYNTHESIS),
          ("resampling", _lib.PROF_PITCH_RESAMPLE))


def stem(n: int, sr: int) -> np.ndarray:
    rng = np.random.default_rng(0)
    t = np.arange(n) / sr
    env = np.exp(-((t * 2.0) % 1.0) * 3.0)
    x = 0.1 * rng.standard_normal((2, n)) + 0.3 * env * np.sin(2 * np.pi * 220.0 * t) + 0.2 * np.sin(2 * np.pi * 613.7 * t)
    return x.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=300.0)
    ap.add_argument("--sr", type=int, default=44100)
    ap.add_argument("--n-fft", type=int, default=4096)
    ap.add_argument("--shifts", type=int, nargs="+", default=[2, -3, 12, -12])
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pitch_shift: needs a GPU (cuda:0)")
    ctx = _lib.Context("cuda:0")
    n = int(args.seconds * args.sr)
    x = stem(n, args.sr)
    x_d = torch.from_numpy(x).cuda()
    print(f"pitch shift of a stereo stem of {args.seconds:g} s at {args.sr} Hz (2 x {n} samples), n_fft {args.n_fft}, default batch (1 GiB workspace); "
          f"{args.warmup} warm-up, median of {args.runs} runs")

    def call(s):
        return pitch.shift_pitch_array(x_d, s, n_fft=args.n_fft, ctx=ctx)

    for s in args.shifts:
        ratio = 2.0 ** (s / 12.0)
        frames = int(ctx.lib.alsep_pitch_shift_frames(n, args.n_fft, ratio))
        for _ in range(args.warmup):
            call(s)
        torch.cuda.synchronize()
        ctx.launch_counts_reset()
        call(s)
        torch.cuda.synchronize()
        batches = ctx.launch_count("pv_recurrence_kernel")
        totals = []
        for _ in range(args.runs):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out = call(s)
            b.record()
            torch.cuda.synchronize()
            totals.append(a.elapsed_time(b))
        line = [f"s {s:+3d} (ratio {ratio:.4f}): {frames} frames per channel in {batches} batches; total {statistics.median(totals):8.1f} ms"]
        for name, cat in STAGES:
            ms = []
            for _ in range(args.runs):
                ctx.profile_begin(cat)
                call(s)
                ms.append(ctx.profile_end()[0])
            line.append(f"{name} {statistics.median(ms):8.1f} ms")
        print("; ".join(line), flush=True)
        if not args.no_cpu_baseline and s == args.shifts[0]:
            from tests import pitch_oracle as po
            m = min(n, 20 * args.sr)
            t0 = time.perf_counter()
            z = po.stretch(x[0, :m], ratio, args.n_fft)
            pos = np.arange(0, m - 8 * args.n_fft, 997)                       # away from the excerpt's end, where the full stem goes on
            t1 = time.perf_counter()
            want = po.resample_at(z, ratio, pos)
            t2 = time.perf_counter()
            full = t1 - t0 + (t2 - t1) * m / len(pos)
            err = float(np.max(np.abs(out[0, torch.from_numpy(pos).cuda()].cpu().numpy().astype(np.float64) - want)))
            print(f"  CPU baseline (the numpy oracle, one channel, a {m / args.sr:g} s excerpt): vocoder {t1 - t0:.2f} s, resampler {t2 - t1:.2f} s for "
                  f"{len(pos)} of {m} samples (all of them: ~{full:.0f} s); max|GPU - oracle| at those samples {err:.2e}", flush=True)


if __name__ == "__main__":
    main()
