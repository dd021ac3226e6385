#!/usr/bin/env python3
"""The resampling sum pass (``audiolab_amd.merge.mix_sum_rates`` -> ``alsep_mix_sum_rates``) at the size a user runs: six float32 stems of a
5-minute stereo track mixed on the 32-bit grid, where one of them comes at another sample rate.

  case A   one 40 kHz stem among 44.1 kHz stems: the stem is resampled inside the one summing launch
  case B   the third stem at 48 kHz: two stems are summed, then the running mix is resampled once in a second launch, which also adds the
           48 kHz stem and resamples the three 44.1 kHz stems behind it

Prints, per launch: ms (device events around a window of repeated launches, after a warm-up), the bytes the launch moves computed from the
shapes (every operand read once, the mix written once), and that traffic over the time as a share of the 6.3 TB/s copy rate of the MI355X.
The yardstick is the equal-rate ``sum`` of scripts/bench_merge.py -- the unchanged ``mix_sum_kernel`` -- timed in the same process on the
same stem count and length.  Each case runs again with one sample more per row, where the second row of every operand starts off the
16-byte grid.  Where the host's Python has ``audioop`` (<= 3.12), the calls pydub makes for the same mix (``ratecv`` and ``add`` on integer
stems already in memory) are timed as a labelled CPU baseline and their result is compared with the GPU's, sample for sample."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from audiolab_amd import _lib, merge  # noqa: E402
from scripts.bench_merge import report, timed  # noqa: E402


def make_stems(seconds: float, rates, extra: int):
    rng = np.random.default_rng(0)
    return [torch.from_numpy((0.2 * rng.standard_normal((2, int(seconds * r) // 4 * 4 + extra))).astype(np.float32)).cuda() for r in rates]


def recorded_launches(ctx, stems, rates):
    """run ``mix_sum_rates`` once and keep the arguments of every launch it made (the buffers stay alive with them)"""
    calls, inner = [], merge._mix_sum_rates

    def record(*args):
        calls.append(args)
        return inner(*args)
    merge._mix_sum_rates = record
    try:
        acc, peak, rate = merge.mix_sum_rates(ctx, stems, [32] * len(stems), rates, 32)
    finally:
        merge._mix_sum_rates = inner
    return calls, acc, peak, rate


def launch_bytes(operands, channels: int, n_out: int) -> float:
    """every operand read once (a mono stem: one row), the mix written once"""
    return 4.0 * (sum(op.n * op.channels for op in operands) + channels * n_out)


def describe(operands) -> str:
    parts = []
    for op in operands:
        what = "mix" if op.is_mix else "stem"
        parts.append(f"{what} {op.in_rate}->{op.out_rate}" if op.in_rate != op.out_rate else what)
    return ", ".join(parts)


def run_case(ctx, label: str, seconds: float, rates, extra: int, window: float):
    stems = make_stems(seconds, rates, extra)
    print(f"{label}: rates {rates}, first stem 2 x {stems[0].shape[1]} samples, 32-bit mix")
    calls, acc, peak, rate = recorded_launches(ctx, stems, rates)
    for i, args in enumerate(calls):
        operands, channels, n_out = args[1], args[2], args[3]
        ms, count = timed(lambda: merge._mix_sum_rates(*args), window)
        print(f"  launch {i + 1}: {describe(operands)} -> 2 x {n_out}")
        report(f"launch {i + 1} (mix_sum_rate_kernel)", ms, count, launch_bytes(operands, channels, n_out))
    ms, count = timed(lambda: merge.mix_sum_rates(ctx, stems, [32] * len(stems), rates, 32), window)
    report("mix_sum_rates, peak read back", ms, count, sum(launch_bytes(a[1], a[2], a[3]) for a in calls))
    return stems, acc, peak, rate


def run_equal(ctx, seconds: float, rate: int, n_stems: int, extra: int, window: float):
    stems = make_stems(seconds, [rate] * n_stems, extra)
    n = stems[0].shape[1]
    print(f"equal rates, the yardstick: {n_stems} float32 stems of 2 x {n} samples at {rate} Hz, 32-bit mix")
    acc, _ = merge.mix_sum(ctx, stems, [32] * n_stems, 32)
    ms, count = timed(lambda: merge.mix_sum(ctx, stems, [32] * n_stems, 32, acc=acc), window)
    report("sum (mix_sum_kernel, peak read back)", ms, count, 4.0 * 2 * n * (n_stems + 1))


def cpu_baseline(label: str, stems, rates, acc, peak):
    try:
        import audioop
    except ImportError:
        print(f"  CPU baseline ({label}): this Python has no audioop")
        return
    ints = [np.ascontiguousarray(np.clip(np.rint(s.cpu().numpy().astype(np.float64) * 2147483648.0), -2147483648.0, 2147483647.0).astype("<i4").T)
            .tobytes() for s in stems]

    def fit(b, size):
        return b[:size] if len(b) >= size else b + bytes(size - len(b))
    t0 = time.perf_counter()
    mix, rate = ints[0], rates[0]
    for seg, r in zip(ints[1:], rates[1:]):
        if r > rate:
            mix, rate = audioop.ratecv(mix, 4, 2, rate, r, None)[0], r
        elif r < rate:
            seg = audioop.ratecv(seg, 4, 2, r, rate, None)[0]
        mix = audioop.add(mix, fit(seg, len(mix)), 4)
    cpu_peak = audioop.max(mix, 4)
    cpu_s = time.perf_counter() - t0
    same = np.array_equal(np.frombuffer(mix, dtype="<i4").reshape(-1, 2).T, acc.cpu().numpy())
    print(f"  CPU baseline ({label}; audioop.ratecv and the adds pydub makes, integer stems in memory): {cpu_s * 1e3:.0f} ms; peak {cpu_peak} / {peak}; "
          f"samples equal to the GPU's: {same}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=300.0)
    ap.add_argument("--window", type=float, default=0.5, help="timed window per line in seconds (at least)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_merge_rates: needs a GPU (cuda:0)")
    ctx = _lib.Context("cuda:0")
    case_a = [44100, 44100, 40000, 44100, 44100, 44100]
    case_b = [44100, 44100, 48000, 44100, 44100, 44100]
    for extra, rows in ((0, "rows on the 16-byte grid"), (1, "second rows off the 16-byte grid")):
        print(f"==== {rows}")
        run_equal(ctx, args.seconds, 44100, 6, extra, args.window)
        for label, rates in (("case A", case_a), ("case B", case_b)):
            stems, acc, peak, _ = run_case(ctx, label, args.seconds, rates, extra, args.window)
            if extra == 0 and not args.no_cpu_baseline:
                cpu_baseline(label, stems, rates, acc, peak)
            del stems, acc
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
