#!/usr/bin/env python3
"""Stem mixdown (``audiolab_amd.merge`` -> ``alsep_mix_sum`` / ``alsep_mix_power`` / ``alsep_mix_finish``) at the size a user runs: six float32
stems of a 5-minute stereo track at 44.1 kHz, mixed on the 32-bit grid and brought to the loudness of a source.

Prints, per pass: ms per launch (device events around a window of repeated launches, after a warm-up), the bytes the pass moves computed
from the shapes, and that traffic over the time as a share of the 6.3 TB/s copy rate of the MI355X; the whole ``mixdown_array`` call (its
three host read-backs included); the same with one sample more per row, where the second row of every stem starts off the 16-byte grid
and is read with scalar loads; and -- labelled as a CPU baseline -- the stdlib ``audioop`` calls pydub makes for the same mix on this host
(integer stems already in memory: five ``add``, ``max``, ``mul``, ``rms``, ``max``, ``mul``)."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from audiolab_amd import _lib, merge  # noqa: E402

COPY_RATE = 6.3e12


def timed(fn, window: float):
    """-> ms per call: device events around at least ``window`` seconds of calls"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    calls, t0 = 0, time.perf_counter()
    start.record()
    while True:
        fn()
        calls += 1
        if calls % 8 == 0:
            torch.cuda.synchronize()
            if time.perf_counter() - t0 >= window:
                break
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / calls, calls


def report(name: str, ms: float, calls: int, nbytes: float):
    rate = nbytes / (ms * 1e-3)
    print(f"  {name:34s} {ms:8.3f} ms over {calls:5d} calls, {nbytes / 1e9:6.3f} GB from the shapes: {rate / 1e12:5.2f} TB/s = "
          f"{100 * rate / COPY_RATE:3.0f} % of the copy rate")


def run(ctx, n: int, n_stems: int, window: float, label: str):
    rng = np.random.default_rng(0)
    stems = [torch.from_numpy((0.2 * rng.standard_normal((2, n))).astype(np.float32)).cuda() for _ in range(n_stems)]
    source = torch.from_numpy((0.1 * rng.standard_normal((2, n))).astype(np.float32)).cuda()
    widths, cells = [32] * n_stems, 2 * n
    print(f"{label}: {n_stems} float32 stems of 2 x {n} samples, 32-bit mix")
    acc, peak = merge.mix_sum(ctx, stems, widths, 32)
    f1 = merge.normalize_factor(peak, 32)
    ms, calls = timed(lambda: merge.mix_sum(ctx, stems, widths, 32, acc=acc), window)
    report("sum (one launch, peak read back)", ms, calls, 4.0 * cells * (n_stems + 1))
    ms, calls = timed(lambda: merge.mix_power(ctx, acc, 32, f1), window)
    report("power (two launches, read back)", ms, calls, 4.0 * cells)
    ms, calls = timed(lambda: merge.mix_finish(ctx, acc, 32, f1, 0.3), window)
    report("finish (integers)", ms, calls, 8.0 * cells)
    ms, calls = timed(lambda: merge.mix_finish(ctx, acc, 32, f1, 0.3, want_float=True), window)
    report("finish (integers and float32)", ms, calls, 12.0 * cells)
    target = merge.source_dbfs(source, ctx)
    ms, calls = timed(lambda: merge.mixdown_array(stems, target, ctx=ctx), window)
    report("mixdown_array, target given", ms, calls, 4.0 * cells * (n_stems + 1) + 4.0 * cells + 8.0 * cells)
    ms, calls = timed(lambda: merge.mixdown_array(stems, source, ctx=ctx), window)
    report("mixdown_array, source measured", ms, calls, 4.0 * cells * (n_stems + 1) + 4.0 * cells + 8.0 * cells + 12.0 * cells)
    return stems, source


def cpu_baseline(ctx, stems, source):
    import audioop
    out, rec = merge.mixdown_array(stems, source, ctx=ctx)
    ints = [np.clip(np.rint(s.cpu().numpy().astype(np.float64) * 2147483648.0), -2147483648.0, 2147483647.0).astype("<i4").tobytes() for s in stems]
    full = float(1 << 31)
    t0 = time.perf_counter()
    acc = ints[0]
    for seg in ints[1:]:
        acc = audioop.add(acc, seg, 4)
    peak = audioop.max(acc, 4)
    f1 = merge.db_to_float(merge.ratio_to_db(full * merge.db_to_float(-0.1) / peak))
    y1 = audioop.mul(acc, 4, f1)
    rms, peak1 = audioop.rms(y1, 4), audioop.max(y1, 4)
    _, _, f2 = merge.match_gain(rec.target_dBFS, rms, peak1, 32, True)
    y2 = audioop.mul(y1, 4, f2)
    cpu_s = time.perf_counter() - t0
    same = np.array_equal(np.frombuffer(y2, dtype="<i4").reshape(out.shape), out.cpu().numpy())
    print(f"CPU baseline (the audioop calls pydub makes, integer stems in memory): {cpu_s * 1e3:.0f} ms; peak {peak} / {rec.peak}, rms {rms} / {rec.rms}, "
          f"f2 {f2!r} / {rec.f2!r}; samples equal to the GPU's: {same}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=300.0)
    ap.add_argument("--sr", type=int, default=44100)
    ap.add_argument("--stems", type=int, default=6)
    ap.add_argument("--window", type=float, default=0.5, help="timed window per line in seconds (at least)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_merge: needs a GPU (cuda:0)")
    ctx = _lib.Context("cuda:0")
    n = int(args.seconds * args.sr) // 4 * 4
    stems, source = run(ctx, n, args.stems, args.window, "rows on the 16-byte grid")
    if not args.no_cpu_baseline:
        cpu_baseline(ctx, stems, source)
    del stems, source
    run(ctx, n + 1, args.stems, args.window, "second rows off the 16-byte grid")


if __name__ == "__main__":
    main()
