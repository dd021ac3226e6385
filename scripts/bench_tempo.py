#!/usr/bin/env python3
"""Tempo and beat tracking (``audiolab_amd.tempo``) at the size a user runs: a 5-minute stereo track at 44.1 kHz.

Prints ``beat_track_array`` from device-resident samples, in total (a host clock around the call, which ends in device-to-host copies; warm-up
first, then the median of ``--runs``) and per stage (device events around each stage's call on the inputs the chain hands it: warm-up, median
of ``--runs``), the sequential beat recursion also per frame; ``detect_bpm`` from the file to the result; and the numpy / scipy restatement
(tests/tempo_oracle.py) on this host's CPU with the same input, with the two results side by side.  Nothing here is asserted: the numbers
are recorded."""
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
from audiolab_amd import _lib, tempo, wavio  # noqa: E402


def song(frames: int, rate: int, bpm: float, seed: int) -> np.ndarray:
    """[2, frames] float32: noise, a decaying 1 kHz click on every beat and a steady tone; the right channel at half the level"""
    rng = np.random.default_rng(seed)
    t = np.arange(frames) / rate
    phase = (t * bpm / 60.0) % 1.0 * 60.0 / bpm
    x = 0.02 * rng.standard_normal(frames) + 0.5 * np.exp(-phase * 250.0) * np.sin(2 * np.pi * 1000.0 * phase) + 0.05 * np.sin(2 * np.pi * 220.0 * t)
    return np.stack([x, 0.5 * x]).astype(np.float32)


def timed(fn, warmup: int, runs: int):
    """-> (median milliseconds between device events around ``fn()``, its last result)"""
    for _ in range(warmup):
        out = fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=300.0)
    ap.add_argument("--bpm", type=float, default=128.0)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_tempo: needs a GPU (cuda:0)")
    ctx = _lib.Context("cuda:0")
    rate = 44100
    y = song(int(args.seconds * rate), rate, args.bpm, 0)
    yd = torch.from_numpy(y).cuda()
    print(f"Tempo of a stereo track of {args.seconds:g} s at {rate} Hz with a click at {args.bpm:g} bpm; {args.warmup} warm-up, median of {args.runs} runs",
          flush=True)

    def whole():
        return tempo.beat_track_array(yd, rate, ctx, want_stages=True)

    for _ in range(args.warmup):
        res = whole()
    torch.cuda.synchronize()
    totals = []
    for _ in range(args.runs):
        t0 = time.perf_counter()
        res = whole()
        torch.cuda.synchronize()
        totals.append((time.perf_counter() - t0) * 1e3)
    frames = int(res.stages["env"].shape[0])
    print(f"beat_track_array ({yd.shape[1]} samples per channel -> {res.stages['y'].shape[0]} at 22050 Hz, {frames} frames): "
          f"total {statistics.median(totals):.2f} ms (host clock, synchronised); bpm {res.bpm:.3f}, period {res.period}, {len(res.beat_frames)} beats",
          flush=True)
    st = res.stages
    stats = tempo.env_stats(ctx, st["env"])
    stages = (("mean of channels + resample", lambda: tempo.to_22050(ctx, yd, rate)),
              ("mel power", lambda: tempo.mel_power(ctx, st["y"])),
              ("flux", lambda: tempo.flux(ctx, st["mel"])),
              ("envelope statistics", lambda: tempo.env_stats(ctx, st["env"])),
              ("tempogram", lambda: tempo.tempogram_mean(ctx, st["env"])),
              ("local score", lambda: tempo.local_score(ctx, st["env"], res.period, stats)),
              ("beat recursion", lambda: tempo.beat_dp(ctx, st["ls"], res.period)))
    for name, fn in stages:
        ms, _ = timed(fn, args.warmup, args.runs)
        extra = f" = {ms * 1e3 / frames:.3f} us per frame ({2 * res.period - int(round(res.period / 2)) + 1} offsets)" if name == "beat recursion" else ""
        print(f"   {name:28s} {ms:9.3f} ms{extra}", flush=True)
    t0 = time.perf_counter()
    cum, back, ls = (st[k].cpu().numpy() for k in ("cum", "back", "ls"))
    tempo.tempo_scores(st["tg"].cpu().numpy())
    tempo.finish(cum, back, ls)
    print(f"   {'host: pick, finish, copies':28s} {(time.perf_counter() - t0) * 1e3:9.3f} ms", flush=True)

    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "song(Instrumental).wav")
        wavio.write_wav(path, y, rate, subtype="PCM_16")
        tempo.detect_bpm(path, ctx=ctx)
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            bpm, beats = tempo.detect_bpm(path, ctx=ctx)
            ts.append(time.perf_counter() - t0)
        print(f"detect_bpm, 16-bit file to result: {statistics.median(ts) * 1e3:.1f} ms (bpm {bpm:.3f}, {len(beats)} beats)", flush=True)

    if not args.no_cpu_baseline:
        from tests import tempo_oracle as o
        t0 = time.perf_counter()
        want = o.beat_track(y.astype(np.float64), rate)
        cpu_s = time.perf_counter() - t0
        same = np.array_equal(want["beats"], res.beat_frames)
        gpu_s = statistics.median(totals) / 1e3
        print(f"numpy / scipy restatement on this host's CPU: {cpu_s:.2f} s (bpm {want['bpm']:.3f}, {len(want['beats'])} beats; beat frames "
              f"{'identical to' if same else 'DIFFER from'} the GPU's); the GPU total is {'under' if gpu_s < cpu_s else 'NOT under'} it "
              f"({cpu_s / gpu_s:.1f}x)", flush=True)


if __name__ == "__main__":
    main()
