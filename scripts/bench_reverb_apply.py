#!/usr/bin/env python3
"""Convolution reverb (``audiolab_amd.reverb.apply_reverb_array`` -> ``alsep_reverb_apply``) at the size a user runs: a 5-minute stereo
track at 44.1 kHz against the 2 s impulse response ``extract_reverb`` stores (88 200 taps).

Prints: ms per call (device events around a window of at least a second of repeated calls, after a warm-up), the bytes the passes move
computed from the shapes, that traffic over the time as a share of the 6.3 TB/s copy rate of the MI355X, a spot check against long-double
dot products, and -- labelled as a CPU baseline -- the reference's method on this host: scipy ``fftconvolve`` per channel in float64,
pad, gain, clip.  Kernel statistics come from a separate run under ``rocprofv3 --kernel-trace --stats`` (``--no-cpu-baseline --window 0.2``)."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from audiolab_amd import _lib, reverb  # noqa: E402

COPY_RATE = 6.3e12


def pass_bytes(n: int, channels: int, taps: int, pre: int, k: int) -> dict:
    """bytes each stage reads + writes for one call, from the shapes: blocks of F = 2^k complex doubles (16 B), S = F - L + 1 new
    samples per block, one set of blocks per channel pair"""
    F, pairs = 1 << k, (channels + 1) // 2
    S = F - taps + 1
    blocks = -(-(n - min(pre, n)) // S) * pairs
    passes = -(-k // 3)
    return {
        "ir_spectrum": 8 * taps + 16 * F + passes * 32 * F,
        "gather": blocks * (8 * F + 16 * F),                                 # two float32 channels in, one complex block out
        "forward_passes": blocks * passes * 32 * F,
        "product": blocks * 32 * F + 16 * F,
        "inverse_passes": blocks * passes * 32 * F,
        "finish": blocks * S * (16 + 8 + 8),                                 # the block's kept outputs, the dry pair in, the result out
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=300.0)
    ap.add_argument("--sr", type=int, default=44100)
    ap.add_argument("--taps", type=int, default=88200)
    ap.add_argument("--pre-delay", type=float, default=0.02)
    ap.add_argument("--window", type=float, default=1.0, help="timed window in seconds (at least)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_reverb_apply: needs a GPU (cuda:0)")
    ctx = _lib.Context("cuda:0")
    n, sr, taps = int(args.seconds * args.sr), args.sr, args.taps
    pre = int(args.pre_delay * sr)
    rng = np.random.default_rng(0)
    dry = (0.2 * rng.standard_normal((2, n)) * np.exp(-((np.arange(n) / sr * 2.0) % 1.0) * 3.0)).astype(np.float32)
    ir = rng.standard_normal(taps) * np.exp(-np.arange(taps) / (taps / 6.9))
    ir[0] = 1.0
    ir /= np.sqrt(np.sum(ir ** 2))
    dry_d, ir_d = torch.from_numpy(dry).cuda(), torch.from_numpy(ir).cuda()
    k = int(ctx.lib.alsep_reverb_apply_block_log2(taps, 0))
    stages = pass_bytes(n, 2, taps, pre, k)
    total = sum(stages.values())
    print(f"track {args.seconds:.0f} s x 2 channels at {sr} Hz ({n} samples), impulse response {taps} taps, pre-delay {pre} samples; "
          f"blocks of 2^{k} points, {-(-(n - pre) // ((1 << k) - taps + 1))} per channel pair")
    print("bytes moved per call (from the shapes): " + ", ".join(f"{name} {b / 1e9:.3f} GB" for name, b in stages.items()) + f"; total {total / 1e9:.3f} GB")

    out = None
    for _ in range(3):                                                       # warm-up: code objects, the allocator's workspace block
        out = reverb.apply_reverb_array(dry_d, ir_d, pre, ctx=ctx)
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    calls, t0 = 0, time.perf_counter()
    start.record()
    while True:
        out = reverb.apply_reverb_array(dry_d, ir_d, pre, ctx=ctx)
        calls += 1
        if calls % 4 == 0:
            torch.cuda.synchronize()
            if time.perf_counter() - t0 >= args.window:
                break
    stop.record()
    torch.cuda.synchronize()
    ms = start.elapsed_time(stop) / calls
    rate = total / (ms * 1e-3)
    print(f"GPU: {ms:.2f} ms per call over {calls} calls ({start.elapsed_time(stop) / 1e3:.2f} s window, device events; the call includes "
          f"its own workspace allocation): {rate / 1e12:.2f} TB/s of computed traffic = {100 * rate / COPY_RATE:.0f} % of the 6.3 TB/s copy rate; "
          f"{args.seconds / (ms * 1e-3):.0f} x realtime")

    pos = np.sort(np.concatenate([[0, pre, n - 1], rng.integers(0, n, 29)]))
    got = out[:, torch.from_numpy(pos).cuda()].cpu().numpy().astype(np.float64)
    x, h = dry.astype(np.longdouble), ir.astype(np.longdouble)[::-1]
    want = np.zeros((2, len(pos)))
    for i, o in enumerate(pos):
        t = int(o) - pre
        m = min(t + 1, taps) if t >= 0 else 0
        wet = x[:, t - m + 1: t + 1] @ h[taps - m:] if m else np.zeros(2, dtype=np.longdouble)
        want[:, i] = np.clip(x[:, o] + np.longdouble(0.7) * wet, -1.0, 1.0).astype(np.float64)
    print(f"spot check: max|ours - exact| at {len(pos)} positions per channel = {np.max(np.abs(got - want)):.3e} (2^-24 = {2.0 ** -24:.3e})")

    if not args.no_cpu_baseline:
        from scipy.signal import fftconvolve
        d64 = dry.astype(np.float64)
        t0 = time.perf_counter()
        wet = np.stack([np.pad(fftconvolve(d64[c], ir, mode="full"), (pre, 0))[:n] for c in range(2)])
        final = np.clip(d64 + 0.7 * wet, -1.0, 1.0)
        cpu_s = time.perf_counter() - t0
        print(f"CPU baseline (the reference's method on this host: scipy fftconvolve per channel in float64, pad, gain, clip): {cpu_s * 1e3:.0f} ms "
              f"= {cpu_s * 1e3 / ms:.0f} x the GPU call; max|ours - it| = {np.max(np.abs(out.cpu().numpy() - final)):.3e}")


if __name__ == "__main__":
    main()
