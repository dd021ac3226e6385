#!/usr/bin/env python3
"""RMVPE pitch extraction (``audiolab_amd.rmvpe``) at the size a user runs: 5 minutes of mono at 16 kHz (30 001 frames), synthetic weights.

Prints ``infer_from_audio`` from device-resident samples in total (a host clock around the call, which ends in a device-to-host copy;
warm-up first, then the median of ``--runs``) and per stage (device events around each stage's call on the inputs the chain hands it): the
log-mel front end, the U-Net (frame padding to the last convolution), the GRU's input GEMM, the GRU recurrence (also per step), the Linear +
sigmoid, the decode.  Beside that the torch restatement of tests/rmvpe_oracle.py on the same GPU, and on this host's CPU over
``--cpu-seconds`` of the same track (the full length takes minutes there).  ``--kernels-only`` runs ``infer_from_audio`` alone a few times:
the run to put under ``rocprofv3 --kernel-trace --stats``.  Nothing here is asserted: the numbers are recorded."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from audiolab_amd import _lib, rmvpe  # noqa: E402


def track(n: int, seed: int = 0) -> np.ndarray:
    """a voice-like tone gliding around 220 Hz with vibrato, a few harmonics and noise, float32"""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64) / rmvpe.SAMPLE_RATE
    f = 220.0 * 2.0 ** (0.5 * np.sin(2 * np.pi * 0.1 * t) + 0.02 * np.sin(2 * np.pi * 5.5 * t))
    phase = 2 * np.pi * np.cumsum(f) / rmvpe.SAMPLE_RATE
    x = sum(np.sin(k * phase) / k for k in (1, 2, 3, 4)) * 0.2 + 0.02 * rng.standard_normal(n)
    return x.astype(np.float32)


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
    ap.add_argument("--cpu-seconds", type=float, default=20.0)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--no-baselines", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_rmvpe: needs a GPU (cuda:0)")
    ctx = _lib.Context("cuda:0")
    n = int(args.seconds * rmvpe.SAMPLE_RATE)
    audio = track(n, 0)
    xd = torch.from_numpy(audio).cuda()
    model = rmvpe.RMVPE(None, ctx=ctx, allow_synthetic=True, seed=args.seed)
    net = model.model
    if args.kernels_only:
        for _ in range(3):
            f0 = model.infer_from_audio(xd)
        print(f"infer_from_audio x 3 over {n} samples: {len(f0)} frames, {int(np.count_nonzero(f0))} voiced", flush=True)
        return
    T = rmvpe.frames_of(n)
    Tp = T + rmvpe.pad_frames_of(T)
    print(f"RMVPE over {args.seconds:g} s of mono at {rmvpe.SAMPLE_RATE} Hz: {n} samples, {T} frames padded to {Tp}; E2E(4, 1, (2, 2)) with synthetic "
          f"weights (seed {args.seed}), float32; {args.warmup} warm-up, median of {args.runs} runs", flush=True)
    for _ in range(args.warmup):
        f0 = model.infer_from_audio(xd)
    torch.cuda.synchronize()
    totals = []
    for _ in range(args.runs):
        t0 = time.perf_counter()
        f0 = model.infer_from_audio(xd)
        torch.cuda.synchronize()
        totals.append((time.perf_counter() - t0) * 1e3)
    total = statistics.median(totals)
    print(f"infer_from_audio: total {total:.1f} ms (host clock, synchronised) = {args.seconds * 1e3 / total:.0f}x real time; "
          f"{int(np.count_nonzero(f0))} of {len(f0)} frames voiced, median f0 {float(np.median(f0[f0 > 0])) if np.any(f0 > 0) else 0.0:.1f} Hz", flush=True)

    logmel = rmvpe.mel_frontend(ctx, xd)

    def unet():
        x = rmvpe.pad_frames(ctx, logmel, Tp, net.in_scale, net.in_shift).view(1, Tp, rmvpe.N_MELS, 1)
        return net.unet(x)

    ms_mel, _ = timed(lambda: rmvpe.mel_frontend(ctx, xd), args.warmup, args.runs)
    ms_unet, y = timed(unet, args.warmup, args.runs)
    feat = y.view(Tp, 3 * rmvpe.N_MELS)
    ms_pre, pre = timed(lambda: net._gemm(feat, Tp, net.wih, net.bih), args.warmup, args.runs)
    pre3 = pre.view(Tp, 1, 6 * rmvpe.GRU_HIDDEN)
    ms_gru, h = timed(lambda: rmvpe.gru(ctx, pre3, net.whh_t, net.bhh), args.warmup, args.runs)

    def linear():
        sal = net._gemm(h, T, net.wfc, net.bfc)
        ctx.check(ctx.lib.alsep_rmvpe_sigmoid(ctx.handle, _lib.ptr(sal), sal.numel()), "alsep_rmvpe_sigmoid")
        return sal

    ms_lin, sal = timed(linear, args.warmup, args.runs)
    ms_dec, _ = timed(lambda: rmvpe.decode_salience(ctx, sal, 0.03), args.warmup, args.runs)
    rows = (("log-mel front end", ms_mel, ""), ("U-Net (padding .. last conv)", ms_unet, ""), ("GRU input GEMM", ms_pre, ""),
            ("GRU recurrence", ms_gru, f" = {ms_gru * 1e3 / Tp:.2f} us per step ({Tp} steps, both directions side by side)"),
            ("Linear + sigmoid", ms_lin, ""), ("decode", ms_dec, ""))
    for name, ms, extra in rows:
        print(f"   {name:30s} {ms:10.3f} ms{extra}", flush=True)
    print(f"   {'sum of the stages':30s} {sum(r[1] for r in rows):10.3f} ms", flush=True)
    if args.no_baselines:
        return

    from tests import rmvpe_oracle as o
    sd = rmvpe.synthetic_state_dict(o.FULL, args.seed)
    lm = logmel.t().cpu().numpy()
    sd_gpu = {k: v.cuda() for k, v in sd.items()}
    want = o.network(sd_gpu, o.FULL, lm, device="cuda")
    torch.cuda.synchronize()
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        want = o.network(sd_gpu, o.FULL, lm, device="cuda")
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    got = sal.cpu().numpy()
    print(f"torch restatement of the network (tests/rmvpe_oracle.py) on this GPU, log-mel to salience: {statistics.median(ts):.1f} ms "
          f"(this project's stages U-Net .. sigmoid: {ms_unet + ms_pre + ms_gru + ms_lin:.1f} ms); max |salience delta| between the two "
          f"{float(np.max(np.abs(got - want))):.2e}", flush=True)
    del sd_gpu, want
    nc = int(args.cpu_seconds * rmvpe.SAMPLE_RATE)
    torch.set_num_threads(min(16, torch.get_num_threads()))
    t0 = time.perf_counter()
    lm_c = o.log_mel(audio[:nc])
    f0_c = o.decode(o.network(sd, o.FULL, lm_c), 0.03)
    cpu_s = time.perf_counter() - t0
    print(f"the same restatement on this host's CPU ({torch.get_num_threads()} threads), audio to f0, over the first {args.cpu_seconds:g} s "
          f"({len(f0_c)} frames): {cpu_s:.2f} s = {args.cpu_seconds / cpu_s:.1f}x real time", flush=True)


if __name__ == "__main__":
    main()
