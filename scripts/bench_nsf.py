#!/usr/bin/env python3
"""RVC's NSF-HiFiGAN vocoder (``audiolab_amd.nsf``) at the sizes a user runs: the v2 40k configuration with synthetic weights over one
pipeline segment of 4100 frames (41 s, the reference's ``x_max``) and over a 5-minute vocal cut into such segments.

Prints ``forward`` in total (device events around the call; warm-up first, then the median of ``--runs``) and per stage (device events
around each stage's call on the inputs the chain hands it): the source, ``conv_pre`` with the speaker conditioning, every upsampling
stage split into its transposed convolution and its resblocks (the stage's median minus the transposed convolution's median: a
difference of two event times, not a kernel time), ``conv_post``; the achieved TFLOP/s of the resblock convolutions against
the 155 TF exact-f32 MFMA figure.  Beside that the same generator as torch.nn.functional calls (tests/nsf_oracle.py) on the
same GPU (float32, folded weights), and on this host's CPU for one short segment (``--cpu-only``: that part alone).
``--kernels-only`` runs ``forward`` alone a few times: the run to put under ``rocprofv3 --kernel-trace --stats``.  Nothing here is asserted: the numbers are recorded."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from audiolab_amd import _lib, nsf  # noqa: E402
from tests import nsf_oracle as oracle  # noqa: E402

PEAK_TF = 155.0


def inputs(cfg, T, seed=0):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((1, cfg.initial_channel, T)).astype(np.float32)
    t = np.arange(T) / 100.0
    f0 = (220.0 * 2.0 ** (0.5 * np.sin(2 * np.pi * 0.1 * t) + 0.02 * np.sin(2 * np.pi * 5.5 * t))).astype(np.float32)
    f0[(t % 4.0) > 3.2] = 0.0                                                # a breath every four seconds
    g = rng.standard_normal((1, cfg.gin_channels, 1)).astype(np.float32)
    noise = rng.standard_normal(T * cfg.upp).astype(np.float32)
    return x, f0[None, :], g, noise


def timed(fn, warmup, runs):
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


def resblock_flops(cfg, i, L):
    c = cfg.stage_channels(i)
    return sum(2.0 * L * c * c * k * 6 for k in cfg.resblock_kernel_sizes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=4100)
    ap.add_argument("--seconds", type=float, default=300.0)
    ap.add_argument("--cpu-frames", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--no-baselines", action="store_true")
    ap.add_argument("--cpu-only", action="store_true", help="only the CPU baseline (needs no GPU)")
    args = ap.parse_args()
    if args.cpu_only:
        cfg = nsf.V2_40K
        x, f0, g, noise = inputs(cfg, args.cpu_frames, args.seed)
        har = torch.from_numpy(oracle.source(f0.reshape(-1), noise, cfg.upp, cfg.sr, 1.0, 0.0).astype(np.float32)).reshape(1, 1, -1)
        cpu_baseline(cfg, nsf.synthetic_state_dict(cfg, args.seed), args.cpu_frames, torch.from_numpy(x), har, torch.from_numpy(g))
        return
    if not torch.cuda.is_available():
        raise SystemExit("bench_nsf: needs a GPU (cuda:0)")
    ctx = _lib.Context("cuda:0")
    cfg = nsf.V2_40K
    sd = nsf.synthetic_state_dict(cfg, args.seed)
    voc = nsf.NSFVocoder(sd, cfg, ctx)
    T = args.frames
    x, f0, g, noise = inputs(cfg, T, args.seed)
    xd, fd, gd, nd = (torch.from_numpy(a).cuda() for a in (x, f0, g, noise))
    if args.kernels_only:
        for _ in range(3):
            out = voc.forward(xd, fd, gd, noise=nd)
        torch.cuda.synchronize()
        print(f"forward x 3 over {T} frames: {out.numel()} samples, rms {float(out.pow(2).mean().sqrt()):.3f}", flush=True)
        return
    print(f"NSF-HiFiGAN v2 40k, synthetic weights (seed {args.seed}), float32; one segment of {T} frames = {T / 100:g} s = {T * cfg.upp} samples; "
          f"{args.warmup} warm-up, median of {args.runs} runs (device events)", flush=True)
    ms_total, out = timed(lambda: voc.forward(xd, fd, gd, noise=nd), args.warmup, args.runs)
    flops_all = sum(resblock_flops(cfg, i, T * int(np.prod(cfg.upsample_rates[:i + 1]))) for i in range(len(cfg.upsample_rates)))
    print(f"forward: total {ms_total:.2f} ms = {T * 10.0 / ms_total:.0f}x real time; output rms {float(out.pow(2).mean().sqrt()):.3f}", flush=True)
    rows = []
    ms, har = timed(lambda: voc.source(fd, nd), args.warmup, args.runs)
    rows.append(("source", ms, ""))
    ms, h = timed(lambda: voc.pre(xd, gd), args.warmup, args.runs)
    rows.append(("conv_pre + cond", ms, ""))
    res_ms = 0.0
    for i, st in enumerate(voc.stages):
        hin = h
        ms_t, _ = timed(lambda: nsf.tconv1d(ctx, hin, st.w, st.b, har, st.nw, st.nb, st.u, st.s), args.warmup, args.runs)
        ms_s, h = timed(lambda: voc.stage(i, hin, har), args.warmup, args.runs)
        L, c = int(h.shape[0]), int(h.shape[1])
        fl = resblock_flops(cfg, i, L)
        res_ms += ms_s - ms_t
        rows.append((f"stage {i}: tconv -> [{L}, {c}]", ms_t, ""))
        rows.append((f"stage {i}: {len(st.blocks)} resblocks (stage - tconv)", ms_s - ms_t,
                     f"  {fl / 1e9:8.1f} GFLOP = {fl / (ms_s - ms_t) / 1e9:6.1f} TFLOP/s = {100 * fl / (ms_s - ms_t) / 1e9 / PEAK_TF:4.1f} % of {PEAK_TF:g}"))
    ms, _ = timed(lambda: voc.post(h), args.warmup, args.runs)
    rows.append(("conv_post", ms, ""))
    for name, ms, extra in rows:
        print(f"   {name:36s} {ms:10.3f} ms{extra}", flush=True)
    print(f"   {'sum of the stages':36s} {sum(r[1] for r in rows):10.3f} ms", flush=True)
    print(f"resblock convolutions: {flops_all / 1e12:.2f} TFLOP in {res_ms:.2f} ms = {flops_all / res_ms / 1e9:.1f} TFLOP/s "
          f"({100 * flops_all / res_ms / 1e9 / PEAK_TF:.1f} % of the {PEAK_TF:g} TF exact-f32 MFMA figure; the floor at that figure is "
          f"{flops_all / PEAK_TF / 1e9:.2f} ms)", flush=True)

    # a 5-minute vocal in segments of `frames`
    total_frames = int(args.seconds * 100)
    segs = [T] * (total_frames // T) + ([total_frames % T] if total_frames % T else [])
    seg_in = {n: tuple(torch.from_numpy(a).cuda() for a in inputs(cfg, n, args.seed)) for n in set(segs)}

    def vocal():
        last = None
        for n in segs:
            a, b, c, d = seg_in[n]
            last = voc.forward(a, b, c, noise=d)
        return last
    ms_vocal, _ = timed(vocal, 1, 3)
    print(f"{args.seconds:g} s vocal in {len(segs)} segments ({segs[0]} frames, the last {segs[-1]}): {ms_vocal:.1f} ms = "
          f"{args.seconds * 1e3 / ms_vocal:.0f}x real time (median of 3)", flush=True)
    if args.no_baselines:
        return

    w_gpu = oracle.weights(sd, torch.float32, "cuda")
    hard = har.reshape(1, 1, -1)
    with torch.no_grad():
        ms_torch, want = timed(lambda: oracle.generator_torch(w_gpu, cfg, xd, hard, gd), 1, 3)
    print(f"the same generator as torch.nn.functional calls (tests/nsf_oracle.py) on this GPU (float32, conv_pre .. tanh, the source excluded): "
          f"{ms_torch:.1f} ms (this project's forward without the source: {ms_total - rows[0][1]:.1f} ms); max |out delta| between the two "
          f"{float((want.reshape(-1) - out.reshape(-1)).abs().max()):.2e}", flush=True)
    del w_gpu
    cpu_baseline(cfg, sd, args.cpu_frames, xd.cpu(), hard.cpu(), gd.cpu(), want.reshape(-1).cpu())


def cpu_baseline(cfg, sd, Tc, x, har, g, gpu_out=None):
    """the same calls on the host's CPU over the first ``Tc`` frames: one warm-up, then three timed runs by the host clock"""
    w_cpu = oracle.weights(sd, torch.float32, "cpu")
    torch.set_num_threads(min(16, torch.get_num_threads()))
    xc, hc = x[:, :, :Tc].contiguous(), har[:, :, :Tc * cfg.upp].contiguous()
    flops = sum(resblock_flops(cfg, i, Tc * int(np.prod(cfg.upsample_rates[:i + 1]))) for i in range(len(cfg.upsample_rates)))
    with torch.no_grad():
        got = oracle.generator_torch(w_cpu, cfg, xc, hc, g)
        secs = []
        for _ in range(3):
            t0 = time.perf_counter()
            got = oracle.generator_torch(w_cpu, cfg, xc, hc, g)
            float(got.sum())                                                 # the result is read: nothing is left pending
            secs.append(time.perf_counter() - t0)
    cpu_s = statistics.median(secs)
    extra = ""
    if gpu_out is not None:                                                  # away from the cut at frame Tc the two segments agree
        n = (Tc // 2) * cfg.upp
        extra = f"; max |out delta| to the GPU run over the first {Tc // 2} frames {float((got.reshape(-1)[:n] - gpu_out[:n]).abs().max()):.2e}"
    print(f"the same calls on this host's CPU ({torch.get_num_threads()} threads, {os.cpu_count()} logical CPUs on the host) over {Tc} frames = "
          f"{Tc / 100:g} s, {got.numel()} samples out: {cpu_s:.3f} s (median of 3: {', '.join(f'{v:.3f}' for v in secs)}) = "
          f"{Tc / 100 / cpu_s:.2f}x real time = {flops / cpu_s / 1e9:.0f} GFLOP/s in the resblock convolutions{extra}", flush=True)


if __name__ == "__main__":
    main()
