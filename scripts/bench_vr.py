#!/usr/bin/env python3
"""Timing of the VR-architecture networks at a production window: n_fft 2048 (1024 bins), 768 frames (512 + 2 x 128 offset), random
weights -- nets_61968KB (``VRNet``) and nets_new with nout 48 (``VRNetNew``).  ``--precision both`` builds the float32 and the f16
network of each, warms each up and then alternates them in one process.  Prints ms per forward, the convolution TFLOP/s from the layer
shapes and its share of the matrix pipe's peak (float32 MFMA 157.3 TFLOP/s, f16 MFMA 2.5 PFLOP/s: whole-forward rates, not a kernel's).
``--track SECONDS`` adds a track of that length through the engine (woodwinds and denoise model, synthetic weights) per precision,
synchronised wall clock."""
import argparse
import os
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from audiolab_amd import _lib  # noqa: E402
from audiolab_amd.vrnet import WIDTHS, VRNet, VRNetNew, random_state_dict, random_state_dict_new  # noqa: E402

PEAK = {"f32": 157.3e12, "f16": 2.5e15}


def conv_flops(net, x):
    """2 x MACs of every convolution of one forward, from the shapes the network passes to its kernels"""
    flops = [0.0]
    conv, dec = net._conv, net._decoder

    def counted(L, x, y=None, c0=0, out_f32=False):
        ho, wo = L.out_hw(x.shape[1], x.shape[2])
        flops[0] += 2.0 * x.shape[0] * ho * wo * L.cout * L.cin * L.kh * L.kw
        return conv(L, x, y, c0, out_f32)

    def counted_dec(L, x, skip):
        if net.half and net.fuse_decoder:                       # the fused decoder does not go through _conv
            flops[0] += 2.0 * x.shape[0] * 4 * x.shape[1] * x.shape[2] * L.cout * L.cin * L.kh * L.kw
        return dec(L, x, skip)
    net._conv, net._decoder = counted, counted_dec
    net.forward_nhwc(x)
    torch.cuda.synchronize()
    net._conv, net._decoder = conv, dec
    return flops[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", choices=("f16", "f32", "both"), default="f32")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--track", type=float, default=0.0, help="seconds of audio through the engine per model and precision")
    args = ap.parse_args()
    precisions = ("f32", "f16") if args.precision == "both" else (args.precision,)
    n_fft, frames = 2048, 768
    ctx = _lib.Context("cuda:0")
    x = torch.rand((args.batch, n_fft // 2 + 1, frames, 2), device="cuda") * 3
    for label, make in (("VRNet nets_61968KB", lambda p: VRNet(n_fft, random_state_dict(WIDTHS["nets_61968KB"], seed=0), variant="nets_61968KB",
                                                                ctx=ctx, precision=p)),
                        ("VRNetNew nout 48", lambda p: VRNetNew(n_fft, random_state_dict_new(n_fft, 48, 128, seed=0), nout=48, nout_lstm=128,
                                                                ctx=ctx, precision=p))):
        nets = {p: make(p) for p in precisions}
        per = {p: conv_flops(nets[p], x) for p in precisions}                  # also the warm-up of every shape
        times = {p: [] for p in precisions}
        for _ in range(args.rounds):                                            # alternated: both see the same machine
            for p in precisions:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.reps):
                    y = nets[p].forward_nhwc(x)
                torch.cuda.synchronize()
                times[p].append((time.perf_counter() - t0) / args.reps)
                assert bool(torch.isfinite(y).all())
        for p in precisions:
            dt = min(times[p])
            print(f"{label} {p} n_fft={n_fft} frames={frames} batch={args.batch}: {dt * 1e3:.2f} ms/forward (rounds: "
                  f"{' '.join(f'{t * 1e3:.2f}' for t in times[p])}), {per[p] / 1e12:.2f} TFLOP conv -> {per[p] / dt / 1e12:.1f} TFLOP/s = "
                  f"{per[p] / dt / PEAK[p] * 100:.1f} % of the {p} MFMA peak; {args.batch * (frames - 256) * 1024 / 44100 / dt:.0f}x realtime per "
                  f"stem pair at hop 1024")
        if len(precisions) == 2:
            print(f"{label}: f16 forward {min(times['f32']) / min(times['f16']):.2f}x the float32 one")
        del nets
    if args.track > 0:
        from audiolab_amd.engine import Separator
        from oracle.toy import synth_mix
        wave = synth_mix(int(44100 * args.track), seed=5)
        tmp = tempfile.mkdtemp()
        for name in ("17_HP-Wind_Inst-UVR.pth", "UVR-DeNoise.pth"):
            seps = {p: Separator(model_file_dir=tmp, ctx=ctx, allow_synthetic=True, vr_precision=p, log_level=40) for p in precisions}
            best = {}
            for p in precisions:
                seps[p].load_model(name)
                seps[p].separate_array(wave[:, :44100 * 10])                    # warm-up
            for _ in range(2):
                for p in precisions:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    seps[p].separate_array(wave)
                    torch.cuda.synchronize()
                    best[p] = min(best.get(p, 1e9), time.perf_counter() - t0)
            print(f"engine {name} {args.track:.0f} s track (front end, network, back end; synthetic weights): " +
                  ", ".join(f"{p} {best[p]:.3f} s" for p in precisions) +
                  (f" -> {best['f32'] / best['f16']:.2f}x" if len(precisions) == 2 else ""))


if __name__ == "__main__":
    main()
