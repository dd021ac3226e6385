"""HDemucs (hdemucs_mmi's structure, synthetic weights) on one GPU: seconds per track through DemucsRunner (shifts 2, overlap 0.25), the
recurrent kernel's time per step at the production shapes against the full-rate estimate, and the LocalState score kernel's bandwidth.

    python scripts/bench_hdemucs.py [--seconds 600] [--micro-only]

Prints one JSON line.  Launch counts and the share of GPU time per kernel come from a ``rocprofv3 --kernel-trace --stats`` run of the same
script (profiles/hdemucs_*.txt)."""
import argparse
import json
import math
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CU_FLOP_PER_CLK, CLK_HZ, CUS = 256, 2.4e9, 256          # the issue's full-rate estimate: one CU, float32 matrix rate


def _events(fn, reps: int) -> float:
    """mean milliseconds of fn() over reps launches, HIP events on the current stream"""
    fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def micro(ctx) -> dict:
    out = {}
    # the recurrence at hdemucs_mmi's shapes on a batch of 8 units of 40 s: layer 4 T 1723 -> 18 frames, H 192; layer 5 T 862 -> 9, H 384
    for H, frames in ((192, 18), (384, 9)):
        N, T = 8 * frames, 200
        pre = torch.randn(T * N, 8 * H, device=ctx.device) * 0.3
        whh = torch.randn(2, H, 4 * H, device=ctx.device) / math.sqrt(H)
        h = torch.empty(T * N, 2 * H, device=ctx.device)
        ms = _events(lambda: ctx.check(ctx.lib.alsep_nn_lstm(ctx.handle, pre.data_ptr(), whh.data_ptr(), h.data_ptr(), T, N, H), "alsep_nn_lstm"), 5)
        step_us = ms * 1e3 / T
        est_us = 2 * 16 * H * 4 * H / (CU_FLOP_PER_CLK * CLK_HZ) * 1e6             # one 16-sequence tile at the CU's full f32 rate
        out[f"lstm_H{H}"] = dict(N=N, T=T, tiles=2 * (-(-N // 16)), ms=round(ms, 3), step_us=round(step_us, 2), estimate_step_us=round(est_us, 2),
                                 ratio=round(step_us / est_us, 2))
    # the LocalState score kernel: 8 units x 4 heads, T 1723 (layer 4 at 40 s), scores read and written in place
    G, heads, T, nd = 8, 4, 1723, 4
    Tp = -(-T // 4) * 4
    sc = torch.randn(G * heads * T, Tp, device=ctx.device)
    qd = torch.randn(G * T, heads * nd, device=ctx.device)
    ms = _events(lambda: ctx.check(ctx.lib.alsep_nn_localstate_softmax(ctx.handle, sc.data_ptr(), qd.data_ptr(), G, heads, T, Tp, nd, heads * nd),
                                   "alsep_nn_localstate_softmax"), 10)
    nbytes = 2 * 4 * G * heads * T * T + 4 * G * T * heads * nd                      # the matrix read and written once + the decay projection
    out["localstate_softmax"] = dict(G=G, heads=heads, T=T, us=round(ms * 1e3, 1), GBps=round(nbytes / (ms * 1e-3) / 1e9, 1),
                                     note="three reads (max, sum, normalise) and one write per element; GB/s counts one read and one write")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=int, default=600)
    ap.add_argument("--micro-only", action="store_true")
    ap.add_argument("--no-micro", action="store_true")
    args = ap.parse_args()
    from audiolab_amd import _lib
    from audiolab_amd.hdemucs import HDemucs, HDemucsConfig, synthetic_state_dict
    from audiolab_amd.htdemucs import DemucsRunner
    ctx = _lib.Context("cuda:0")
    res = {"workload": "hdemucs_mmi", "weights": "synthetic", "shifts": 2, "overlap": 0.25}
    if not args.no_micro:
        res["micro"] = micro(ctx)
    if not args.micro_only:
        cfg = HDemucsConfig()
        net = HDemucs(cfg, synthetic_state_dict(cfg, seed=0), ctx=ctx)
        runner = DemucsRunner(net, shifts=2, overlap=0.25)
        g = torch.Generator().manual_seed(0)
        warm = (torch.randn(2, 45 * 44100, generator=g) * 0.2).cuda()
        runner.separate(warm)
        torch.cuda.synchronize()
        mix = (torch.randn(2, args.seconds * 44100, generator=g) * 0.2).cuda()
        t0 = time.perf_counter()
        out = runner.separate(mix)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        res.update(track_seconds=args.seconds, seconds_per_track=round(dt, 3), units=len(runner.units(mix.shape[-1])[0]),
                   batched_forwards=runner.batches_run, lanes=runner.lanes, finite=all(bool(torch.isfinite(v).all()) for v in out.values()))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
