#!/usr/bin/env python3
"""The Compare chain (``audiolab_amd.compare.compare_arrays`` and the ``Compare`` wrapper) at the size a user runs: a 5-minute stereo 16-bit
pair, once both at 44.1 kHz and once with the second file at 48 kHz.

Prints, per pair: ``compare_arrays`` from device-resident samples (device events around the call: warm-up first, then the median of
``--runs``) and its kernels by class -- resampling, sums of squares, normalisation / difference, spectra, and the two reductions at the
wrapper's column counts -- each from a profiled call of its own (the library's event brackets); the oracle's scipy time on this host's CPU
(tests/compare_oracle.py: resample, normalise, two stft calls, magnitudes, decibels) with a spot check of the GPU result against it; and the
wrapper end to end, file to PNG, with ``render`` "reduced" and "full".  Nothing here is asserted: the numbers are recorded."""
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
from audiolab_amd import _lib, compare, wavio  # noqa: E402

STAGES = (("resample", _lib.PROF_COMPARE_RESAMPLE), ("sums of squares", _lib.PROF_COMPARE_RMS), ("normalise / difference", _lib.PROF_COMPARE_WAVE),
          ("spectra", _lib.PROF_COMPARE_SPECTRA))


def song(frames: int, rate: int, seed: int) -> np.ndarray:
    """[2, frames] float32: noise, a decaying 220 Hz pulse train and a steady tone"""
    rng = np.random.default_rng(seed)
    t = np.arange(frames) / rate
    env = np.exp(-((t * 2.0) % 1.0) * 3.0)
    x = 0.1 * rng.standard_normal((2, frames)) + 0.3 * env * np.sin(2 * np.pi * 220.0 * t) + 0.2 * np.sin(2 * np.pi * 613.7 * t)
    return np.clip(x, -1.0, 1.0).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=300.0)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-full-render", action="store_true", help="skip the wrapper run with render='full' (matplotlib on the full arrays)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_compare: needs a GPU (cuda:0)")
    ctx = _lib.Context("cuda:0")
    from audiolab_amd.handlers import config
    from audiolab_amd.util.data_classes import ProjectFiles
    from audiolab_amd.wrappers.compare import Compare
    Compare.ctx = ctx
    print(f"Compare of two stereo 16-bit files of {args.seconds:g} s; {args.warmup} warm-up, median of {args.runs} runs", flush=True)
    with tempfile.TemporaryDirectory() as tmp:
        config.output_path = os.path.join(tmp, "outputs")
        for rate_b in (44100, 48000):
            pa, pb = os.path.join(tmp, "a.wav"), os.path.join(tmp, f"b{rate_b}.wav")
            a = song(int(args.seconds * 44100), 44100, 0)
            wavio.write_wav(pa, a, 44100, subtype="PCM_16")
            b = song(int(args.seconds * rate_b), rate_b, 0)
            b += 0.01 * np.random.default_rng(1).standard_normal(b.shape).astype(np.float32)
            wavio.write_wav(pb, b, rate_b, subtype="PCM_16")
            del a, b
            ta, tb = compare.load_track(pa), compare.load_track(pb)
            da, db = (ta[0].cuda(), ta[1]), (tb[0].cuda(), tb[1])
            print(f"-- 44100 Hz against {rate_b} Hz: {len(ta[0])} and {len(tb[0])} interleaved samples", flush=True)

            def call():
                return compare.compare_arrays(da, db, ctx=ctx)

            for _ in range(args.warmup):
                res = call()
            torch.cuda.synchronize()
            totals = []
            for _ in range(args.runs):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                res = call()
                e1.record()
                torch.cuda.synchronize()
                totals.append(e0.elapsed_time(e1))
            line = [f"compare_arrays ({res.differences.shape[0]} samples, {res.spec1_db.shape[1]} frames): total {statistics.median(totals):8.1f} ms"]
            for name, cat in STAGES:
                ms = []
                for _ in range(args.runs):
                    ctx.profile_begin(cat)
                    call()
                    ms.append(ctx.profile_end()[0])
                line.append(f"{name} {statistics.median(ms):8.2f} ms")
            ms = []
            for _ in range(args.runs):
                ctx.profile_begin(_lib.PROF_COMPARE_REDUCE)
                res.envelopes(Compare.plot_columns)
                res.spectra_reduced(Compare.spec_columns)
                ms.append(ctx.profile_end()[0])
            line.append(f"reductions ({Compare.plot_columns} / {Compare.spec_columns} columns) {statistics.median(ms):8.2f} ms")
            print("; ".join(line), flush=True)

            scipy_s = None
            if not args.no_cpu_baseline:
                from tests import compare_oracle as co
                t0 = time.perf_counter()
                want = co.compare((ta[0].numpy(), ta[1]), (tb[0].numpy(), tb[1]))
                scipy_s = time.perf_counter() - t0
                cols = np.linspace(0, want["spec1"].shape[1] - 1, 200).astype(np.int64)
                got = res.spec1_db[:, torch.from_numpy(cols).cuda()].cpu().numpy()
                err = float(np.max(np.abs(got - want["spec1_db"][:, cols])))
                pos = np.linspace(0, len(want["differences"]) - 1, 5000).astype(np.int64)
                errw = float(np.max(np.abs(res.differences[torch.from_numpy(pos).cuda()].cpu().numpy() - want["differences"][pos])))
                print(f"   scipy on this host's CPU (the oracle: resample, normalise, two stft, magnitudes, decibels): {scipy_s:.2f} s; "
                      f"max|GPU - scipy|: spec1_db at 200 frames {err:.2e} dB, differences at 5000 samples {errw:.2e}", flush=True)
                del want
            del res
            for render in ("reduced",) + (() if args.no_full_render else ("full",)):
                Compare.render = render
                project = ProjectFiles(pa)
                project.add_output("stems", [pb])
                t0 = time.perf_counter()
                Compare().process_audio([project])
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                note = ""
                if scipy_s is not None:
                    note = f" ({'under' if dt < scipy_s else 'NOT under'} the scipy arithmetic alone, {scipy_s:.2f} s)"
                print(f"   wrapper, file to PNG, render = {render!r}: {dt:.2f} s{note}", flush=True)
            Compare.render = "full"


if __name__ == "__main__":
    main()
