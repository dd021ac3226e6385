"""htdemucs_6s on the 10-minute synthetic track (shifts 2, overlap 0.25, synthetic weights) in one process: the float32 default and the
half-precision mode back to back after a warm-up, ``--runs`` timed runs each, per-track launch counts of the main kernels and the f16-vs-f32
rel-L2 / SDR of the stems.  ``--bag`` also times the htdemucs_ft-shaped bag (four members)."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=600.0)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--batch", type=int, default=None)
    ap.add_argument("--bag", action="store_true")
    ap.add_argument("--only-f16", action="store_true", help="time the half-precision mode alone (batch sweeps, profiles)")
    ap.add_argument("--classes", action="store_true", help="after the timed runs, one more f16 track with the per-class kernel timers "
                    "(convolution, norm, GEMM, attention): ms, TFLOP/s and share of the 2.5 PFLOP/s dense f16 MFMA peak")
    a = ap.parse_args()
    from audiolab_amd import _lib
    from audiolab_amd.htdemucs import DemucsRunner, HTDemucs, HTDemucsConfig, synthetic_state_dict
    from audiolab_amd.synth import synth_mix
    ctx = _lib.Context("cuda:0")
    cfg = HTDemucsConfig()
    sd = synthetic_state_dict(cfg, 0)
    mix = torch.from_numpy(synth_mix(int(a.seconds * cfg.samplerate))).cuda()
    kernels = ("nn_dconv_h_kernel", "nn_gemm_hh_kernel", "nn_gemm_h2_kernel", "nn_attn_h_kernel", "nn_xattn_h_kernel", "nn_norm_h_apply_kernel",
               "nn_conv2d_tiled_kernel", "nn_gemm_tn_kernel", "nn_bgemm_kernel")
    res = {}
    for prec in (("f16",) if a.only_f16 else ("f32", "f16")):
        nets = [HTDemucs(cfg, synthetic_state_dict(cfg, i) if a.bag else sd, ctx=ctx, precision=prec) for i in range(4 if a.bag else 1)]
        r = DemucsRunner(nets if a.bag else nets[0], shifts=2, overlap=0.25, batch=a.batch)
        out = r.separate(mix)
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.runs):
            ctx.launch_counts_reset()
            t0 = time.perf_counter()
            out = r.separate(mix)
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        counts = {k: ctx.launch_count(k) for k in kernels}
        counts = {k: v for k, v in counts.items() if v}
        res[prec] = torch.stack([out[s] for s in cfg.sources]).float()
        if a.classes and prec == "f16":
            for name, cat in (("conv (nn_dconv_h_kernel)", _lib.PROF_NN_DCONV_H), ("norm (nn_norm_h_*)", _lib.PROF_NN_NORM_H),
                              ("gemm (alsep_nn_gemm_f16)", _lib.PROF_NN_GEMM_H), ("attention", _lib.PROF_NN_ATTN_H)):
                ctx.profile_begin(cat)
                r.separate(mix)
                torch.cuda.synchronize()
                fl, by = ctx.profile_work()
                ms, n = ctx.profile_end()
                print(f"  class {name}: {n} launches, {ms:.1f} ms kernel time per track, {fl / ms * 1e-9:.1f} TFLOP/s = "
                      f"{fl / ms * 1e-9 / 2500 * 100:.1f} % of the f16 MFMA peak, {by / ms * 1e-6:.0f} GB/s", flush=True)
        print(f"{'bag' if a.bag else 'htdemucs_6s'} {prec}: lanes {r.lanes} batch {r.batch}: " + " ".join(f"{t * 1e3:.0f}" for t in ts) +
              f" ms per {a.seconds:.0f} s track (best {min(ts) * 1e3:.0f}); launches of the main kernels per track {counts}", flush=True)
    if a.only_f16:
        return
    d = res["f16"] - res["f32"]
    rel = float(d.norm() / res["f32"].norm())
    print(f"f16 vs f32: rel-L2 {rel:.3e}, SDR {-20 * torch.log10(torch.tensor(rel)).item():.1f} dB")


if __name__ == "__main__":
    main()
