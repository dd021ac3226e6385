"""Shared by test_emul_tdf_us_fold.py and test_gpu_tdf_us_fold.py: forwards of small networks in a fresh process per environment (the
routing switches are read once per process), returning outputs, launch counts and, on request, the storage oracle's output.

tdf_bf16_persist_kernel<3, false, true> is the residual TDF linear of the level-1 block under the last upsampling (C = 96, K = 192)
with that upsampling (2x2 transposed conv 96 -> 48, BN, ReLU, times the level-0 skip) folded into its epilogue; ALSEP_TDF_US_FOLD=0 is
the pair it replaces, tdf_bf16_persist_kernel<3, false> + us_stream_kernel<96, 48>.  Shapes are the smallest that route the level-1
residual linear to the persistent kernel at C = 96: g = 48, level-1 F a multiple of 384, hidden width 192, level-1 frames x batch even:
  F384      dim_f = 768, bn = 2: level-1 F = 384, one row block per wave; three blocks, so the folded launch is the bottleneck's
  F768      dim_f = 1536, bn = 4: level-1 F = 768, two row blocks per wave
  T16       F384 with dim_t = 16 (8 level-1 frames per batch entry instead of the minimum 4)
  DEEP      F384 with five blocks: the folded launch is the first decoder block's, behind a level-2 bottleneck and a 144 -> 96 upsampling
An item is one level-1 frame: batch 1 at dim_t = 8 is 4 items, batch 3 is 12; ALSEP_TDF_PERSIST_GRID caps the grid (1 and 2 workgroups
walk 12 / 6 items each, refilling the resident tile)."""
import json
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = "tdf_bf16_persist_kernel<us>"
US = ("us_stream_kernel", "us_stream_kernel<96,48>")
PINNED = ("tdf_bf16_kernel", "tdf_bf16_wide_kernel<res>", "tdf_bf16_wide_kernel<nores>", "tdf_bf16_wide_kernel<res,final>",
          "tdf_bf16_persist_kernel", "tdf_gemm_kernel", "pix_gemm_kernel", "ds_stream_kernel", "final_conv_kernel", "conv3x3_bf16_kernel",
          "pix stream kernel") + US
OFF = {"ALSEP_TDF_US_FOLD": "0"}
ON = {"ALSEP_TDF_US_FOLD": "1"}
DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
F384 = dict(dim_f=768, dim_t=8, g=48, num_blocks=3, n_fft=1536, hop=256, bn=2)
F768 = dict(dim_f=1536, dim_t=8, g=48, num_blocks=3, n_fft=3072, hop=256, bn=4)
T16 = dict(F384, dim_t=16)
DEEP = dict(F384, num_blocks=5)

# argv: out.pt  device ("cuda" or the path of the emulation library)  dtype  jobs (json: [[config, batch], ...])  oracle ("1": also the
# storage oracle)
SCRIPT = r"""
import json, os, sys, torch
sys.path.insert(0, %(root)r)
from audiolab_amd import _lib
if sys.argv[2] != "cuda":
    _lib._LIB = _lib.bind(sys.argv[2]); _lib.DEVICE_TYPE = "cpu"
from audiolab_amd.synth import synthetic_state_dict
from audiolab_amd.tdfnet import TDFNet, TDFNetConfig
dev = "cuda:0" if sys.argv[2] == "cuda" else "cpu"
dt = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}[sys.argv[3]]
ctx = _lib.Context(dev)
res = []
for kw, batch in json.loads(sys.argv[4]):
    cfg = TDFNetConfig(**kw)
    sd = synthetic_state_dict(cfg, seed=1, calib_frames=8)
    x = (torch.randn((batch, cfg.dim_t, cfg.dim_f, 4), generator=torch.Generator().manual_seed(100)) * 4).to(dt)
    net = TDFNet(cfg, sd, ctx=ctx, dtype=dt, max_batch=batch)
    xd = x.to(dev)
    ctx.launch_counts_reset()
    first = net.forward_nhwc(xd).float().cpu()
    counts = {k: ctx.launch_count(k) for k in %(names)r}
    again = net.forward_nhwc(xd).float().cpu() if dev != "cpu" else first      # the emulation is synchronous: nothing to race
    want = None
    if sys.argv[5] == "1":
        from oracle import tdfnet_oracle
        with torch.no_grad():
            want = tdfnet_oracle.forward(sd, x.float().permute(0, 3, 2, 1).contiguous(), cfg.num_blocks, cfg.l, cfg.bn, storage=dt)
        want = want.float().permute(0, 3, 2, 1).contiguous()
    res.append((first, again, counts, want))
    del net
torch.save(res, sys.argv[1])
"""


def run_jobs(device, tmp_path, tag, dtype, jobs, env, timeout, oracle=False):
    """jobs: [(config, batch), ...], all in one process -> per job (output [B,T,F,4] float32, the same forward once more, launch counts
    of the first, the storage oracle's output or None)"""
    path = str(tmp_path / f"{tag}.pt")
    clean = {k: v for k, v in os.environ.items() if not k.startswith(("ALSEP_TDF_US_FOLD", "ALSEP_TDF_PERSIST"))}
    r = subprocess.run([sys.executable, "-c", SCRIPT % {"root": ROOT, "names": PINNED + (NEW,)}, path, device, dtype,
                        json.dumps([[c, b] for c, b in jobs]), "1" if oracle else "0"], env=dict(clean, **env), capture_output=True,
                       text=True, timeout=timeout)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    return torch.load(path)


def run(device, tmp_path, tag, dtype, cfg, env, timeout, batch=1, oracle=False):
    return run_jobs(device, tmp_path, tag, dtype, [(cfg, batch)], env, timeout, oracle)[0]


def check(off, on, what, folded):
    """a run against the reference run (ALSEP_TDF_US_FOLD=0): the same bits and every forward equal to its repetition; the new name
    `folded` times / never.  The pinned names count layer launches, whichever instance serves them (the folded launch is a residual
    TDF linear and the 96 -> 48 us layer), so every one of them is counted as often as in the reference run; only the new name tells
    the folded launch from the pair."""
    base, base2, cb, _ = off
    got, got2, cg, _ = on
    print(what, "folded launches", cb[NEW], cg[NEW], "us", [cb[k] for k in US], [cg[k] for k in US], "persist", cb["tdf_bf16_persist_kernel"],
          "peak", float(base.abs().max()), "max diff", float((base - got).abs().max()))
    assert torch.isfinite(base).all() and float(base.abs().max()) > 1e-3, what
    assert cb[NEW] == 0 and cg[NEW] == folded, (what, cb, cg)
    if folded:
        assert cb["us_stream_kernel<96,48>"] == 1 and cb["tdf_bf16_persist_kernel"] >= 1, (what, cb)
    assert {k: cg[k] for k in PINNED} == {k: cb[k] for k in PINNED}, (what, cb, cg)          # the pinned names count layer launches
    assert torch.equal(base, base2), what
    assert torch.equal(got, got2), f"{what}: two forwards differ by {(got - got2).abs().max()}"
    assert torch.equal(base, got), f"{what}: max diff {(base - got).abs().max()} (peak {base.abs().max()})"


def check_oracle(res, dtype, what):
    """against oracle/tdfnet_oracle.forward(storage=dtype), with the bound the half-precision network tests use for a three-block
    network against the storage oracle (tests/test_gpu_parity.py: HALF_BOUNDS)"""
    from test_gpu_parity import HALF_BOUNDS
    got, want = res[0], res[3]
    rel = float((got - want).double().norm() / want.double().norm())
    print(what, dtype, "rel L2 against the storage oracle", rel, "bound", HALF_BOUNDS[dtype][3][0])
    assert rel < HALF_BOUNDS[dtype][3][0], (what, dtype, rel)
