"""GPU (-m gpu): the final 1x1 convolution folded into the last residual TDF launch (tdf_bf16_wide_kernel<4, true, 2, FINAL>) against
the separate final_conv_kernel (ALSEP_TDF_FINAL=0, the path before the fold).  The folded epilogue rounds the block's output to the
storage type exactly as the store did and reduces each pixel's 48 channels in final_conv_kernel's order, so the network's output must
be the same bits; the launch counts say which of the two ran.  One subprocess per environment (the switches are read once)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# argv: out.npy counts.json dtype dim_f denoise
SCRIPT = r"""
import json, os, sys, numpy as np, torch
sys.path.insert(0, %(root)r)
from audiolab_amd import _lib
from audiolab_amd.synth import synthetic_state_dict
from audiolab_amd.tdfnet import TDFNet, TDFNetConfig
dt = {"bf16": torch.bfloat16, "f16": torch.float16}[sys.argv[3]]
dim_f, denoise = int(sys.argv[4]), sys.argv[5] == "1"
ctx = _lib.Context("cuda:0")
cfg = TDFNetConfig(dim_f=dim_f, dim_t=128, n_fft=4096, hop=256, num_blocks=7, g=48)
sd = synthetic_state_dict(cfg, seed=1, calib_frames=32)
net = TDFNet(cfg, sd, ctx=ctx, dtype=dt, max_batch=6)
outs, counts = [], []
for rep in range(3):
    g = torch.Generator().manual_seed(100 + rep)
    x = (torch.randn((7, cfg.dim_t, cfg.dim_f, 4), generator=g) * 4).to(dt).cuda()
    ctx.launch_counts_reset()
    outs.append(net.forward_nhwc(x, denoise=denoise).float().cpu().numpy())
    counts.append({k: ctx.launch_count(k) for k in ("final_conv_kernel", "tdf_bf16_wide_kernel<res,final>", "tdf_bf16_wide_kernel<res>")})
np.save(sys.argv[1], np.stack(outs))
json.dump(counts, open(sys.argv[2], "w"))
"""


def run(tmp_path, tag, dtype="bf16", dim_f=1536, denoise=False, **env):
    out, cnt = str(tmp_path / f"{tag}.npy"), str(tmp_path / f"{tag}.json")
    r = subprocess.run([sys.executable, "-c", SCRIPT % {"root": ROOT}, out, cnt, dtype, str(dim_f), "1" if denoise else "0"],
                       env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return np.load(out), json.load(open(cnt))


def check_counts(counts, final_conv, folded, what):
    for c in counts:                                          # one entry per input: batch 7 over max_batch 6 = two network launches
        assert c["final_conv_kernel"] == final_conv and c["tdf_bf16_wide_kernel<res,final>"] == folded, f"{what}: {c}"


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_fold_bit_identical(tmp_path, dtype):
    """Bench-like geometry (level 0: M = 1536, C = 48): the last decoder block's residual launch writes the spectrogram."""
    base, cb = run(tmp_path, "off", dtype, ALSEP_TDF_FINAL="0")
    assert np.isfinite(base).all() and np.abs(base).max() > 1e-3
    check_counts(cb, 2, 0, "fold off")
    got, cg = run(tmp_path, "on", dtype)                      # the default
    check_counts(cg, 0, 2, "fold on")
    for c, d in zip(cb, cg):                                  # the folded launch still counts as the residual wide kernel
        assert c["tdf_bf16_wide_kernel<res>"] == d["tdf_bf16_wide_kernel<res>"] >= 2, (c, d)
    assert np.array_equal(base, got), f"{dtype}: max diff {np.abs(base - got).max()} (peak {np.abs(base).max()})"


def test_fold_denoise_first_pass_only(tmp_path):
    """denoise: out = 0.5 f(x), then out += -0.5 f(-x).  The first pass (beta == 0) folds, the accumulating pass reads `out` back and
    keeps the separate kernel."""
    base, cb = run(tmp_path, "doff", denoise=True, ALSEP_TDF_FINAL="0")
    assert np.isfinite(base).all() and np.abs(base).max() > 1e-3
    check_counts(cb, 4, 0, "fold off")
    got, cg = run(tmp_path, "don", denoise=True)
    check_counts(cg, 2, 2, "fold on")
    assert np.array_equal(base, got), f"max diff {np.abs(base - got).max()}"


@pytest.mark.parametrize("case", [dict(dim_f=2048), dict(ALSEP_TDF_WIDE="0"), dict(ALSEP_TDF_WIDE="8"), dict(ALSEP_TDF_RPF="0")],
                         ids=["kuielab-2048", "wide0", "wide8", "rpf0"])
def test_fallbacks_keep_the_separate_kernel(tmp_path, case):
    """Where the 192-row wide kernel does not serve the last residual launch (level-0 M = 2048 is no multiple of 192; ALSEP_TDF_WIDE=0:
    128-row kernel; =8: 384-row workgroups; ALSEP_TDF_RPF=0: the timing-comparison instance) the final conv stays a launch of its own."""
    case = dict(case)
    dim_f = case.pop("dim_f", 1536)
    base, cb = run(tmp_path, "foff", dim_f=dim_f, ALSEP_TDF_FINAL="0", **case)
    assert np.isfinite(base).all() and np.abs(base).max() > 1e-3
    got, cg = run(tmp_path, "fon", dim_f=dim_f, **case)
    check_counts(cb, 2, 0, "fold off")
    check_counts(cg, 2, 0, "fold on")
    assert np.array_equal(base, got), f"max diff {np.abs(base - got).max()}"
