"""GPU (-m gpu): the persistent register-weight 3x3 conv (counted vmcnt, LDS-DMA ring) must be
bit-identical to the plain LDS-DMA kernel (same MFMA order), on several batches -- a race in the
asynchronous ring would show up as a mismatch."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SCRIPT = r"""
import os, sys, numpy as np, torch
sys.path.insert(0, %(root)r)
from audiolab_amd import _lib
from audiolab_amd.synth import synthetic_state_dict
from audiolab_amd.tdfnet import TDFNet, TDFNetConfig
ctx = _lib.Context("cuda:0")
cfg = TDFNetConfig(dim_f=1536, dim_t=128, n_fft=4096, hop=256, num_blocks=7, g=48)      # 1536: a multiple of 64 and of 48 (the level-0 tiles)
sd = synthetic_state_dict(cfg, seed=1, calib_frames=32)
net = TDFNet(cfg, sd, ctx=ctx, dtype=torch.bfloat16, max_batch=6)
outs = []
for rep in range(3):
    g = torch.Generator().manual_seed(100 + rep)
    x = (torch.randn((7, cfg.dim_t, cfg.dim_f, 4), generator=g) * 4).to(torch.bfloat16).cuda()
    outs.append(net.forward_nhwc(x).float().cpu().numpy())
np.save(sys.argv[1], np.stack(outs))
"""


def run_mode(mode, path, **extra):
    regw, big = mode
    # ALSEP_CONV_MQ=0 unless asked for: the default level-1 kernel sums in another order (not bit-identical with the kernels compared here)
    env = dict(os.environ, ALSEP_CONV_REGW=str(regw), ALSEP_CONV_BIG=str(big))
    env.update({"ALSEP_CONV_MQ": "0", "ALSEP_CONV_M0": "0", **extra})
    r = subprocess.run([sys.executable, "-c", SCRIPT % {"root": ROOT}, path], env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    return np.load(path)


def test_persistent_conv_bit_identical(tmp_path):
    base = run_mode((0, 0), str(tmp_path / "m0.npy"))        # plain LDS-DMA kernel everywhere
    assert np.isfinite(base).all() and np.abs(base).max() > 1e-3
    for mode in [(1, 0), (2, 0), (3, 0), (1, 1), (0, 2)]:    # register-weight / big-tile (NY = 3)
        got = run_mode(mode, str(tmp_path / ("m%d%d.npy" % mode)))
        assert np.array_equal(base, got), f"REGW,BIG={mode}: max diff {np.abs(base - got).max()}"


def test_streaming_ds_us_match_tile_gemm(tmp_path):
    """The register-weight streaming ds / us kernels (48<->96, 96<->144 and 144<->192 channels) against the generic tile GEMM on the
    same layers: same bf16 MFMA and the same k order, so the results must agree bit for bit."""
    base = run_mode((1, 1), str(tmp_path / "s0.npy"), ALSEP_PIX_STREAM="0")
    got = run_mode((1, 1), str(tmp_path / "s1.npy"), ALSEP_PIX_STREAM="1")
    assert np.isfinite(base).all() and np.abs(base).max() > 1e-3
    assert np.array_equal(base, got), f"max diff {np.abs(base - got).max()} (peak {np.abs(base).max()})"


def test_dispatch_orders_and_prefetch_bit_identical(tmp_path):
    """XCD-local dispatch orders (plain conv: ALSEP_CONV_NYFAST, wide TDF: ALSEP_TDF_YFAST), the NY = 3 big-tile conv
    (ALSEP_CONV_BIG3) and the residual prefetch of the wide TDF epilogue (ALSEP_TDF_RPF) only change WHICH workgroup
    computes a tile or when a row is loaded -- every switch off must reproduce the default bit for bit."""
    base = run_mode((1, 1), str(tmp_path / "d0.npy"))
    assert np.isfinite(base).all() and np.abs(base).max() > 1e-3
    cases = [dict(ALSEP_CONV_NYFAST="0"), dict(ALSEP_TDF_YFAST="0"), dict(ALSEP_CONV_BIG3="0"), dict(ALSEP_TDF_RPF="0"), dict(ALSEP_CONV_M0="2"),
             dict(ALSEP_CONV_NYFAST="0", ALSEP_TDF_YFAST="0", ALSEP_CONV_BIG3="0", ALSEP_TDF_RPF="0")]
    for extra in cases:
        got = run_mode((1, 1), str(tmp_path / "d1.npy"), **extra)
        assert np.array_equal(base, got), f"{extra}: max diff {np.abs(base - got).max()}"
    # the fully double-buffered level-1 kernel sums a layer's products in another order (32-channel chunks): equal up to flipped bf16
    # roundings (measured 4.5e-3 relative L2 after three blocks), and deterministic -- a race in its LDS-DMA rings would not be
    a = run_mode((1, 1), str(tmp_path / "q0.npy"), ALSEP_CONV_MQ="1")
    b = run_mode((1, 1), str(tmp_path / "q1.npy"), ALSEP_CONV_MQ="1")
    assert np.array_equal(a, b), f"mq is not deterministic: max diff {np.abs(a - b).max()}"
    rel = float(np.linalg.norm(a - base) / np.linalg.norm(base))
    assert rel < 2e-2, f"mq vs the 48-channel kernels: rel L2 {rel:.3e}"
