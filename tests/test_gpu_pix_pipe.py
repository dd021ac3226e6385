"""GPU (-m gpu): the ds / us of the middle levels on the pipelined kernels (ds_pipe_kernel<96|144>, us_pipe_kernel<192,144|144,96>:
persistent workgroups, activation and skip tiles in an LDS ring by LDS-DMA ahead of the MFMAs, the output image of a tile stored
under the next tile's MFMAs) against the stream kernels they replace (ALSEP_PIX_PIPE=0).  Same weight fragments, same k order, same
fp32 epilogue values and one rounding: the network's output must be the same bits, and the launch counts say which instance ran.
ALSEP_PIX_PIPE=1 is the product's routing (kPixPipeRouted in tdfnet.hip: an instance is routed to its new kernel only where it measured
faster), =2 sends all four instances to the new kernels.  Shapes: seven blocks reach all six stream launches once per forward;
dim_f = 512 makes the level-3 row one 64-pixel tile (the frame / window index changes at every tile) and, with the grid capped at 2,
gives a workgroup three to twelve tiles -- ring start-up, steady state and drain; dim_f = 1024, dim_t = 16 has several tiles per row
and, at three workgroups, uneven tails (11 + 11 + 10, 6 + 5 + 5).  One subprocess per environment (the switches are read once)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PINNED = ("ds_stream_kernel", "us_stream_kernel", "ds48_stream_kernel", "ds_split_stream_kernel<96>", "ds_split_stream_kernel<144>",
          "us_stream_kernel<96,48>", "us_stream_kernel<144,96>", "us_stream_kernel<192,144>", "pix_gemm_kernel")
NEW = ("ds_pipe_kernel<96>", "ds_pipe_kernel<144>", "us_pipe_kernel<192,144>", "us_pipe_kernel<144,96>")
ROUTED = {"ds_pipe_kernel<96>": 1, "ds_pipe_kernel<144>": 1, "us_pipe_kernel<192,144>": 1, "us_pipe_kernel<144,96>": 1}   # kPixPipeRouted
SHAPES = {"f512-t8-b3": (512, 8, 3), "f1024-t16-b2": (1024, 16, 2)}

# argv: out.npy counts.json dtype dim_f dim_t batch
SCRIPT = r"""
import json, os, sys, numpy as np, torch
sys.path.insert(0, %(root)r)
from audiolab_amd import _lib
from audiolab_amd.synth import synthetic_state_dict
from audiolab_amd.tdfnet import TDFNet, TDFNetConfig
dt = {"bf16": torch.bfloat16, "f16": torch.float16}[sys.argv[3]]
dim_f, dim_t, batch = int(sys.argv[4]), int(sys.argv[5]), int(sys.argv[6])
ctx = _lib.Context("cuda:0")
cfg = TDFNetConfig(dim_f=dim_f, dim_t=dim_t, g=48, num_blocks=7, bn=8, n_fft=2 * dim_f)
sd = synthetic_state_dict(cfg, seed=1, calib_frames=8)
net = TDFNet(cfg, sd, ctx=ctx, dtype=dt, max_batch=batch)
x = (torch.randn((batch, cfg.dim_t, cfg.dim_f, 4), generator=torch.Generator().manual_seed(100)) * 4).to(dt).cuda()
ctx.launch_counts_reset()
out = net.forward_nhwc(x).float().cpu().numpy()
json.dump({k: ctx.launch_count(k) for k in %(names)r}, open(sys.argv[2], "w"))
np.save(sys.argv[1], out)
"""


def run(tmp_path, tag, dtype, shape, **env):
    out, cnt = str(tmp_path / f"{tag}.npy"), str(tmp_path / f"{tag}.json")
    dim_f, dim_t, batch = SHAPES[shape]
    r = subprocess.run([sys.executable, "-c", SCRIPT % {"root": ROOT, "names": PINNED + NEW}, out, cnt, dtype, str(dim_f), str(dim_t), str(batch)],
                       env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return np.load(out), json.load(open(cnt))


def compare(tmp_path, dtype, shape, **env):
    base, cb = run(tmp_path, "off", dtype, shape, ALSEP_PIX_PIPE="0")
    assert np.isfinite(base).all() and np.abs(base).max() > 1e-3
    # the shape reaches all six stream launches once each and never the generic kernel
    assert all(cb[k] == 0 for k in NEW) and cb["pix_gemm_kernel"] == 0, cb
    assert all(cb[k] == (3 if k in ("ds_stream_kernel", "us_stream_kernel") else 1) for k in PINNED if k != "pix_gemm_kernel"), cb
    every = dict.fromkeys(NEW, 1)
    for mode, want in [("1", ROUTED)] + ([("2", every)] if ROUTED != every else []):     # all routed: the two modes are the same launches
        got, cg = run(tmp_path, "on" + mode, dtype, shape, ALSEP_PIX_PIPE=mode, **env)
        print("mode", mode, "counts", cg, "peak", float(np.abs(base).max()), "max diff", float(np.abs(base - got).max()))
        assert {k: cg[k] for k in NEW} == want, (mode, cg)
        assert {k: cg[k] for k in PINNED} == {k: cb[k] for k in PINNED}, (mode, cb, cg)
        assert np.array_equal(base, got), f"mode {mode}: max diff {np.abs(base - got).max()} (peak {np.abs(base).max()})"


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("shape,grid", [("f512-t8-b3", "2"), ("f1024-t16-b2", "3")])
def test_several_tiles_per_workgroup(tmp_path, dtype, shape, grid):
    """64-pixel tiles of ds<96> / 32-pixel tiles of the others: 12 / 6 / 6 / 24 at dim_f = 512 over two workgroups (three tiles
    each for ds<144> and us<192,144>), 32 / 16 / 16 / 64 at dim_f = 1024 over three (11 + 11 + 10 and 6 + 5 + 5)"""
    compare(tmp_path, dtype, shape, ALSEP_PIX_PIPE_GRID=grid)


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_one_tile_per_workgroup(tmp_path, dtype, shape):
    """no grid cap: fewer tiles than CUs, every workgroup fills its ring once and drains it"""
    compare(tmp_path, dtype, shape)


def test_fallback_stays_where_it_was(tmp_path):
    """ALSEP_PIX_STREAM=0: the generic kernel serves every ds / us, neither kernel family is reached and the new switch changes nothing"""
    base, cb = run(tmp_path, "foff", "bf16", "f512-t8-b3", ALSEP_PIX_STREAM="0", ALSEP_PIX_PIPE="0")
    got, cg = run(tmp_path, "fon", "bf16", "f512-t8-b3", ALSEP_PIX_STREAM="0", ALSEP_PIX_PIPE="2")
    print("counts off", cb, "on", cg)
    assert np.isfinite(base).all() and np.abs(base).max() > 1e-3
    assert all(cg[k] == 0 for k in NEW) and cg["pix_gemm_kernel"] == 6 and cg["ds_stream_kernel"] == 0, cg
    assert cb == cg, (cb, cg)
    assert np.array_equal(base, got), f"max diff {np.abs(base - got).max()}"
