"""CPU emulation of the unchanged kernel sources: the ds / us of the middle levels on the pipelined kernels (ds_pipe_kernel,
us_pipe_kernel: LDS ring filled by LDS-DMA ahead of the MFMAs, swizzled B fragment reads, the us product formed over the skip tile) against
the stream kernels they replace (ALSEP_PIX_PIPE=0).  Same weight fragments, k order, epilogue arithmetic and rounding: the network's output
must be the same bits; the launch counts say which instance ran.  dim_f = 512, dim_t = 8, batch 3, seven blocks: every stream launch once
per forward, 12 / 6 / 6 / 24 tiles of ds<96> / ds<144> / us<192,144> / us<144,96>; with the grid capped at 2 a workgroup runs 3 to 12 of them
(ring start-up, steady state, drain).  ALSEP_PIX_PIPE=2 sends all four instances to the new kernels whatever the product routes.  One
subprocess per environment: the switches are read once."""
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PINNED = ("ds_stream_kernel", "us_stream_kernel", "ds48_stream_kernel", "ds_split_stream_kernel<96>", "ds_split_stream_kernel<144>",
          "us_stream_kernel<96,48>", "us_stream_kernel<144,96>", "us_stream_kernel<192,144>", "pix_gemm_kernel")
NEW = ("ds_pipe_kernel<96>", "ds_pipe_kernel<144>", "us_pipe_kernel<192,144>", "us_pipe_kernel<144,96>")

# argv: out.pt dtype
CODE = (
    "import os, sys, torch; sys.path.insert(0, %r)\n"
    "from audiolab_amd import _lib\n"
    "_lib._LIB=_lib.bind(%r); _lib.DEVICE_TYPE='cpu'\n"
    "from audiolab_amd.synth import synthetic_state_dict\n"
    "from audiolab_amd.tdfnet import TDFNet, TDFNetConfig\n"
    "dt={'bf16': torch.bfloat16, 'f16': torch.float16}[sys.argv[2]]\n"
    "cfg=TDFNetConfig(dim_f=512, dim_t=8, g=48, num_blocks=7, bn=8, n_fft=1024)\n"
    "sd=synthetic_state_dict(cfg, calib_frames=8)\n"
    "ctx=_lib.Context('cpu')\n"
    "net=TDFNet(cfg, sd, ctx=ctx, dtype=dt, max_batch=3)\n"
    "x=(torch.randn((3,cfg.dim_t,cfg.dim_f,4), generator=torch.Generator().manual_seed(7))*4).to(dt)\n"
    "ctx.launch_counts_reset()\n"
    "got=net.forward_nhwc(x).float()\n"
    "counts={k: ctx.launch_count(k) for k in %r}\n"
    "torch.save((got, counts), sys.argv[1])\n"
)


def run(emul_lib_path, tmp_path, tag, dtype="bf16", **env):
    path = str(tmp_path / f"{tag}.pt")
    r = subprocess.run([sys.executable, "-c", CODE % (ROOT, emul_lib_path, PINNED + NEW), path, dtype],
                       env=dict(os.environ, **env), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    return torch.load(path)


def check(off, coff, on, con, what):
    assert torch.isfinite(off).all() and float(off.abs().max()) > 1e-3, what
    assert all(coff[k] == 0 for k in NEW) and all(con[k] == 1 for k in NEW), (what, coff, con)
    assert coff["pix_gemm_kernel"] == 0 and coff["ds_stream_kernel"] == 3 and coff["us_stream_kernel"] == 3, (what, coff)
    assert {k: con[k] for k in PINNED} == {k: coff[k] for k in PINNED}, (what, coff, con)      # the pinned names count layer launches
    assert torch.equal(off, on), f"{what}: max diff {(off - on).abs().max()}"


def test_several_tiles_per_workgroup(emul_lib_path, tmp_path):
    """grid capped at 2, bf16 translation unit; the uncapped grid (one tile per workgroup) against the same reference"""
    off, coff = run(emul_lib_path, tmp_path, "off", ALSEP_PIX_PIPE="0")
    on, con = run(emul_lib_path, tmp_path, "on", ALSEP_PIX_PIPE="2", ALSEP_PIX_PIPE_GRID="2")
    check(off, coff, on, con, "grid 2")
    on, con = run(emul_lib_path, tmp_path, "on1", ALSEP_PIX_PIPE="2")
    check(off, coff, on, con, "one tile per workgroup")


def test_f16_translation_unit(emul_lib_path, tmp_path):
    """the f16 unit compiles the same source with f16 MFMAs and storage"""
    off, coff = run(emul_lib_path, tmp_path, "hoff", "f16", ALSEP_PIX_PIPE="0")
    on, con = run(emul_lib_path, tmp_path, "hon", "f16", ALSEP_PIX_PIPE="2", ALSEP_PIX_PIPE_GRID="2")
    check(off, coff, on, con, "f16 grid 2")
