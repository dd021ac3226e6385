"""Which kernel run_conv_dma sends a bf16 3x3 conv to, per setting of the ALSEP_CONV_* switches, on the CPU emulation and on the GPU.
The network is the smallest at which every level fits its 8-wave kernel's tiles: dim_f = 768, dim_t = 32, five blocks, batch 1 -- level 0
32 x 768 at c = 48 (m0: 8 x 48 tiles), level 1 16 x 384 at c = 96 (mq: 8 x 64), level 2 (the bottleneck) 8 x 192 at c = 144 (big<3>: 8 x 64);
three convs per block, so every level's kernel is launched 6, 6 and 3 times.  One subprocess per setting and back end: the switches are
read once per process.  Each run is made once and shared by the tests below."""
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("conv3x3_bf16_m0_kernel", "conv3x3_bf16_mq_kernel", "conv3x3_bf16_big_kernel", "conv3x3_bf16_big_kernel<2>",
         "conv3x3_bf16_big_kernel<3>", "conv3x3_bf16_regw_kernel", "conv3x3_bf16_kernel", "conv3x3_bf16_kernel<64>",
         "conv3x3_bf16_kernel<small>", "conv3x3_bf16_pipe_kernel", "conv3x3_bf16_mny_kernel<2>", "conv3x3_bf16_mny_kernel<3>")

# argv: out.pt device library ("" = the package's own)
CODE = (
    "import os, sys, torch; sys.path.insert(0, %r)\n"
    "from audiolab_amd import _lib\n"
    "if sys.argv[3]: _lib._LIB=_lib.bind(sys.argv[3]); _lib.DEVICE_TYPE='cpu'\n"
    "from audiolab_amd.synth import synthetic_state_dict\n"
    "from audiolab_amd.tdfnet import TDFNet, TDFNetConfig\n"
    "cfg=TDFNetConfig(dim_f=768, dim_t=32, n_fft=2048, hop=64, num_blocks=5, g=48)\n"
    "sd=synthetic_state_dict(cfg, calib_frames=8)\n"
    "ctx=_lib.Context(sys.argv[2])\n"
    "net=TDFNet(cfg, sd, ctx=ctx, dtype=torch.bfloat16, max_batch=1)\n"
    "x=(torch.randn((1,cfg.dim_t,cfg.dim_f,4), generator=torch.Generator().manual_seed(11))*4).to(torch.bfloat16).to(ctx.device)\n"
    "ctx.launch_counts_reset()\n"
    "got=net.forward_nhwc(x).float().cpu()\n"
    "counts={k: ctx.launch_count(k) for k in %r}\n"
    "torch.save((got, counts), sys.argv[1])\n"
)

SETTINGS = {
    "default": {},
    "m0_big": dict(M0=2, BIG=2),
    "big": dict(M0=0, BIG=2),
    "m0_big_nomq": dict(M0=2, BIG=2, MQ=0),
    "m0_big_nobig3": dict(M0=2, BIG=2, BIG3=0),
    "plain": dict(M0=0, BIG=0, REGW=0),
    "regw2": dict(M0=0, BIG=0, REGW=2),
    "regw3": dict(M0=0, BIG=0, REGW=3),
}


def counts(m0=0, mq=0, big3=0, regw=0, k64=0):
    """the non-zero entries of a row; a big<3> / plain launch is noted under its generic and its instance name"""
    row = dict.fromkeys(NAMES, 0)
    row.update({"conv3x3_bf16_m0_kernel": m0, "conv3x3_bf16_mq_kernel": mq, "conv3x3_bf16_big_kernel": big3,
                "conv3x3_bf16_big_kernel<3>": big3, "conv3x3_bf16_regw_kernel": regw, "conv3x3_bf16_kernel": k64,
                "conv3x3_bf16_kernel<64>": k64})
    return row


# Recorded from the parent of the commit that introduced this test (the tree that still had the experiments build): CODE above run on
# that tree's CPU emulation with each setting and no experiments variable set.  The code under test never writes this table.
# One row needs a second look.  The parent's emulation was compiled with the experiments define, a dispatch the shipped library never had:
# there MQ=0 sent c = 96 to the experiments-only big<2> instance, and "m0_big_nomq" read big_kernel 9, big_kernel<2> 6, big_kernel<3> 3
# and no plain launch.  The shipped dispatch fell through to the plain kernel; that instance is removed with the experiments build.
# The row below is the parent's sources compiled for the emulation WITHOUT that define (its product dispatch); the other seven rows
# came out the same from both builds of the parent.
TABLE = {
    "default": counts(regw=6, k64=9),
    "m0_big": counts(m0=6, mq=6, big3=3),
    "big": counts(regw=6, mq=6, big3=3),
    "m0_big_nomq": counts(m0=6, big3=3, k64=6),
    "m0_big_nobig3": counts(m0=6, mq=6, k64=3),
    "plain": counts(k64=15),
    "regw2": counts(regw=12, k64=3),
    "regw3": counts(regw=12, k64=3),
}

# Every 48-channel-chunk kernel (plain, regw, big<3>, m0) sums a layer's products in the same order: bit-identical results
# (test_gpu_conv_variants.py, test_gpu_parity.py).  mq (32-channel chunks) sums in another order: its runs form a group of their own.
GROUPS = (("default", "plain", "regw2", "regw3", "m0_big_nomq"), ("m0_big", "big", "m0_big_nobig3"))

_runs = {}


def run(dev, request, tmp_path_factory, key):
    """(output, launch counts) of SETTINGS[key] on dev's back end, computed once"""
    cpu = dev.device.type == "cpu"
    if (cpu, key) not in _runs:
        lib = request.getfixturevalue("emul_lib_path") if cpu else ""
        path = str(tmp_path_factory.mktemp("conv_dispatch") / f"{key}.pt")
        env = dict(os.environ, **{f"ALSEP_CONV_{k}": str(v) for k, v in SETTINGS[key].items()})
        r = subprocess.run([sys.executable, "-c", CODE % (ROOT, NAMES), path, "cpu" if cpu else "cuda:0", lib], env=env,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        _runs[(cpu, key)] = torch.load(path)
    return _runs[(cpu, key)]


@pytest.mark.parametrize("key", list(SETTINGS))
def test_launch_counts(dev, request, tmp_path_factory, key):
    got, n = run(dev, request, tmp_path_factory, key)
    assert torch.isfinite(got).all() and float(got.abs().max()) > 1e-3
    assert n == TABLE[key], (key, {k: (n[k], TABLE[key][k]) for k in NAMES if n[k] != TABLE[key][k]})


def test_bit_identical_groups(dev, request, tmp_path_factory):
    for group in GROUPS:
        base = run(dev, request, tmp_path_factory, group[0])[0]
        for key in group[1:]:
            got = run(dev, request, tmp_path_factory, key)[0]
            assert torch.equal(base, got), f"{key} vs {group[0]}: max diff {(base - got).abs().max()}"
