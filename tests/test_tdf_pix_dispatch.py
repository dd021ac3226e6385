"""Which kernel run_tdf_dma / run_tdf_fused send a bf16 TDF linear to, and run_pix_stream a ds / us layer, per setting of the ALSEP_TDF_*
and ALSEP_PIX_* switches: what test_conv_dispatch.py does for the 3x3 convs.  GPU only (the seven-block network is too slow on the
emulation).  The network is tdf_fused_common.DEEP at batch 1, the smallest in the tree in which level 0 (F = 3072, c = 48, K = 384)
reaches the persistent K = 384 and folded-final instances, level 1 (F = 1536, c = 96, K = 192) the K = 192 instance, levels 2 and 3
(F = 768 / 384) both fused instances, and every ds / us instance is launched (48 -> 96 -> 144 -> 192 and back).  One subprocess per
setting: the switches are read once per process.  Each run is made once and shared by the tests below."""
import json
import os
import subprocess
import sys

import pytest
import torch

from tdf_fused_common import DEEP

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tdf_bf16_kernel", "tdf_bf16_wide_kernel", "tdf_bf16_wide_kernel<res>", "tdf_bf16_wide_kernel<nores>",
         "tdf_bf16_wide_kernel<res,final>", "tdf_bf16_persist_kernel", "tdf_bf16_fused_kernel", "tdf_gemm_kernel", "tdf_gemm_f32s_kernel",
         "final_conv_kernel",
         "ds_stream_kernel", "ds48_stream_kernel", "ds_split_stream_kernel<96>", "ds_split_stream_kernel<144>", "ds_pipe_kernel<96>",
         "ds_pipe_kernel<144>", "us_stream_kernel", "us_stream_kernel<96,48>", "us_stream_kernel<144,96>", "us_stream_kernel<192,144>",
         "us_pipe_kernel<144,96>", "us_pipe_kernel<192,144>", "pix stream kernel", "pix_gemm_kernel", "pix_gemm_f32s_kernel")

# argv: out.pt config (json)
CODE = (
    "import json, sys, torch; sys.path.insert(0, %r)\n"
    "from audiolab_amd import _lib\n"
    "from audiolab_amd.synth import synthetic_state_dict\n"
    "from audiolab_amd.tdfnet import TDFNet, TDFNetConfig\n"
    "cfg=TDFNetConfig(**json.loads(sys.argv[2]))\n"
    "sd=synthetic_state_dict(cfg, seed=1, calib_frames=8)\n"
    "ctx=_lib.Context('cuda:0')\n"
    "net=TDFNet(cfg, sd, ctx=ctx, dtype=torch.bfloat16, max_batch=1)\n"
    "x=(torch.randn((1,cfg.dim_t,cfg.dim_f,4), generator=torch.Generator().manual_seed(11))*4).to(torch.bfloat16).to(ctx.device)\n"
    "ctx.launch_counts_reset()\n"
    "got=net.forward_nhwc(x).float().cpu()\n"
    "counts={k: ctx.launch_count(k) for k in %r}\n"
    "torch.save((got, counts), sys.argv[1])\n"
)

SETTINGS = {
    "default": {},
    "fused0": dict(TDF_FUSED=0),
    "fused2": dict(TDF_FUSED=2),
    "persist0": dict(TDF_PERSIST=0),
    "persist2": dict(TDF_PERSIST=2),
    "final0": dict(TDF_FINAL=0),
    "wide0": dict(TDF_WIDE=0),
    "wide4": dict(TDF_WIDE=4),
    "wide8": dict(TDF_WIDE=8),
    "rpf0": dict(TDF_RPF=0),
    "stream0": dict(PIX_STREAM=0),
    "pipe0": dict(PIX_PIPE=0),
    "pipe2": dict(PIX_PIPE=2),
}


def counts(plain=6, wide=4, res=4, nores=4, fold=1, persist=4, fused=0, final_conv=0, stream=1, pipe=1):
    """a row from its TDF entries (the default's unless given) and its ds / us entries (stream: the six layers on the stream path,
    else on pix_gemm_kernel; pipe: the four middle ones on the pipelined kernels, counted under their stream kernels' names as well)"""
    row = dict.fromkeys(NAMES, 0)
    row.update({"tdf_bf16_kernel": plain, "tdf_bf16_wide_kernel": wide, "tdf_bf16_wide_kernel<res>": res, "tdf_bf16_wide_kernel<nores>": nores,
                "tdf_bf16_wide_kernel<res,final>": fold, "tdf_bf16_persist_kernel": persist, "tdf_bf16_fused_kernel": fused,
                "final_conv_kernel": final_conv, "pix_gemm_kernel": 0 if stream else 6})
    if stream:
        row.update({"ds_stream_kernel": 3, "us_stream_kernel": 3, "pix stream kernel": 6, "ds48_stream_kernel": 1, "ds_split_stream_kernel<96>": 1,
                    "ds_split_stream_kernel<144>": 1, "us_stream_kernel<96,48>": 1, "us_stream_kernel<144,96>": 1, "us_stream_kernel<192,144>": 1,
                    "ds_pipe_kernel<96>": pipe, "ds_pipe_kernel<144>": pipe, "us_pipe_kernel<144,96>": pipe, "us_pipe_kernel<192,144>": pipe})
    return row


# Recorded on the GPU from the parent of the commit that introduced this test (the tree whose routing still sat in the launchers), before
# the host code was touched: CODE above run on that tree's library with each setting.  The code under test never writes this table.
# Fourteen TDF linears per forward: levels 0 and 1 (four blocks) on the wide kernel -- the four first linears on tdf_bf16_wide_kernel
# itself, the four residual ones on tdf_bf16_persist_kernel, counted under the wide kernel's <res> name and the last one under
# <res,final> as well --, levels 2 and 3 (three blocks) on tdf_bf16_kernel.  At batch 1 the default is below the fused kernel's floor, so
# only TDF_FUSED=2 reaches it: three launches, each counted twice under tdf_bf16_kernel.  TDF_PERSIST=0 / TDF_WIDE=4 keep the residual
# linears on the wide kernel; TDF_WIDE=8 and TDF_RPF=0 also lose the fold (final_conv_kernel is launched); TDF_WIDE=0 leaves every linear
# on tdf_bf16_kernel.  In the parent every setting gave the default's bits: one group.
TABLE = {
    "default": counts(),
    "fused0": counts(),
    "fused2": counts(fused=3),
    "persist0": counts(wide=8, persist=0),
    "persist2": counts(),
    "final0": counts(fold=0, final_conv=1),
    "wide0": counts(plain=14, wide=0, res=0, nores=0, fold=0, persist=0, final_conv=1),
    "wide4": counts(wide=8, persist=0),
    "wide8": counts(wide=8, persist=0, fold=0, final_conv=1),
    "rpf0": counts(wide=8, persist=0, fold=0, final_conv=1),
    "stream0": counts(stream=0),
    "pipe0": counts(pipe=0),
    "pipe2": counts(),
}

# Every one of these switches only chooses between kernels documented as bit-identical
GROUPS = (tuple(SETTINGS),)

_runs = {}


def run(tmp_path_factory, key):
    """(output, launch counts) of SETTINGS[key], computed once"""
    if key not in _runs:
        path = str(tmp_path_factory.mktemp("tdf_pix_dispatch") / f"{key}.pt")
        clean = {k: v for k, v in os.environ.items() if not k.startswith(("ALSEP_TDF_", "ALSEP_PIX_"))}
        env = dict(clean, **{f"ALSEP_{k}": str(v) for k, v in SETTINGS[key].items()})
        r = subprocess.run([sys.executable, "-c", CODE % (ROOT, NAMES), path, json.dumps(DEEP)], env=env, capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
        _runs[key] = torch.load(path)
    return _runs[key]


@pytest.mark.parametrize("key", list(SETTINGS))
def test_launch_counts(tmp_path_factory, key):
    got, n = run(tmp_path_factory, key)
    print(key, {k: v for k, v in n.items() if v})
    assert torch.isfinite(got).all() and float(got.abs().max()) > 1e-3
    assert n == TABLE[key], (key, {k: (n[k], TABLE[key][k]) for k in NAMES if n[k] != TABLE[key][k]})


def test_bit_identical_groups(tmp_path_factory):
    for group in GROUPS:
        base = run(tmp_path_factory, group[0])[0]
        for key in group[1:]:
            got = run(tmp_path_factory, key)[0]
            assert torch.equal(base, got), f"{key} vs {group[0]}: max diff {(base - got).abs().max()}"
