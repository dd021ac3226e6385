"""CPU emulation of the unchanged kernel sources: the final 1x1 convolution folded into the last residual TDF launch against the
separate final_conv_kernel (ALSEP_TDF_FINAL=0).  The network has one level, so the folded launch is a decoder block (level 0:
second linear 192 -> 768 on the wide 192-row kernel, C = 48) and the encoder's level-0 launch of the same kernel stays unfolded;
the bottleneck runs the 128-row kernel.  One subprocess per environment: the switch is read once."""
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CODE = (
    "import json, os, sys, torch; sys.path.insert(0, %r)\n"
    "from audiolab_amd import _lib\n"
    "_lib._LIB=_lib.bind(%r); _lib.DEVICE_TYPE='cpu'\n"
    "from audiolab_amd.synth import synthetic_state_dict\n"
    "from audiolab_amd.tdfnet import TDFNet, TDFNetConfig\n"
    "from oracle import tdfnet_oracle\n"
    "dt={'bf16': torch.bfloat16, 'f16': torch.float16}[sys.argv[2]]\n"
    "cfg=TDFNetConfig(dim_f=768, dim_t=8, n_fft=2048, hop=64, num_blocks=3, g=48, bn=4)\n"
    "sd=synthetic_state_dict(cfg, calib_frames=8)\n"
    "ctx=_lib.Context('cpu')\n"
    "net=TDFNet(cfg, sd, ctx=ctx, dtype=dt, max_batch=2)\n"
    "x=(torch.randn((2,4,768,8), generator=torch.Generator().manual_seed(5))*4).to(dt)\n"
    "want=tdfnet_oracle.forward(sd, x.float(), cfg.num_blocks, cfg.l, cfg.bn)\n"
    "ctx.launch_counts_reset()\n"
    "got=net.forward_nhwc(x.permute(0,3,2,1).contiguous(), denoise=sys.argv[3]=='1').float().permute(0,3,2,1)\n"
    "counts={k: ctx.launch_count(k) for k in ('final_conv_kernel','tdf_bf16_wide_kernel<res,final>','tdf_bf16_wide_kernel<res>','tdf_bf16_wide_kernel<nores>')}\n"
    "if sys.argv[3]=='0':\n"
    "    rel=float((got-want).norm()/want.norm()); print('rel', rel); assert rel < 3e-2\n"
    "torch.save((got, counts), sys.argv[1])\n"
)


def run(emul_lib_path, tmp_path, tag, dtype, denoise, **env):
    path = str(tmp_path / f"{tag}.pt")
    r = subprocess.run([sys.executable, "-c", CODE % (ROOT, emul_lib_path), path, dtype, "1" if denoise else "0"],
                       env=dict(os.environ, **env), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    return torch.load(path)


def test_fold_matches_separate_final_conv(emul_lib_path, tmp_path):
    for dtype in ("bf16", "f16"):
        off, coff = run(emul_lib_path, tmp_path, "off" + dtype, dtype, False, ALSEP_TDF_FINAL="0")
        on, con = run(emul_lib_path, tmp_path, "on" + dtype, dtype, False)
        assert coff["final_conv_kernel"] == 1 and coff["tdf_bf16_wide_kernel<res,final>"] == 0, coff
        assert con["final_conv_kernel"] == 0 and con["tdf_bf16_wide_kernel<res,final>"] == 1, con
        # encoder and decoder level 0 on the wide kernel either way: the folded launch still counts as the residual one
        assert coff["tdf_bf16_wide_kernel<res>"] == con["tdf_bf16_wide_kernel<res>"] == 2, (coff, con)
        assert torch.equal(off, on), f"{dtype}: max diff {(off - on).abs().max()}"


def test_fold_skips_the_accumulating_denoise_pass(emul_lib_path, tmp_path):
    """out = 0.5 f(x) folds; out += -0.5 f(-x) reads `out` back and keeps final_conv_kernel."""
    off, coff = run(emul_lib_path, tmp_path, "doff", "bf16", True, ALSEP_TDF_FINAL="0")
    on, con = run(emul_lib_path, tmp_path, "don", "bf16", True)
    assert coff["final_conv_kernel"] == 2 and coff["tdf_bf16_wide_kernel<res,final>"] == 0, coff
    assert con["final_conv_kernel"] == 1 and con["tdf_bf16_wide_kernel<res,final>"] == 1, con
    assert torch.equal(off, on), f"max diff {(off - on).abs().max()}"
