"""CPU emulation of the unchanged kernel sources: the residual TDF linear on the persistent kernel (tdf_bf16_persist_kernel: two units
x all M rows per work item, the hidden tile resident in LDS) against the wide kernel it replaces (ALSEP_TDF_PERSIST=0).  Same MFMA
order and the same epilogue arithmetic, so the network's output must be the same bits; the launch counts say which instance ran.
Level-0 shape at the benchmark's K: M = 3072, K = 384, C = 48, 16 row blocks; the network's only block is its last one, so the launch
also folds the final 1x1 convolution (FINAL), and the accumulating denoise pass runs the unfolded instance.  One subprocess per
environment: the switches are read once."""
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# argv: out.pt dtype batch denoise
CODE = (
    "import os, sys, torch; sys.path.insert(0, %r)\n"
    "from audiolab_amd import _lib\n"
    "_lib._LIB=_lib.bind(%r); _lib.DEVICE_TYPE='cpu'\n"
    "from audiolab_amd.synth import synthetic_state_dict\n"
    "from audiolab_amd.tdfnet import TDFNet, TDFNetConfig\n"
    "dt={'bf16': torch.bfloat16, 'f16': torch.float16}[sys.argv[2]]\n"
    "nb=int(sys.argv[3])\n"
    "cfg=TDFNetConfig(dim_f=3072, dim_t=8, g=48, num_blocks=1, bn=8)\n"
    "sd=synthetic_state_dict(cfg, calib_frames=8)\n"
    "ctx=_lib.Context('cpu')\n"
    "net=TDFNet(cfg, sd, ctx=ctx, dtype=dt, max_batch=nb)\n"
    "x=(torch.randn((nb,cfg.dim_t,cfg.dim_f,4), generator=torch.Generator().manual_seed(7))*4).to(dt)\n"
    "ctx.launch_counts_reset()\n"
    "got=net.forward_nhwc(x, denoise=sys.argv[4]=='1').float()\n"
    "counts={k: ctx.launch_count(k) for k in ('tdf_bf16_persist_kernel','tdf_bf16_wide_kernel<res,final>','tdf_bf16_wide_kernel<res>','final_conv_kernel')}\n"
    "torch.save((got, counts), sys.argv[1])\n"
)


def run(emul_lib_path, tmp_path, tag, dtype="bf16", batch=2, denoise=False, **env):
    path = str(tmp_path / f"{tag}.pt")
    r = subprocess.run([sys.executable, "-c", CODE % (ROOT, emul_lib_path), path, dtype, str(batch), "1" if denoise else "0"],
                       env=dict(os.environ, **env), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    return torch.load(path)


def check(off, coff, on, con, launches, folded, what):
    assert torch.isfinite(off).all() and float(off.abs().max()) > 1e-3, what
    assert coff["tdf_bf16_persist_kernel"] == 0 and con["tdf_bf16_persist_kernel"] == launches, (what, coff, con)
    for c in (coff, con):                                     # the pinned names count layer launches, whichever instance serves them
        assert c["tdf_bf16_wide_kernel<res>"] == launches and c["tdf_bf16_wide_kernel<res,final>"] == folded, (what, coff, con)
    assert coff["final_conv_kernel"] == con["final_conv_kernel"], (what, coff, con)
    assert torch.equal(off, on), f"{what}: max diff {(off - on).abs().max()}"


def test_level0_bench_k_with_fold(emul_lib_path, tmp_path):
    """batch 2 = 16 units = 8 items, one per workgroup; bf16 and f16 translation units"""
    for dtype in ("bf16", "f16"):
        off, coff = run(emul_lib_path, tmp_path, "off" + dtype, dtype, ALSEP_TDF_PERSIST="0")
        on, con = run(emul_lib_path, tmp_path, "on" + dtype, dtype, ALSEP_TDF_PERSIST="1")
        check(off, coff, on, con, 1, 1, dtype)


def test_unfolded_instance_in_the_denoise_pass(emul_lib_path, tmp_path):
    """out = 0.5 f(x) folds; out += -0.5 f(-x) keeps final_conv_kernel, so its residual launch stores Y (batch 1: 4 items)"""
    off, coff = run(emul_lib_path, tmp_path, "doff", batch=1, denoise=True, ALSEP_TDF_PERSIST="0")
    on, con = run(emul_lib_path, tmp_path, "don", batch=1, denoise=True, ALSEP_TDF_PERSIST="1")
    check(off, coff, on, con, 2, 1, "denoise")


def test_several_items_per_workgroup(emul_lib_path, tmp_path):
    """grid capped at 3: the workgroups loop over 3, 3 and 2 of the 8 items, refilling the resident tile"""
    off, coff = run(emul_lib_path, tmp_path, "goff", ALSEP_TDF_PERSIST="0")
    on, con = run(emul_lib_path, tmp_path, "gon", ALSEP_TDF_PERSIST="1", ALSEP_TDF_PERSIST_GRID="3")
    check(off, coff, on, con, 1, 1, "grid 3")
