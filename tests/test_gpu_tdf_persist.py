"""GPU (-m gpu): the residual TDF linear of levels 0 and 1 on the persistent kernel (tdf_bf16_persist_kernel: a work item is two units x
all M rows, the hidden tile resident in LDS, workgroups striding over the items) against the wide kernel it replaces
(ALSEP_TDF_PERSIST=0).  Same MFMA order, same epilogue arithmetic: the network's output must be the same bits, and the launch counts
say which instance ran.  Shapes are the smallest that reach every branch: level 0 at the benchmark's K (M = 3072, K = 384, C = 48,
16 row blocks; with one block the launch also folds the final 1x1 convolution), level 1 (C = 96: the two units of an item are one
frame; M = 1536, K = 192: three K tiles).  One subprocess per environment (the switches are read once)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("tdf_bf16_persist_kernel", "tdf_bf16_wide_kernel<res>", "tdf_bf16_wide_kernel<res,final>", "final_conv_kernel")

# argv: out.npy counts.json dtype dim_f num_blocks batch denoise
SCRIPT = r"""
import json, os, sys, numpy as np, torch
sys.path.insert(0, %(root)r)
from audiolab_amd import _lib
from audiolab_amd.synth import synthetic_state_dict
from audiolab_amd.tdfnet import TDFNet, TDFNetConfig
dt = {"bf16": torch.bfloat16, "f16": torch.float16}[sys.argv[3]]
dim_f, num_blocks, batch, denoise = int(sys.argv[4]), int(sys.argv[5]), int(sys.argv[6]), sys.argv[7] == "1"
ctx = _lib.Context("cuda:0")
cfg = TDFNetConfig(dim_f=dim_f, dim_t=8, g=48, num_blocks=num_blocks, bn=8)
sd = synthetic_state_dict(cfg, seed=1, calib_frames=8)
net = TDFNet(cfg, sd, ctx=ctx, dtype=dt, max_batch=batch)
x = (torch.randn((batch, cfg.dim_t, cfg.dim_f, 4), generator=torch.Generator().manual_seed(100)) * 4).to(dt).cuda()
ctx.launch_counts_reset()
out = net.forward_nhwc(x, denoise=denoise).float().cpu().numpy()
json.dump({k: ctx.launch_count(k) for k in %(names)r}, open(sys.argv[2], "w"))
np.save(sys.argv[1], out)
"""


def run(tmp_path, tag, dtype="bf16", dim_f=3072, num_blocks=1, batch=4, denoise=False, **env):
    out, cnt = str(tmp_path / f"{tag}.npy"), str(tmp_path / f"{tag}.json")
    r = subprocess.run([sys.executable, "-c", SCRIPT % {"root": ROOT, "names": NAMES}, out, cnt, dtype, str(dim_f), str(num_blocks),
                        str(batch), "1" if denoise else "0"], env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return np.load(out), json.load(open(cnt))


def compare(tmp_path, launches, folded, on_env=None, **kw):
    """ALSEP_TDF_PERSIST=0 against the default: `launches` residual launches of the wide family, all of them on the new instance"""
    base, cb = run(tmp_path, "off", ALSEP_TDF_PERSIST="0", **kw)
    got, cg = run(tmp_path, "on", ALSEP_TDF_PERSIST="1", **(on_env or {}), **kw)
    print("counts off", cb, "on", cg, "peak", float(np.abs(base).max()), "max diff", float(np.abs(base - got).max()))
    assert np.isfinite(base).all() and np.abs(base).max() > 1e-3
    assert cb["tdf_bf16_persist_kernel"] == 0 and cg["tdf_bf16_persist_kernel"] == launches, (cb, cg)
    for c in (cb, cg):                                        # the pinned names count layer launches, whichever instance serves them
        assert c["tdf_bf16_wide_kernel<res>"] == launches and c["tdf_bf16_wide_kernel<res,final>"] == folded, (cb, cg)
    assert cb["final_conv_kernel"] == cg["final_conv_kernel"], (cb, cg)
    assert np.array_equal(base, got), f"max diff {np.abs(base - got).max()} (peak {np.abs(base).max()})"


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("batch", [4, 3], ids=["b4-1d-grid", "b3-2d-grid"])
def test_level0_bench_k(tmp_path, dtype, batch):
    """batch 4: 8 column tiles, the wide kernel's row-block-fastest 1-D grid; batch 3: 6 column tiles, its 2-D grid.  The only block
    is the last one: the launch folds the final convolution."""
    compare(tmp_path, 1, 1, dtype=dtype, batch=batch)


def test_level0_denoise_unfolded_second_pass(tmp_path):
    """out = 0.5 f(x) folds; out += -0.5 f(-x) keeps final_conv_kernel: its residual launch is the unfolded K = 384 instance"""
    compare(tmp_path, 2, 1, denoise=True)


@pytest.mark.parametrize("batch", [2, 3])
def test_level1_shape(tmp_path, batch):
    """three blocks: level 0 unfolded (encoder), level 1 (C = 96, M = 1536, K = 192), level 0 folded (decoder)"""
    compare(tmp_path, 3, 1, num_blocks=3, batch=batch)


def test_several_items_per_workgroup(tmp_path):
    """grid capped at 3: 16 items over three workgroups (6, 5, 5), each refilling its resident tile"""
    compare(tmp_path, 1, 1, on_env=dict(ALSEP_TDF_PERSIST_GRID="3"))


@pytest.mark.parametrize("case", [dict(dim_f=2048), dict(ALSEP_TDF_WIDE="0"), dict(ALSEP_TDF_WIDE="8"), dict(ALSEP_TDF_RPF="0")],
                         ids=["kuielab-2048", "wide0", "wide8", "rpf0"])
def test_fallbacks_stay_where_they_were(tmp_path, case):
    """M = 2048 is no multiple of 192; ALSEP_TDF_WIDE=0: 128-row kernel; =8: 384-row workgroups; ALSEP_TDF_RPF=0: the timing-comparison
    instance -- none of them reaches the new instance, and the switch changes nothing"""
    case = dict(case)
    dim_f = case.pop("dim_f", 3072)
    base, cb = run(tmp_path, "foff", dim_f=dim_f, ALSEP_TDF_PERSIST="0", **case)
    got, cg = run(tmp_path, "fon", dim_f=dim_f, ALSEP_TDF_PERSIST="1", **case)
    print("counts off", cb, "on", cg)
    assert np.isfinite(base).all() and np.abs(base).max() > 1e-3
    assert cb["tdf_bf16_persist_kernel"] == 0 and cg["tdf_bf16_persist_kernel"] == 0, (cb, cg)
    assert cb == cg, (cb, cg)
    assert np.array_equal(base, got), f"max diff {np.abs(base - got).max()}"
