"""Shared by test_emul_tdf_fused.py and test_gpu_tdf_fused.py: forwards of small networks in a fresh process per environment (the
routing switches are read once per process), returning outputs and launch counts.

tdf_bf16_fused_kernel runs both TDF linears of a block in one launch where F = 768 (one unit of 48 channels per work item) or
F = 384 (two units per item); ALSEP_TDF_FUSED=0 is the pair of tdf_bf16_kernel launches it replaces, =2 forces every shape an
instance serves.  Shapes are the smallest that reach every branch:
  L2    one block at F = 768, c = 144, T = 4, batch 3: 36 items (the channel group of an item cycles through 0, 48, 96)
  L3    one block at F = 384, c = 192, T = 4, batch 3: 48 units = 24 items
  DEEP  seven blocks from F = 3072, c = 48, T = 8: level 2 (T = 2, 18 items) in the encoder and the decoder, level 3 (T = 1, 12 units)
        at the bottleneck; levels 0 and 1 stay on the wide / persistent kernels
with the grid uncapped (one item per workgroup) and capped at 5 (several items per workgroup, the tile buffer parity flipping, a
partial last round)."""
import json
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = "tdf_bf16_fused_kernel"
PINNED = ("tdf_bf16_kernel", "tdf_bf16_wide_kernel<res>", "tdf_bf16_wide_kernel<nores>", "tdf_bf16_wide_kernel<res,final>",
          "tdf_bf16_persist_kernel", "tdf_gemm_kernel", "final_conv_kernel", "conv3x3_bf16_kernel", "conv3x3_bf16_big_kernel<3>")
BATCH = 3
OFF = {"ALSEP_TDF_FUSED": "0"}
ON = {"ALSEP_TDF_FUSED": "2"}
DT = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
L2 = dict(dim_f=768, dim_t=4, g=144, num_blocks=1, n_fft=1536, hop=256, bn=8)
L3 = dict(dim_f=384, dim_t=4, g=192, num_blocks=1, n_fft=768, hop=256, bn=8)
DEEP = dict(dim_f=3072, dim_t=8, g=48, num_blocks=7, bn=8)

# argv: out.pt  device ("cuda" or the path of the emulation library)  dtype  config (json)  batch  kinds (comma separated)
SCRIPT = r"""
import json, os, sys, torch
sys.path.insert(0, %(root)r)
from audiolab_amd import _lib
if sys.argv[2] != "cuda":
    _lib._LIB = _lib.bind(sys.argv[2]); _lib.DEVICE_TYPE = "cpu"
from audiolab_amd.synth import synthetic_state_dict
from audiolab_amd.tdfnet import TDFNet, TDFNetConfig
from oracle.tdfnet_structured import integer_input, structured_state_dict
dev = "cuda:0" if sys.argv[2] == "cuda" else "cpu"
dt = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}[sys.argv[3]]
cfg = TDFNetConfig(**json.loads(sys.argv[4]))
batch = int(sys.argv[5])
ctx = _lib.Context(dev)
res = {}
for kind in sys.argv[6].split(","):
    if kind == "random":
        sd = synthetic_state_dict(cfg, seed=1, calib_frames=8)
        x = torch.randn((batch, cfg.dim_t, cfg.dim_f, 4), generator=torch.Generator().manual_seed(100)) * 4
    else:
        sd = structured_state_dict(cfg, None, final="dyadic", shift=True)
        x = integer_input(cfg, batch, seed=5).permute(0, 3, 2, 1).contiguous()
    net = TDFNet(cfg, sd, ctx=ctx, dtype=dt, max_batch=batch)
    x = x.to(dt).to(dev)
    ctx.launch_counts_reset()
    first = net.forward_nhwc(x).float().cpu()
    counts = {k: ctx.launch_count(k) for k in %(names)r}
    again = net.forward_nhwc(x).float().cpu() if dev != "cpu" else first      # the emulation is synchronous: nothing to race
    res[kind] = (first, again, counts)
    del net
torch.save(res, sys.argv[1])
"""


def run(device, tmp_path, tag, dtype, cfg, env, timeout, kinds="random,shift", batch=BATCH):
    """-> {kind: (output [B,T,F,4] float32, the same forward once more, launch counts of the first)}"""
    path = str(tmp_path / f"{tag}.pt")
    clean = {k: v for k, v in os.environ.items() if not k.startswith("ALSEP_TDF_FUSED")}
    r = subprocess.run([sys.executable, "-c", SCRIPT % {"root": ROOT, "names": PINNED + (NEW,)}, path, device, dtype, json.dumps(cfg),
                        str(batch), kinds], env=dict(clean, **env), capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    return torch.load(path)


_ORACLE = {}


def shift_oracle(dtype, cfg):
    """the storage oracle of the shifting all-passthrough network on the integer input, as [B,T,F,4]; computed once per (dtype, shape)"""
    key = (dtype, json.dumps(cfg, sort_keys=True))
    if key not in _ORACLE:
        from audiolab_amd.tdfnet import TDFNetConfig
        from oracle import tdfnet_oracle
        from oracle.tdfnet_structured import integer_input, structured_state_dict
        c = TDFNetConfig(**cfg)
        sd = structured_state_dict(c, None, final="dyadic", shift=True)
        with torch.no_grad():
            want = tdfnet_oracle.forward(sd, integer_input(c, BATCH, seed=5), c.num_blocks, c.l, c.bn, storage=DT[dtype])
        _ORACLE[key] = want.float().permute(0, 3, 2, 1).contiguous()
    return _ORACLE[key]


def check(off, on, what, launches):
    """a run against the reference run (ALSEP_TDF_FUSED=0): the same bits, the new name `launches` times / never, every pinned name
    the same number of times; every forward equal to its repetition"""
    for kind in off:
        base, base2, cb = off[kind]
        got, got2, cg = on[kind]
        w = f"{what}, {kind} weights"
        print(w, "fused launches", cb[NEW], cg[NEW], "peak", float(base.abs().max()), "max diff", float((base - got).abs().max()))
        assert torch.isfinite(base).all() and float(base.abs().max()) > 1e-3, w
        assert cb[NEW] == 0 and cg[NEW] == launches, (w, cb, cg)
        assert {k: cg[k] for k in PINNED} == {k: cb[k] for k in PINNED}, (w, cb, cg)      # the pinned names count layer launches
        assert torch.equal(base, base2), w
        assert torch.equal(got, got2), f"{w}: two forwards differ by {(got - got2).abs().max()}"
        assert torch.equal(base, got), f"{w}: max diff {(base - got).abs().max()} (peak {base.abs().max()})"


def check_oracle(on, dtype, cfg, what):
    want = shift_oracle(dtype, cfg)
    assert float((want != 0).double().mean()) > 0.3
    assert torch.equal(on["shift"][0], want), (what, float((on["shift"][0] - want).abs().max()))
