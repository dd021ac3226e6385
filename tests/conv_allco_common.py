"""Shared by test_emul_conv_allco.py and test_gpu_conv_allco.py: one forward of a one-block network per weight kind in a fresh process
(the routing switches are read once per process), returning outputs and launch counts.

Network: TDFNetConfig(dim_f=192, dim_t=16, g=c, num_blocks=1, n_fft=384, hop=256), batch 3: three 3x3 convs at c channels on 16 x 192
pixels.  conv3x3_bf16_allco_kernel's 8 x 48 tiles: two tile rows (top border, bottom border, one seam), four tile columns, 24 tiles,
three input chunks of 48 (an odd number: the patch buffer parity flips from tile to tile); a grid capped at 5 gives four workgroups
five tiles and one four (ring start-up, steady state, a partial last round).  Only c = 144 has an instance of the kernel: at c = 192
it needs scratch memory and is not built."""
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = "conv3x3_bf16_allco_kernel"
PINNED = ("conv3x3_bf16_kernel<64>", "conv3x3_bf16_kernel", "conv3x3_bf16_kernel<small>", "conv3x3_bf16_big_kernel",
          "conv3x3_bf16_big_kernel<3>", "tdf_bf16_kernel")
BATCH = 3
OFF = {"ALSEP_CONV_ALLCO": "0", "ALSEP_CONV_BIG": "2"}
ON = {"ALSEP_CONV_ALLCO": "2", "ALSEP_CONV_BIG": "2"}
DT = {"bf16": torch.bfloat16, "f16": torch.float16}

# argv: out.pt  device ("cuda" or the path of the emulation library)  dtype  c
SCRIPT = r"""
import os, sys, torch
sys.path.insert(0, %(root)r)
from audiolab_amd import _lib
if sys.argv[2] != "cuda":
    _lib._LIB = _lib.bind(sys.argv[2]); _lib.DEVICE_TYPE = "cpu"
from audiolab_amd.synth import synthetic_state_dict
from audiolab_amd.tdfnet import TDFNet, TDFNetConfig
from oracle.tdfnet_structured import integer_input, structured_state_dict
dev = "cuda:0" if sys.argv[2] == "cuda" else "cpu"
dt = {"bf16": torch.bfloat16, "f16": torch.float16}[sys.argv[3]]
cfg = TDFNetConfig(dim_f=192, dim_t=16, g=int(sys.argv[4]), num_blocks=1, n_fft=384, hop=256)
ctx = _lib.Context(dev)
res = {}
for kind in ("random", "shift"):
    if kind == "random":
        sd = synthetic_state_dict(cfg, seed=1, calib_frames=8)
        x = torch.randn((%(batch)d, cfg.dim_t, cfg.dim_f, 4), generator=torch.Generator().manual_seed(100)) * 4
    else:
        sd = structured_state_dict(cfg, None, final="dyadic", shift=True)
        x = integer_input(cfg, %(batch)d, seed=5).permute(0, 3, 2, 1).contiguous()
    net = TDFNet(cfg, sd, ctx=ctx, dtype=dt, max_batch=%(batch)d)
    x = x.to(dt).to(dev)
    ctx.launch_counts_reset()
    first = net.forward_nhwc(x).float().cpu()
    counts = {k: ctx.launch_count(k) for k in %(names)r}
    again = net.forward_nhwc(x).float().cpu() if dev != "cpu" else first      # the emulation is synchronous: nothing to race
    res[kind] = (first, again, counts)
    del net
torch.save(res, sys.argv[1])
"""


def run(device, tmp_path, tag, dtype, c, env, timeout):
    """-> {"random" | "shift": (output [B,T,F,4] float32, the same forward once more, launch counts of the first)}"""
    path = str(tmp_path / f"{tag}.pt")
    r = subprocess.run([sys.executable, "-c", SCRIPT % {"root": ROOT, "batch": BATCH, "names": PINNED + (NEW,)}, path, device, dtype, str(c)],
                       env=dict(os.environ, **env), capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    return torch.load(path)


_ORACLE = {}


def shift_oracle(dtype, c):
    """the storage oracle of the shifting all-passthrough network on the integer input, as [B,T,F,4]; computed once per (dtype, c)"""
    if (dtype, c) not in _ORACLE:
        from audiolab_amd.tdfnet import TDFNetConfig
        from oracle import tdfnet_oracle
        from oracle.tdfnet_structured import integer_input, structured_state_dict
        cfg = TDFNetConfig(dim_f=192, dim_t=16, g=c, num_blocks=1, n_fft=384, hop=256)
        sd = structured_state_dict(cfg, None, final="dyadic", shift=True)
        with torch.no_grad():
            want = tdfnet_oracle.forward(sd, integer_input(cfg, BATCH, seed=5), cfg.num_blocks, cfg.l, cfg.bn, storage=DT[dtype])
        _ORACLE[dtype, c] = want.float().permute(0, 3, 2, 1).contiguous()
    return _ORACLE[dtype, c]


def check(off, on, what, dtype, c):
    """the forced run against the reference run: same bits, the new name 3 / 0, the pinned names equal; the shifting network also
    against the oracle"""
    for kind in ("random", "shift"):
        base, base2, cb = off[kind]
        got, got2, cg = on[kind]
        w = f"{what}, {kind} weights"
        assert torch.isfinite(base).all() and float(base.abs().max()) > 1e-3, w
        assert cb[NEW] == 0 and cg[NEW] == 3, (w, cb, cg)
        assert {k: cg[k] for k in PINNED} == {k: cb[k] for k in PINNED}, (w, cb, cg)      # the pinned names count layer launches
        assert cb["conv3x3_bf16_big_kernel<3>"] == 3 and cb["conv3x3_bf16_kernel<64>"] == 0, (w, cb)      # the kernel it replaces
        assert torch.equal(base, base2), w
        assert torch.equal(got, got2), f"{w}: two forwards differ by {(got - got2).abs().max()}"
        assert torch.equal(base, got), f"{w}: max diff {(base - got).abs().max()} (peak {base.abs().max()})"
    want = shift_oracle(dtype, c)
    assert float((want != 0).double().mean()) > 0.3
    assert torch.equal(on["shift"][0], want), (what, float((on["shift"][0] - want).abs().max()))
