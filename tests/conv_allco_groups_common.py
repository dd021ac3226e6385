"""Shared by test_emul_conv_allco_groups.py and test_gpu_conv_allco_groups.py: conv3x3_bf16_allco_kernel in output groups of 96 channels
(c = 192: two groups, four input chunks; c = 288: three groups, six chunks) against the plain kernel, on the one-block network of
conv_allco_common.SCRIPT (16 x 192 pixels, batch 3, three 3x3 convs, one process per environment).

Tiles of 8 x 48: two tile rows (top border, bottom border, one seam) x four tile columns (left border, two interior, right border),
24 tiles; 8 x 64: three columns, 18 tiles.  A work item is (tile, group), a workgroup takes the groups of a tile back to back: with the
grid capped at 5 a workgroup runs 4 or 5 tiles = 8 to 15 items (ring start-up, steady state, the hand-over from a tile's last group to
the next tile's first, a partial last round); uncapped it runs the groups of one tile.  An even chunk count keeps a tile's first patch in
buffer 0; the odd one of the c = 144 tests is in test_*_conv_allco.py."""
import os
import subprocess
import sys

import torch

from conv_allco_common import BATCH, NEW, PINNED, ROOT, SCRIPT, shift_oracle

INST = {48: "conv3x3_bf16_allco_kernel<6,48>", 64: "conv3x3_bf16_allco_kernel<6,64>"}
NAMES = PINNED + (NEW,) + tuple(INST.values())
CASES = [(192, 48), (192, 64), (288, 48), (288, 64)]
SWITCHES = ("ALSEP_CONV_ALLCO", "ALSEP_CONV_ALLCO_TW", "ALSEP_CONV_ALLCO_GRID", "ALSEP_CONV_BIG")
OFF = {"ALSEP_CONV_ALLCO": "0", "ALSEP_CONV_BIG": "2"}
# run_conv_dma's defaults (kConvAllcoRouted, kConvAllcoTw): is c = 192 routed to the kernel without ALSEP_CONV_ALLCO, and at which width
ROUTED_192 = True
DEFAULT_TW = 64


def on_env(tw, grid):
    env = {"ALSEP_CONV_ALLCO": "2", "ALSEP_CONV_BIG": "2", "ALSEP_CONV_ALLCO_TW": str(tw)}
    if grid:
        env["ALSEP_CONV_ALLCO_GRID"] = str(grid)
    return env


def run(device, tmp_path, tag, dtype, c, env, timeout):
    """conv_allco_common.run with the instance names counted too, and with only the switches of env set
    -> {"random" | "shift": (output [B,T,F,4] float32, the same forward once more, launch counts of the first)}"""
    path = str(tmp_path / f"{tag}.pt")
    base = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    r = subprocess.run([sys.executable, "-c", SCRIPT % {"root": ROOT, "batch": BATCH, "names": NAMES}, path, device, dtype, str(c)],
                       env=dict(base, **env), capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    return torch.load(path)


_OFF = {}


def off_run(device, tmp_path, dtype, c, timeout):
    """the plain kernel's run, made once per (device, dtype, c) and shared by the cases"""
    if (device, dtype, c) not in _OFF:
        _OFF[device, dtype, c] = run(device, tmp_path, "off", dtype, c, OFF, timeout)
    return _OFF[device, dtype, c]


def check(off, on, what, dtype, c, tw, routed=True):
    """a run against the plain kernel's: same bits (also forward against forward, and the shifting network against the oracle); the
    kernel's names 3 where it is routed and 0 where not, the pinned names the same either way"""
    for kind in ("random", "shift"):
        base, base2, cb = off[kind]
        got, got2, cg = on[kind]
        w = f"{what}, {kind} weights"
        assert torch.isfinite(base).all() and float(base.abs().max()) > 1e-3, w
        assert cb[NEW] == 0 and cb[INST[48]] == 0 and cb[INST[64]] == 0, (w, cb)
        assert cg[NEW] == (3 if routed else 0) and cg[INST[tw]] == (3 if routed else 0) and cg[INST[112 - tw]] == 0, (w, cg)
        assert {k: cg[k] for k in PINNED} == {k: cb[k] for k in PINNED}, (w, cb, cg)      # the pinned names count layer launches
        assert cb["conv3x3_bf16_kernel<64>"] == 3, (w, cb)                                # the kernel it replaces
        assert torch.equal(base, base2), w
        assert torch.equal(got, got2), f"{w}: two forwards differ by {(got - got2).abs().max()}"
        assert torch.equal(base, got), f"{w}: max diff {(base - got).abs().max()} (peak {base.abs().max()})"
    want = shift_oracle(dtype, c)
    assert float((want != 0).double().mean()) > 0.3
    assert torch.equal(on["shift"][0], want), (what, float((on["shift"][0] - want).abs().max()))
