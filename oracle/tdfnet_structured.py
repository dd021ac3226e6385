"""Structured-weight TFC-TDF U-Nets: one layer computes, every other layer passes its input through exactly.

TEST INFRASTRUCTURE -- see ``oracle/__init__.py``.  Not imported by the product.

A full-size network with random weights everywhere amplifies one flipped half-precision rounding about 100x over its
40 layers, so its end-to-end bounds cannot see a small error in one kernel.  ``structured_state_dict`` builds a
``state_dict`` for a whole ``TDFNetConfig`` in which every layer except one TARGET is an exact passthrough: the kernel
output of such a layer is bit-identical to the storage oracle's (``tdfnet_oracle.forward(storage=...)``), so a GPU
forward differs from the oracle only where the target layer (and the final 1x1 projection) sum in another order.
The target runs at its real place in the production network, with its real dispatch.

Passthrough layers carry no BatchNorm entries (``fold_batchnorm`` then gives scale 1 and shift 0 exactly, and the
oracle's ``_bn`` is the identity) and no biases:

- first conv (4 -> g): channel 2i = +x[i mod 4], channel 2i+1 = -x[i mod 4] (the ReLU keeps one of the two);
- 3x3 convs: identity centre tap (``shift=True``: one off-centre tap, a shift by one frame / bin);
- TDF: both linears zero, so the block output is x + relu(0) = x;
- ds (2x2 / 2, c -> c+g): channels < c take tap (0,0); the g new channels take tap (1,1) of channel i - c;
- us (c+g -> c): out channel i = in i + in (i+c) where that exists, on all four taps -- every channel of a deeper
  level reaches level 0;
- final conv: ``final="random"`` a positive random fp32 projection (no cancellation, so a relative error of the
  network output is one of its inputs); ``final="dyadic"`` +-2^-5 weights, exact on integer data (``integer_input``).

The target has random weights ``(N(0,1) + mu) / (mu * fan_in)``, mu = max(0.5, 8 / sqrt(fan_in)): every activation it reads is a ReLU output (>= 0), so
the pre-activation is positive except with probability Phi(-mu sqrt(fan_in) E x / rms x); a small positive bias
covers all-zero receptive fields.  The ReLU therefore hides almost nothing, and the output keeps the input's scale.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch

KINDS = ("conv", "tdf", "ds", "us")
MU = 0.5                   # mean of the target weights in units of their standard deviation
TARGET_BIAS = 2.0 ** -6


def block_name(cfg, k: int) -> str:
    """the encoder block at level k (k < n), the bottleneck at k = n"""
    return "bottleneck_block" if k == cfg.n else f"encoding_blocks.{k}"


def target_layer(cfg, target: Tuple[str, int]) -> str:
    """the oracle's name (``tdfnet_oracle.forward(perturb=...)``) of the target's stored output:
    conv -> the block's first 3x3 conv; tdf -> the block output (second linear + residual); ds k -> k+1; us k+1 -> k"""
    kind, k = target
    if kind == "conv":
        return f"{block_name(cfg, k)}.tfc.0"
    if kind == "tdf":
        return f"{block_name(cfg, k)}.tdf.1"
    if kind == "ds":
        return f"ds.{k}"
    return f"us.{cfg.n - 1 - k}"


def _rand(gen: torch.Generator, shape, fan_in: int) -> torch.Tensor:
    mu = max(MU, 8.0 / fan_in ** 0.5)                # narrow layers (TDF hidden width 12 at the bottleneck): a larger mean
    return (torch.randn(shape, generator=gen) + mu) / (mu * fan_in)


SHIFT_TAPS = ((0, 1), (1, 0), (2, 2))       # shift=True: the passthrough 3x3 convs of a block move the data by one frame, one bin, one of each


def structured_state_dict(cfg, target: Optional[Tuple[str, int]] = None, seed: int = 0, final: str = "random",
                          sel_scale: float = 1.0, shift: bool = False) -> Dict[str, torch.Tensor]:
    """``target``: None (all passthrough) or (kind, level) with kind in KINDS; conv / tdf at level 0..n (n = bottleneck),
    ds at k -> k+1 for k < n, us at k+1 -> k for k < n.  ``sel_scale`` (a power of two) scales the first conv's
    selection, to keep the skip products of a deep network inside the f16 range.  ``shift``: the passthrough 3x3 convs
    take one off-centre tap each (SHIFT_TAPS) instead of the centre one, so that their output rows and columns at a
    tile edge come from the halo and the zero padding -- still exact (one product per output)."""
    if cfg.bn is None or cfg.bn == 0 or cfg.k != 3:
        raise ValueError("structured networks: k = 3 and two TDF linears (bn > 0) only")
    if target is not None:
        kind, k = target
        if kind not in KINDS or not 0 <= k <= cfg.n or (kind in ("ds", "us") and k == cfg.n):
            raise ValueError(f"no layer {target} in a network of {cfg.num_blocks} blocks")
    gen = torch.Generator().manual_seed(seed)
    g, n = cfg.g, cfg.n
    sd: Dict[str, torch.Tensor] = {}

    w = torch.zeros(g, 4, 1, 1)
    for i in range(g // 2):
        w[2 * i, i % 4] = sel_scale
        w[2 * i + 1, i % 4] = -sel_scale
    sd["first_conv.0.weight"] = w

    def block(p: str, c: int, f: int, level: int):
        hit = target is not None and target[1] == level and p == block_name(cfg, level)
        for j in range(cfg.l):
            q = f"{p}.tfc.H.{j}.0"
            if hit and target[0] == "conv" and j == 0:
                sd[q + ".weight"] = _rand(gen, (c, c, 3, 3), 9 * c)
                sd[q + ".bias"] = torch.full((c,), TARGET_BIAS)
            else:
                tap = torch.zeros(3, 3)
                tap[SHIFT_TAPS[j % 3] if shift else (1, 1)] = 1.0
                sd[q + ".weight"] = torch.eye(c)[:, :, None, None] * tap
        h = f // cfg.bn
        if hit and target[0] == "tdf":
            sd[f"{p}.tdf.0.weight"] = _rand(gen, (h, f), f)
            sd[f"{p}.tdf.0.bias"] = torch.full((h,), TARGET_BIAS)
            sd[f"{p}.tdf.3.weight"] = _rand(gen, (f, h), h)
            sd[f"{p}.tdf.3.bias"] = torch.full((f,), TARGET_BIAS)
        else:
            sd[f"{p}.tdf.0.weight"] = torch.zeros(h, f)
            sd[f"{p}.tdf.3.weight"] = torch.zeros(f, h)

    levels = cfg.levels()
    for i in range(n):
        c, _, f = levels[i]
        block(f"encoding_blocks.{i}", c, f, i)
        if target == ("ds", i):
            sd[f"ds.{i}.0.weight"] = _rand(gen, (c + g, c, 2, 2), 4 * c)
            sd[f"ds.{i}.0.bias"] = torch.full((c + g,), TARGET_BIAS)
        else:
            w = torch.zeros(c + g, c, 2, 2)
            for o in range(c):
                w[o, o, 0, 0] = 1.0
            for o in range(g):
                w[c + o, o, 1, 1] = 1.0
            sd[f"ds.{i}.0.weight"] = w
        # us.i and decoding_blocks.i run at level n-i-1; ConvTranspose2d weight [in = c_(k+1), out = c_k, 2, 2]
        k = n - 1 - i
        ck, _, fk = levels[k]
        block(f"decoding_blocks.{i}", ck, fk, -1)
        if target == ("us", k):
            sd[f"us.{i}.0.weight"] = _rand(gen, (ck + g, ck, 2, 2), ck + g)
            sd[f"us.{i}.0.bias"] = torch.full((ck,), TARGET_BIAS)
        else:
            w = torch.zeros(ck + g, ck, 2, 2)
            for o in range(ck):
                w[o, o] = 1.0
                if o + ck < ck + g:
                    w[o + ck, o] = 1.0
            sd[f"us.{i}.0.weight"] = w
    c, _, f = levels[n]
    block("bottleneck_block", c, f, n)

    if final == "random":
        sd["final_conv.0.weight"] = (0.5 + torch.rand(4, g, 1, 1, generator=gen)) / g
    elif final == "dyadic":
        sd["final_conv.0.weight"] = torch.where(torch.rand(4, g, 1, 1, generator=gen) < 0.5, -1.0, 1.0) * 2.0 ** -5
    else:
        raise ValueError(f"final={final!r}: 'random' or 'dyadic'")
    return sd


def integer_input(cfg, batch: int, seed: int = 0, amp: int = 3) -> torch.Tensor:
    """[B,4,dim_f,dim_t] of integers in [-amp, amp].  Through an all-passthrough network every value stays an integer
    (sums and skip products; at the bench depth |x| <= amp (2 amp)^5 < 2^24), so every sum is exact in fp32 in any
    order, the storage roundings are the same on both sides, and with ``final="dyadic"`` the output is exact too:
    the GPU forward must be bit-identical to the oracle's."""
    gen = torch.Generator().manual_seed(seed)
    return torch.randint(-amp, amp + 1, (batch, 4, cfg.dim_f, cfg.dim_t), generator=gen).float()
