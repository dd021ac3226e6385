"""HTDemucs' half-precision mode restated on the CPU (torch): oracle.htdemucs_oracle's forward with the rounding points of
``HTDemucs(precision="f16")``, without editing the oracle.  Every convolution, transposed convolution and Linear reads
its input and weights rounded to IEEE half and accumulates in float32 (bias after the product, float32); the attention reads q, k, v as
half (q scaled by d^-1/2 log2 e before its rounding, as the kernel folds it), rounds exp(s - max) to half for P V and divides by the
float32 row sum.  Everything else -- norms, GELU / GLU, residuals, STFT / iSTFT -- is the float32 oracle's."""
from __future__ import annotations

import contextlib

import types

import torch
import torch.nn.functional as F

from oracle import htdemucs_oracle as ho


def _h(t: torch.Tensor) -> torch.Tensor:
    return t.half().float()


def _half_functional() -> types.SimpleNamespace:
    ns = types.SimpleNamespace(**{k: getattr(F, k) for k in dir(F) if not k.startswith("__")})
    ns.conv1d = lambda x, w, b=None, **kw: F.conv1d(_h(x), _h(w), b, **kw)
    ns.conv2d = lambda x, w, b=None, **kw: F.conv2d(_h(x), _h(w), b, **kw)
    ns.conv_transpose1d = lambda x, w, b=None, **kw: F.conv_transpose1d(_h(x), _h(w), b, **kw)
    ns.conv_transpose2d = lambda x, w, b=None, **kw: F.conv_transpose2d(_h(x), _h(w), b, **kw)
    ns.linear = lambda x, w, b=None: F.linear(_h(x), _h(w), b)
    return ns


def _mha_half(w, p: str, q: torch.Tensor, kv: torch.Tensor, heads: int) -> torch.Tensor:
    """nn.MultiheadAttention (see ho._mha) with the half-precision kernel's rounding points"""
    c = q.shape[-1]
    wi, bi = w[p + ".in_proj_weight"], w[p + ".in_proj_bias"]
    qq = _h(F.linear(_h(q), _h(wi[:c]), bi[:c]))                       # projections stored as half
    kk = _h(F.linear(_h(kv), _h(wi[c:2 * c]), bi[c:2 * c]))
    vv = _h(F.linear(_h(kv), _h(wi[2 * c:]), bi[2 * c:]))
    b, tq, _ = qq.shape
    tk = kk.shape[1]
    dh = c // heads
    qh = _h(qq.view(b, tq, heads, dh).transpose(1, 2) * (dh ** -0.5 * 1.4426950408889634))
    kh = kk.view(b, tk, heads, dh).transpose(1, 2)
    vh = vv.view(b, tk, heads, dh).transpose(1, 2)
    s2 = qh @ kh.transpose(-1, -2)                                     # base-2 exponents
    e = torch.exp2(s2 - s2.amax(dim=-1, keepdim=True))
    out = (_h(e) @ vh) / e.sum(-1, keepdim=True)
    out = _h(out.transpose(1, 2).reshape(b, tq, c))
    return F.linear(out, _h(w[p + ".out_proj.weight"]), w[p + ".out_proj.bias"])


@contextlib.contextmanager
def _half_mode():
    saved = ho.F, ho._mha
    ho.F, ho._mha = _half_functional(), _mha_half
    try:
        yield
    finally:
        ho.F, ho._mha = saved


@torch.no_grad()
def forward(cfg: ho.HTDemucsConfig, w, mix: torch.Tensor) -> torch.Tensor:
    """ho.forward with the half-precision rounding points: mix [B, 2, L] -> [B, S, 2, L]"""
    with _half_mode():
        return ho.forward(cfg, w, mix)


def half_forward(cfg: ho.HTDemucsConfig, w):
    """a ``fwd`` for ho.separate / ho.apply_model"""
    return lambda x: forward(cfg, w, x)


def rel(a, b) -> float:
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).norm() / b.norm())



