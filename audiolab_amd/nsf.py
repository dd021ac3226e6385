"""RVC's NSF-HiFiGAN vocoder on the GPU: ``GeneratorNSF`` of the reference (modules/rvc/infer/lib/infer_pack/models.py:449-566), the decoder
``self.dec`` of Clone's synthesizer, with the reference's ``forward(x, f0, g, n_res)`` surface.

  1. the sine source (models.py:313-446): per-frame phase steps summed in float64, ``har = tanh(w (0.1 sin(2 pi rad) uv + amp noise) + b)``;
     the standard-normal ``noise`` is an explicit input (drawn from a ``torch.Generator`` on the device when the caller gives none), so
     that the network is a function;
  2. ``conv_pre`` (192 -> 512, 7 taps) with the speaker conditioning ``cond(g)`` folded into its bias on the device;
  3. per upsampling stage: LeakyReLU(0.1), ``ConvTranspose1d`` and the stage's noise convolution of the source in one kernel, then the
     ResBlock1s, one kernel launch per convolution: the LeakyReLU in front, the residual, the running sum over the resblocks and their
     mean all inside it;
  4. LeakyReLU(0.01), ``conv_post`` (C -> 1), tanh.

Float32, batch 1, channels-last ``[L, C]`` on the device (csrc/nsf.h).  Not built: ``resblock = "2"``, ``n_res`` interpolation, half
precision, the ``_nono`` generators without f0.  The text encoder, the flow, HuBERT and the ``Clone`` wrapper are not here either.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import AlsepError, Context

LRELU_SLOPE = 0.1
MAX_FRAMES = 1 << 20                                                          # kNsfMaxFrames of csrc/nsf.h
MAX_UPP = 1024
MAX_PHASE_TAPS = 8                                                            # kNsfMaxPhaseTaps
SR_NAMES = {"32k": 32000, "40k": 40000, "48k": 48000}


@dataclass(frozen=True)
class NSFConfig:
    """the constructor arguments of the reference's ``GeneratorNSF``; the default is RVC v2 at 40 kHz"""
    initial_channel: int = 192
    resblock: str = "1"
    resblock_kernel_sizes: Tuple[int, ...] = (3, 7, 11)
    resblock_dilation_sizes: Tuple[Tuple[int, ...], ...] = ((1, 3, 5), (1, 3, 5), (1, 3, 5))
    upsample_rates: Tuple[int, ...] = (10, 10, 2, 2)
    upsample_initial_channel: int = 512
    upsample_kernel_sizes: Tuple[int, ...] = (16, 16, 4, 4)
    gin_channels: int = 256
    sr: int = 40000

    @property
    def upp(self) -> int:
        return int(math.prod(self.upsample_rates))

    def stage_channels(self, i: int) -> int:
        return self.upsample_initial_channel >> (i + 1)

    def source_stride(self, i: int) -> int:
        return int(math.prod(self.upsample_rates[i + 1:]))

    @classmethod
    def from_rvc(cls, config_list: Sequence) -> "NSFConfig":
        """the positional ``cpt["config"]`` of an RVC checkpoint, in the argument order of ``SynthesizerTrnMs256NSFsid.__init__``:
        spec_channels, segment_size, inter_channels, hidden_channels, filter_channels, n_heads, n_layers, kernel_size, p_dropout, resblock,
        resblock_kernel_sizes, resblock_dilation_sizes, upsample_rates, upsample_initial_channel, upsample_kernel_sizes, spk_embed_dim,
        gin_channels, sr"""
        c = list(config_list)
        if len(c) < 18:
            raise AlsepError(f"nsf: a checkpoint configuration of {len(c)} entries (18 are needed)")
        sr = c[17]
        if isinstance(sr, str):
            if sr not in SR_NAMES:
                raise AlsepError(f"nsf: sample rate {sr!r} (one of {sorted(SR_NAMES)})")
            sr = SR_NAMES[sr]
        return cls(initial_channel=int(c[2]), resblock=str(c[9]), resblock_kernel_sizes=tuple(int(v) for v in c[10]),
                   resblock_dilation_sizes=tuple(tuple(int(v) for v in d) for d in c[11]), upsample_rates=tuple(int(v) for v in c[12]),
                   upsample_initial_channel=int(c[13]), upsample_kernel_sizes=tuple(int(v) for v in c[14]), gin_channels=int(c[16]), sr=int(sr))

    def check(self) -> None:
        if str(self.resblock) != "1":
            raise AlsepError(f"nsf: resblock = {self.resblock!r} not built (ResBlock1 only)")
        if len(self.upsample_rates) < 1 or len(self.upsample_rates) != len(self.upsample_kernel_sizes):
            raise AlsepError(f"nsf: upsample_rates {self.upsample_rates} and upsample_kernel_sizes {self.upsample_kernel_sizes} do not pair up")
        if len(self.resblock_kernel_sizes) < 1 or len(self.resblock_kernel_sizes) != len(self.resblock_dilation_sizes):
            raise AlsepError(f"nsf: resblock_kernel_sizes {self.resblock_kernel_sizes} and resblock_dilation_sizes "
                             f"{self.resblock_dilation_sizes} do not pair up")
        if self.initial_channel < 8 or self.initial_channel % 8:
            raise AlsepError(f"nsf: initial_channel = {self.initial_channel} not built (channels in eights)")
        if self.gin_channels < 0:
            raise AlsepError(f"nsf: gin_channels = {self.gin_channels}")
        if self.sr < 1:
            raise AlsepError(f"nsf: sr = {self.sr}")
        n = len(self.upsample_rates)
        if self.upsample_initial_channel % (1 << n) or self.stage_channels(n - 1) % 8 or self.stage_channels(n - 1) < 8:
            raise AlsepError(f"nsf: upsample_initial_channel = {self.upsample_initial_channel} over {n} stages leaves "
                             f"{self.upsample_initial_channel / (1 << n):g} channels (not built: channels in eights)")
        for k, dil in zip(self.resblock_kernel_sizes, self.resblock_dilation_sizes):
            if k < 1 or k > 11 or k % 2 == 0:
                raise AlsepError(f"nsf: resblock kernel size {k} not built (odd, 1 .. 11)")
            if len(dil) != 3:
                raise AlsepError(f"nsf: resblock dilations {tuple(dil)} not built (ResBlock1 has three)")
            for d in dil:
                if d < 1 or d > 5:
                    raise AlsepError(f"nsf: resblock dilation {d} not built (1 .. 5)")
        for i, (u, k) in enumerate(zip(self.upsample_rates, self.upsample_kernel_sizes)):
            if u < 1 or u > 64 or k < u or (k - u) % 2:
                raise AlsepError(f"nsf: upsampling kernel {k} at rate {u} not built (rate 1 .. 64, kernel >= rate and kernel - rate even: "
                                 f"otherwise the stage's length is not rate times its input's)")
            if k > MAX_PHASE_TAPS * u:
                raise AlsepError(f"nsf: upsampling kernel {k} at rate {u} not built (the kernel walks at most {MAX_PHASE_TAPS} taps per "
                                 f"output phase: kernel <= {MAX_PHASE_TAPS} rate)")
            s = self.source_stride(i)
            if s > 1 and s % 2:
                raise AlsepError(f"nsf: source stride {s} after stage {i} not built (even or 1: an odd stride's noise convolution is one "
                                 f"sample short)")
        if self.upp > MAX_UPP:
            raise AlsepError(f"nsf: {self.upp} samples a frame not built (at most {MAX_UPP})")


V2_40K = NSFConfig()


# ---- the state dict of GeneratorNSF --------------------------------------------------------------------------------------------------------
def _wn_shapes(out: Dict[str, tuple], p: str, shape: tuple) -> None:
    """a weight-normed layer: bias, weight_g (the first axis, the others 1), weight_v"""
    bias = shape[1] if p.startswith("ups.") else shape[0]                     # ConvTranspose1d's weight is [Cin, Cout, K]
    out[f"{p}.bias"] = (bias,)
    out[f"{p}.weight_g"] = (shape[0], 1, 1)
    out[f"{p}.weight_v"] = tuple(shape)


def param_shapes(cfg: NSFConfig = V2_40K) -> Dict[str, tuple]:
    """name -> shape of every tensor of ``GeneratorNSF(...).state_dict()``, in its order"""
    cfg.check()
    out: Dict[str, tuple] = {}
    out["m_source.l_linear.weight"] = (1, 1)
    out["m_source.l_linear.bias"] = (1,)
    n = len(cfg.upsample_rates)
    for i in range(n):
        s = cfg.source_stride(i)
        out[f"noise_convs.{i}.weight"] = (cfg.stage_channels(i), 1, 2 * s if i + 1 < n else 1)
        out[f"noise_convs.{i}.bias"] = (cfg.stage_channels(i),)
    out["conv_pre.weight"] = (cfg.upsample_initial_channel, cfg.initial_channel, 7)
    out["conv_pre.bias"] = (cfg.upsample_initial_channel,)
    for i, k in enumerate(cfg.upsample_kernel_sizes):
        _wn_shapes(out, f"ups.{i}", (cfg.upsample_initial_channel >> i, cfg.stage_channels(i), k))
    nk = len(cfg.resblock_kernel_sizes)
    for i in range(n):
        ch = cfg.stage_channels(i)
        for j, k in enumerate(cfg.resblock_kernel_sizes):
            for group in ("convs1", "convs2"):
                for m in range(3):
                    _wn_shapes(out, f"resblocks.{i * nk + j}.{group}.{m}", (ch, ch, k))
    out["conv_post.weight"] = (1, cfg.stage_channels(n - 1), 7)
    if cfg.gin_channels:
        out["cond.weight"] = (cfg.upsample_initial_channel, cfg.gin_channels, 1)
        out["cond.bias"] = (cfg.upsample_initial_channel,)
    return out


def synthetic_state_dict(cfg: NSFConfig = V2_40K, seed: int = 0) -> Dict[str, torch.Tensor]:
    """seeded random-init weights for any configuration (tests, benchmarks), drawn from ``np.random.default_rng(seed)`` in the state dict's
    order.  The draw keeps the network non-degenerate at full depth.  Every weight-normed layer gets ``weight_v`` standard normal and a
    ``weight_g`` that sets the gain: the first convolution of a ResBlock pair at unit gain behind LeakyReLU(0.1) (which keeps 0.505 of the
    variance), the second at 0.3 so that the three residual additions of a block grow the signal by a few tenths, not eightfold; a
    transposed convolution has Cin K / u products per output, so g = sqrt(Cout K / (0.505 Cin K / u)).  The noise convolutions carry the
    source (|har| around 0.07) into every stage at about a third of the stage's level, and conv_post brings the value in front of the final
    tanh to a standard deviation of about 0.5."""
    rng = np.random.default_rng(seed)
    sd: Dict[str, torch.Tensor] = {}
    for name, shape in param_shapes(cfg).items():
        leaf = name.rsplit(".", 1)[1]
        if name == "m_source.l_linear.weight":
            v = 1.0 + 0.05 * rng.standard_normal(shape)
        elif name == "m_source.l_linear.bias":
            v = 0.02 * rng.standard_normal(shape)
        elif leaf == "bias":
            v = 0.05 * rng.standard_normal(shape)
        elif name.startswith("noise_convs."):                                # ks taps of a source of rms 0.07 -> about 0.35
            v = rng.standard_normal(shape) * (5.0 / np.sqrt(shape[2]))
        elif name == "conv_pre.weight":
            v = rng.standard_normal(shape) / np.sqrt(shape[1] * shape[2])
        elif name == "cond.weight":
            v = 0.3 * rng.standard_normal(shape) / np.sqrt(shape[1])
        elif name == "conv_post.weight":
            v = 0.5 * rng.standard_normal(shape) / np.sqrt(0.5 * shape[1] * shape[2])
        elif leaf == "weight_v":
            v = rng.standard_normal(shape)
        elif leaf == "weight_g":                                             # w = v g / |v|, |v| about sqrt(fan) for a standard-normal v
            vs = param_shapes(cfg)[name[:-1] + "v"]
            if name.startswith("ups."):
                u = cfg.upsample_rates[int(name.split(".")[1])]
                gain = np.sqrt(vs[1] * u / (0.505 * vs[0]))                  # per-weight sigma sqrt(u / (0.505 Cin K)) times sqrt(Cout K)
            elif ".convs1." in name:
                gain = np.sqrt(1.0 / 0.505)
            else:
                gain = 0.3 * np.sqrt(1.0 / 0.505)
            v = gain * rng.uniform(0.9, 1.1, shape)
        else:
            raise AssertionError(name)
        sd[name] = torch.from_numpy(np.asarray(v, dtype=np.float32).reshape(shape))
    return sd


def _wn_names(cfg: NSFConfig) -> List[str]:
    return [k[:-len(".weight_v")] for k in param_shapes(cfg) if k.endswith(".weight_v")]


def check_state_dict(sd: Dict[str, torch.Tensor], cfg: NSFConfig = V2_40K) -> None:
    """every tensor's name and shape against the configuration; AlsepError names the first that does not fit.  A weight-normed layer may
    carry ``weight_g`` / ``weight_v`` or the plain ``weight`` that ``remove_weight_norm`` leaves."""
    want = dict(param_shapes(cfg))
    for p in _wn_names(cfg):
        if f"{p}.weight" in sd and f"{p}.weight_v" not in sd and f"{p}.weight_g" not in sd:
            want[f"{p}.weight"] = want.pop(f"{p}.weight_v")
            want.pop(f"{p}.weight_g")
    for name, shape in want.items():
        if name not in sd:
            raise AlsepError(f"nsf: the state dict has no tensor {name}")
        if tuple(sd[name].shape) != tuple(shape):
            raise AlsepError(f"nsf: tensor {name} has shape {tuple(sd[name].shape)}, the configuration needs {tuple(shape)}")
    extra = [k for k in sd if k not in want]
    if extra:
        raise AlsepError(f"nsf: the state dict has a tensor the configuration does not know: {extra[0]}")


def fold_weight_norm(g: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    """``w = v g / |v|``, the norm over every axis but the first (``torch._weight_norm(v, g, 0)``), in float64, rounded once"""
    v64, g64 = v.double(), g.double()
    norm = torch.sqrt(torch.sum(v64 * v64, dim=tuple(range(1, v64.dim())), keepdim=True))
    return (v64 * (g64 / norm)).float()


def layer_weight(sd: Dict[str, torch.Tensor], p: str) -> torch.Tensor:
    """the float32 weight of layer ``p``: folded from weight_g / weight_v, or the plain weight"""
    if f"{p}.weight_v" in sd:
        return fold_weight_norm(sd[f"{p}.weight_g"], sd[f"{p}.weight_v"])
    return sd[f"{p}.weight"].float()


# ---- stage wrappers -----------------------------------------------------------------------------------------------------------------------
def _t(ctx: Context, a, dtype=torch.float32) -> torch.Tensor:
    t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else torch.as_tensor(a)
    return t.to(ctx.device, dtype).contiguous()


def source(ctx: Context, f0: torch.Tensor, noise: torch.Tensor, upp: int, sr: int, lin_w: float, lin_b: float) -> torch.Tensor:
    """``f0 [T]``, ``noise [T upp]`` on the device -> ``har [T upp]``"""
    T = int(f0.shape[0])
    if f0.dim() != 1 or T < 1 or T > MAX_FRAMES:
        raise AlsepError(f"nsf: f0 of shape {tuple(f0.shape)} ([1 .. {MAX_FRAMES}] frames)")
    if tuple(noise.shape) != (T * upp,):
        raise AlsepError(f"nsf: noise of shape {tuple(noise.shape)}, {T} frames of {upp} samples need ({T * upp},)")
    nbytes = int(ctx.lib.alsep_nsf_source_workspace_bytes(T))
    ws = ctx.empty(((nbytes + 7) // 8,), torch.float64)
    har = ctx.empty((T * upp,))
    ctx.check(ctx.lib.alsep_nsf_source(ctx.handle, _lib.ptr(f0), T, int(upp), int(sr), _lib.ptr(noise), float(lin_w), float(lin_b), _lib.ptr(har),
                                       _lib.ptr(ws), nbytes), "alsep_nsf_source")
    return har


def conv1d(ctx: Context, x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, res: Optional[torch.Tensor] = None,
           acc: Optional[torch.Tensor] = None, dilation: int = 1, pre_slope: float = 1.0, post: int = 0, out_scale: float = 1.0,
           out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``x [L, Cin]``, ``w [K, Cin, Cout]`` -> ``out_scale (acc + post(conv(lrelu(x, pre_slope)) + bias + res))`` ``[L, Cout]``"""
    L, Cin = (int(v) for v in x.shape)
    K, Cout = int(w.shape[0]), int(w.shape[2])
    if int(w.shape[1]) != Cin:
        raise AlsepError(f"nsf: convolution of {tuple(x.shape)} by {tuple(w.shape)}")
    for name, t in (("res", res), ("acc", acc), ("out", out)):
        if t is not None and tuple(t.shape) != (L, Cout):
            raise AlsepError(f"nsf: {name} of shape {tuple(t.shape)}, the convolution gives {(L, Cout)}")
    if bias is not None and bias.numel() != Cout:
        raise AlsepError(f"nsf: bias of {bias.numel()} values for {Cout} channels")
    y = out if out is not None else ctx.empty((L, Cout))
    ctx.check(ctx.lib.alsep_nsf_conv1d(ctx.handle, _lib.ptr(x), _lib.ptr(w), _lib.ptr(bias), _lib.ptr(res), _lib.ptr(acc), _lib.ptr(y), L, Cin, Cout,
                                       K, int(dilation), float(pre_slope), int(post), float(out_scale)), "alsep_nsf_conv1d")
    return y


def conv_post(ctx: Context, x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """``x [L, C]``, ``w [7, C]`` -> ``tanh(conv(lrelu(x, 0.01)))`` ``[L]``"""
    L, Cc = (int(v) for v in x.shape)
    if tuple(w.shape) != (7, Cc):
        raise AlsepError(f"nsf: conv_post of {tuple(x.shape)} by {tuple(w.shape)}")
    y = ctx.empty((L,))
    ctx.check(ctx.lib.alsep_nsf_conv_post(ctx.handle, _lib.ptr(x), _lib.ptr(w), _lib.ptr(y), L, Cc), "alsep_nsf_conv_post")
    return y


def tconv1d(ctx: Context, x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, har: torch.Tensor, noise_w: torch.Tensor, noise_b: torch.Tensor,
            u: int, s: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``x [L, Cin]``, ``w [K, Cin, Cout]``, ``har [L u s]``, ``noise_w [2 s or 1, Cout]`` -> ``[L u, Cout]``"""
    L, Cin = (int(v) for v in x.shape)
    K, Cout = int(w.shape[0]), int(w.shape[2])
    ks = 2 * s if s > 1 else 1
    if int(w.shape[1]) != Cin or tuple(noise_w.shape) != (ks, Cout) or bias.numel() != Cout or noise_b.numel() != Cout or \
            tuple(har.shape) != (L * u * s,):
        raise AlsepError(f"nsf: transposed convolution of {tuple(x.shape)} by {tuple(w.shape)} at rate {u}, source {tuple(har.shape)} by "
                         f"{tuple(noise_w.shape)} at stride {s}")
    y = out if out is not None else ctx.empty((L * u, Cout))
    if tuple(y.shape) != (L * u, Cout):
        raise AlsepError(f"nsf: out of shape {tuple(y.shape)}, the transposed convolution gives {(L * u, Cout)}")
    ctx.check(ctx.lib.alsep_nsf_tconv1d(ctx.handle, _lib.ptr(x), _lib.ptr(w), _lib.ptr(bias), _lib.ptr(har), _lib.ptr(noise_w), _lib.ptr(noise_b),
                                        _lib.ptr(y), L, Cin, Cout, K, int(u), int(s)), "alsep_nsf_tconv1d")
    return y


# ---- the network --------------------------------------------------------------------------------------------------------------------------
class _Stage:
    pass


class NSFVocoder:
    """the host mirror of ``GeneratorNSF``: weights folded and packed on the device at construction, ``forward`` is launches only"""

    def __init__(self, state_dict: Dict[str, torch.Tensor], cfg: NSFConfig = V2_40K, ctx: Optional[Context] = None):
        cfg.check()
        check_state_dict(state_dict, cfg)
        self.cfg, self.ctx = cfg, ctx if ctx is not None else _lib.default_context(None)
        ctx, sd = self.ctx, state_dict
        self.upp = cfg.upp
        self.lin_w, self.lin_b = float(sd["m_source.l_linear.weight"].reshape(-1)[0]), float(sd["m_source.l_linear.bias"].reshape(-1)[0])
        dev = lambda t: t.float().contiguous().to(ctx.device)                 # noqa: E731
        self.w_pre = dev(sd["conv_pre.weight"].permute(2, 1, 0))              # [Cout, Cin, K] -> [K][Cin][Cout]
        self.b_pre = dev(sd["conv_pre.bias"])
        if cfg.gin_channels:
            self.w_cond = dev(sd["cond.weight"][:, :, 0])                     # [C0, gin]
            self.b_cond_pre = dev((sd["cond.bias"].double() + sd["conv_pre.bias"].double()).float())
        nk = len(cfg.resblock_kernel_sizes)
        self.stages: List[_Stage] = []
        for i, (u, k) in enumerate(zip(cfg.upsample_rates, cfg.upsample_kernel_sizes)):
            st = _Stage()
            st.u, st.k, st.s = u, k, cfg.source_stride(i)
            st.w = dev(layer_weight(sd, f"ups.{i}").permute(2, 0, 1))         # [Cin, Cout, K] -> [K][Cin][Cout]
            st.b = dev(sd[f"ups.{i}.bias"])
            st.nw = dev(sd[f"noise_convs.{i}.weight"][:, 0, :].t())           # [Cout, 1, ks] -> [ks][Cout]
            st.nb = dev(sd[f"noise_convs.{i}.bias"])
            st.blocks = []
            for j, dil in enumerate(cfg.resblock_dilation_sizes):
                p = f"resblocks.{i * nk + j}"
                pairs = []
                for m, d in enumerate(dil):
                    pairs.append((dev(layer_weight(sd, f"{p}.convs1.{m}").permute(2, 1, 0)), dev(sd[f"{p}.convs1.{m}.bias"]), int(d),
                                  dev(layer_weight(sd, f"{p}.convs2.{m}").permute(2, 1, 0)), dev(sd[f"{p}.convs2.{m}.bias"])))
                st.blocks.append(pairs)
            self.stages.append(st)
        self.w_post = dev(sd["conv_post.weight"][0].t())                      # [1, C, 7] -> [7][C]
        self.generator = torch.Generator(device=ctx.device)

    def manual_seed(self, seed: int) -> "NSFVocoder":
        """seed of the generator ``forward`` draws the source's noise from when the caller gives none"""
        self.generator.manual_seed(int(seed))
        return self

    def source(self, f0, noise=None) -> torch.Tensor:
        """``f0 [1, T]`` (or ``[T]``), ``noise [T upp]`` standard normal or None -> ``har [T upp]`` on the device"""
        ctx = self.ctx
        f = _t(ctx, f0).reshape(-1)
        n = int(f.shape[0]) * self.upp
        if noise is None:
            noise = torch.randn((n,), device=ctx.device, dtype=torch.float32, generator=self.generator)
        return source(ctx, f, _t(ctx, noise).reshape(-1), self.upp, self.cfg.sr, self.lin_w, self.lin_b)

    def pre(self, x, g=None) -> torch.Tensor:
        """``x [1, C, T]``, ``g [1, gin, 1]`` or None -> ``conv_pre(x) + cond(g)`` ``[T, C0]``"""
        ctx, cfg = self.ctx, self.cfg
        xt = _t(ctx, x)
        if xt.dim() != 3 or int(xt.shape[0]) != 1 or int(xt.shape[1]) != cfg.initial_channel:
            raise AlsepError(f"nsf: x of shape {tuple(xt.shape)} ([1, {cfg.initial_channel}, T]: batch 1 only)")
        xc = xt[0].t().contiguous()
        bias = self.b_pre
        if g is not None:
            if not cfg.gin_channels:
                raise AlsepError("nsf: g given to a network with gin_channels = 0")
            gv = _t(ctx, g).reshape(1, -1)
            if int(gv.shape[1]) != cfg.gin_channels:
                raise AlsepError(f"nsf: g of shape {tuple(torch.as_tensor(g).shape)} ([1, {cfg.gin_channels}, 1])")
            c0, k, arr = cfg.upsample_initial_channel, cfg.gin_channels, C.c_int64 * 4
            bias = ctx.empty((c0,))
            ctx.check(ctx.lib.alsep_nn_bgemm_bias(ctx.handle, _lib.ptr(gv), _lib.ptr(self.w_cond), _lib.ptr(bias), 1, 1, 1, c0, k, arr(0, 0, k, 1),
                                                  arr(0, 0, k, 1), arr(0, 0, c0, 1), 1.0, _lib.ptr(self.b_cond_pre), 0), "alsep_nn_bgemm_bias")
        return conv1d(ctx, xc, self.w_pre, bias=bias, pre_slope=1.0)

    def stage(self, i: int, x: torch.Tensor, har: torch.Tensor) -> torch.Tensor:
        """upsampling stage ``i`` with its resblocks: ``x [L, C]``, ``har [L upp_i]`` -> ``[L u, C / 2]``"""
        ctx, st = self.ctx, self.stages[i]
        h = tconv1d(ctx, x, st.w, st.b, har, st.nw, st.nb, st.u, st.s)
        nk = len(st.blocks)
        xs = None
        for j, pairs in enumerate(st.blocks):
            xb = h
            for m, (w1, b1, d, w2, b2) in enumerate(pairs):
                t = conv1d(ctx, xb, w1, bias=b1, dilation=d, pre_slope=LRELU_SLOPE)
                last = m == len(pairs) - 1
                xb = conv1d(ctx, t, w2, bias=b2, res=xb, acc=xs if last else None, pre_slope=LRELU_SLOPE,
                            out_scale=1.0 / nk if (last and j == nk - 1) else 1.0)
            xs = xb
        return xs

    def post(self, x: torch.Tensor) -> torch.Tensor:
        return conv_post(self.ctx, x, self.w_post)

    def forward(self, x, f0, g=None, n_res=None, noise=None) -> torch.Tensor:
        """``x [1, C, T]``, ``f0 [1, T]``, ``g [1, gin, 1]`` or None -> ``[1, 1, T upp]`` on the device"""
        if n_res is not None:
            raise AlsepError("nsf: n_res not built (no interpolation of the frame axis)")
        T = int(torch.as_tensor(x).shape[-1])
        if int(torch.as_tensor(f0).numel()) != T:
            raise AlsepError(f"nsf: f0 of {int(torch.as_tensor(f0).numel())} frames beside x of {T}")
        har = self.source(f0, noise)
        h = self.pre(x, g)
        for i in range(len(self.stages)):
            h = self.stage(i, h, har)
        return self.post(h).view(1, 1, T * self.upp)

    __call__ = forward


def load_rvc_vocoder(path, ctx: Optional[Context] = None) -> Tuple[NSFVocoder, torch.Tensor]:
    """an RVC ``.pth`` -> ``(NSFVocoder, emb_g [speakers, gin])``; ``g = emb_g[sid][None, :, None]``"""
    if not os.path.exists(str(path)):
        raise FileNotFoundError(f"nsf: {path} not found")
    cpt = torch.load(str(path), map_location="cpu", weights_only=True)
    if int(cpt.get("f0", 1)) != 1:
        raise AlsepError(f"nsf: checkpoint with f0 = {cpt.get('f0')} not built (the generators without f0 are not)")
    version = cpt.get("version", "v1")
    if version not in ("v1", "v2"):
        raise AlsepError(f"nsf: checkpoint version {version!r} (v1 or v2)")
    cfg = NSFConfig.from_rvc(cpt["config"])
    weights = cpt["weight"]
    sd = {k[len("dec."):]: v.float() for k, v in weights.items() if k.startswith("dec.")}
    if "emb_g.weight" not in weights:
        raise AlsepError("nsf: the checkpoint has no tensor emb_g.weight")
    return NSFVocoder(sd, cfg, ctx), weights["emb_g.weight"].float()
