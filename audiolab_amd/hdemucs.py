"""HDemucs (Hybrid Demucs v3, ``hdemucs_mmi.yaml``) on the GPU, float32.

The network is demucs 4.0.1's ``demucs.hdemucs.HDemucs`` in eval mode, restated from the published design (PARITY UNPINNED, as for
HTDemucs; tests/hdemucs_oracle.py is the torch-CPU twin).  Parameter names are demucs', so a real ``state_dict`` loads as it is.

What differs from HTDemucs (htdemucs.py, whose float32 building blocks ``_DemucsOps`` this class reuses):
  * frequency layers run until one bin is left: the layer where ``freqs <= kernel_size`` has ``kernel = freqs``, no padding, and an EMPTY
    time-branch partner (a convolution only) whose output is added to the frequency convolution's before norm and GELU; its decoder
    partner takes the frequency decoder's ``pre[:, :, 0]``;
  * later layers are 1-D on the merged branch (kernel ``2 time_stride``, stride ``time_stride``);
  * GroupNorm(norm_groups) as norm1 / norm2 of the layers ``index >= norm_starts`` (``alsep_nn_group_norm``; a decoder normalises its
    whole transposed-convolution output, then crops it);
  * the DConv branches of the layers ``index >= dconv_lstm`` / ``dconv_attn`` hold a BLSTM (``alsep_nn_blstm_unfold`` -> input GEMM ->
    ``alsep_nn_lstm`` per layer -> GEMM -> ... -> Linear -> ``alsep_nn_blstm_stitch``) and a LocalState (one fused 1x1 projection, a
    strided batched GEMM, ``alsep_nn_localstate_softmax``, a second GEMM, the output projection);
  * no transformer, no bottleneck: the decoder starts from zeros.
``forward`` takes [2, L] or a batch [B, 2, L] of any length (no padding to a training length: the network pads to its own strides); every
launch covers the whole batch, and every sample comes out bit-identical to that sample run alone.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import torch

from . import _lib
from ._lib import AlsepError, Context
from .htdemucs import ACT_GELU, ACT_GLU, ACT_NONE, _Conv, _DemucsOps

LSTM_MAX_STEPS = 200          # demucs DConv: BLSTM(hidden, layers=2, max_steps=200, skip=True)
LOCAL_HEADS, LOCAL_NDECAY = 4, 4


@dataclass(frozen=True)
class HDemucsConfig:
    sources: Tuple[str, ...] = ("drums", "bass", "other", "vocals")
    audio_channels: int = 2
    channels: int = 48
    growth: int = 2
    nfft: int = 4096
    depth: int = 6
    kernel_size: int = 8
    stride: int = 4
    time_stride: int = 2
    context: int = 1
    context_enc: int = 0
    norm_starts: int = 4
    norm_groups: int = 4
    dconv_mode: int = 1
    dconv_depth: int = 2
    dconv_comp: int = 4
    dconv_attn: int = 4
    dconv_lstm: int = 4
    dconv_init: float = 1e-4
    freq_emb: float = 0.2
    emb_scale: float = 10.0
    samplerate: int = 44100
    segment_samples: int = 40 * 44100

    @property
    def hop(self) -> int:
        return self.nfft // 4

    @property
    def S(self) -> int:
        return len(self.sources)


@dataclass(frozen=True)
class _Layer:
    """one encoder index of HDemucs.__init__: geometry and widths (enc: frequency / merged branch, tenc: time branch)"""
    index: int
    freq: bool
    last_freq: bool
    ker: int
    stri: int
    pad: int
    norm: bool
    lstm: bool
    attn: bool
    enc_in: int
    enc_out: int
    dec_out: int
    tenc_in: int
    tenc_out: int
    tdec_out: int


def layer_plan(cfg: HDemucsConfig) -> List[_Layer]:
    """HDemucs.__init__'s loop over the encoder indexes (multi_freqs off, hybrid, cac)"""
    out = []
    freqs = cfg.nfft // 2
    chin, chin_z = cfg.audio_channels, cfg.audio_channels * 2
    chout = chout_z = cfg.channels
    for index in range(cfg.depth):
        freq = freqs > 1
        ker, stri = (cfg.kernel_size, cfg.stride) if freq else (2 * cfg.time_stride, cfg.time_stride)
        pad, last_freq = ker // 4, False
        if freq and freqs <= cfg.kernel_size:
            ker, pad, last_freq = freqs, 0, True
        if last_freq:
            chout_z = max(chout, chout_z)
            chout = chout_z
        enc_in, tenc_in = chin_z, chin
        if index == 0:
            chin = cfg.audio_channels * cfg.S
            chin_z = chin * 2
        out.append(_Layer(index, freq, last_freq, ker, stri, pad, index >= cfg.norm_starts, index >= cfg.dconv_lstm, index >= cfg.dconv_attn,
                          enc_in, chout_z, chin_z, tenc_in, chout, chin))
        chin, chin_z = chout, chout_z
        chout, chout_z = int(cfg.growth * chout), int(cfg.growth * chout_z)
        if freq:
            freqs = 1 if freqs <= cfg.kernel_size else freqs // cfg.stride
    return out


def _dconv_index(lstm: bool, attn: bool) -> Dict[str, int]:
    """positions inside one DConv layer's nn.Sequential: conv, norm, GELU, [BLSTM], [LocalState], conv, norm, GLU, LayerScale"""
    i = 3
    pos = {}
    if lstm:
        pos["lstm"] = i
        i += 1
    if attn:
        pos["attn"] = i
        i += 1
    pos.update(conv2=i, norm2=i + 1, scale=i + 3)
    return pos


def expected_shapes(cfg: HDemucsConfig) -> Dict[str, Tuple[Tuple[int, ...], str]]:
    """name -> (shape, hyper-parameter that fixes it) of every tensor an HDemucs with this configuration reads (demucs' names)"""
    exp: Dict[str, Tuple[Tuple[int, ...], str]] = {}
    wch = f"channels={cfg.channels} / growth={cfg.growth} / depth={cfg.depth} / nfft={cfg.nfft}"

    def conv(p, cout, cin, *k, transposed=False, hyper=wch):
        exp[p + ".weight"] = (((cin, cout) if transposed else (cout, cin)) + tuple(k), hyper)
        exp[p + ".bias"] = ((cout,), hyper)

    def norm(p, c, hyper):
        exp[p + ".weight"] = ((c,), hyper)
        exp[p + ".bias"] = ((c,), hyper)

    def dconv(p, c, L: _Layer):
        hid = c // cfg.dconv_comp
        hy = f"dconv_comp={cfg.dconv_comp} / dconv_depth={cfg.dconv_depth} / {wch}"
        pos = _dconv_index(L.lstm, L.attn)
        for d in range(cfg.dconv_depth):
            q = f"{p}.layers.{d}"
            conv(q + ".0", hid, c, 3, hyper=hy)
            norm(q + ".1", hid, hy)
            if L.lstm:
                hl = f"dconv_lstm={cfg.dconv_lstm} / {hy}"
                for layer in range(2):
                    for sfx in ("", "_reverse"):
                        exp[f"{q}.{pos['lstm']}.lstm.weight_ih_l{layer}{sfx}"] = ((4 * hid, hid if layer == 0 else 2 * hid), hl)
                        exp[f"{q}.{pos['lstm']}.lstm.weight_hh_l{layer}{sfx}"] = ((4 * hid, hid), hl)
                        exp[f"{q}.{pos['lstm']}.lstm.bias_ih_l{layer}{sfx}"] = ((4 * hid,), hl)
                        exp[f"{q}.{pos['lstm']}.lstm.bias_hh_l{layer}{sfx}"] = ((4 * hid,), hl)
                conv(f"{q}.{pos['lstm']}.linear", hid, 2 * hid, hyper=hl)
            if L.attn:
                ha = f"dconv_attn={cfg.dconv_attn} / {hy}"
                for n in ("content", "query", "key", "proj"):
                    conv(f"{q}.{pos['attn']}.{n}", hid, hid, 1, hyper=ha)
                conv(f"{q}.{pos['attn']}.query_decay", LOCAL_HEADS * LOCAL_NDECAY, hid, 1, hyper=ha)
            conv(f"{q}.{pos['conv2']}", 2 * c, hid, 1, hyper=hy)
            norm(f"{q}.{pos['norm2']}", 2 * c, hy)
            exp[f"{q}.{pos['scale']}.scale"] = ((c,), hy)

    ke, kd = 1 + 2 * cfg.context_enc, 1 + 2 * cfg.context
    hn = f"norm_starts={cfg.norm_starts} / {wch}"
    n_freq = sum(L.freq for L in layer_plan(cfg))
    for L in layer_plan(cfg):
        i, di = L.index, cfg.depth - 1 - L.index
        fk = (L.ker, 1) if L.freq else (L.ker,)
        conv(f"encoder.{i}.conv", L.enc_out, L.enc_in, *fk, hyper=f"kernel_size={cfg.kernel_size} / {wch}")
        conv(f"decoder.{di}.conv_tr", L.dec_out, L.enc_out, *fk, transposed=True, hyper=f"sources ({cfg.S}) / {wch}")
        conv(f"encoder.{i}.rewrite", 2 * L.enc_out, L.enc_out, *((ke, ke) if L.freq else (ke,)), hyper=f"context_enc={cfg.context_enc} / {wch}")
        conv(f"decoder.{di}.rewrite", 2 * L.enc_out, L.enc_out, *((kd, kd) if L.freq else (kd,)), hyper=f"context={cfg.context} / {wch}")
        if L.norm:
            norm(f"encoder.{i}.norm1", L.enc_out, hn)
            norm(f"encoder.{i}.norm2", 2 * L.enc_out, hn)
            norm(f"decoder.{di}.norm1", 2 * L.enc_out, hn)
            norm(f"decoder.{di}.norm2", L.dec_out, hn)
        if cfg.dconv_mode & 1:
            dconv(f"encoder.{i}.dconv", L.enc_out, L)
        if cfg.dconv_mode & 2:
            dconv(f"decoder.{di}.dconv", L.enc_out, L)
        if not L.freq:
            continue
        ti = n_freq - 1 - i
        conv(f"tencoder.{i}.conv", L.tenc_out, L.tenc_in, cfg.kernel_size, hyper=f"kernel_size={cfg.kernel_size} / {wch}")
        conv(f"tdecoder.{ti}.conv_tr", L.tdec_out, L.tenc_out, cfg.kernel_size, transposed=True, hyper=f"sources ({cfg.S}) / {wch}")
        if L.norm:
            norm(f"tdecoder.{ti}.norm2", L.tdec_out, hn)
        if L.last_freq:
            continue
        conv(f"tencoder.{i}.rewrite", 2 * L.tenc_out, L.tenc_out, ke, hyper=f"context_enc={cfg.context_enc} / {wch}")
        conv(f"tdecoder.{ti}.rewrite", 2 * L.tenc_out, L.tenc_out, kd, hyper=f"context={cfg.context} / {wch}")
        if L.norm:
            norm(f"tencoder.{i}.norm1", L.tenc_out, hn)
            norm(f"tencoder.{i}.norm2", 2 * L.tenc_out, hn)
            norm(f"tdecoder.{ti}.norm1", 2 * L.tenc_out, hn)
        if cfg.dconv_mode & 1:
            dconv(f"tencoder.{i}.dconv", L.tenc_out, L)
        if cfg.dconv_mode & 2:
            dconv(f"tdecoder.{ti}.dconv", L.tenc_out, L)
    exp["freq_emb.embedding.weight"] = ((cfg.nfft // 2 // cfg.stride, cfg.channels), f"nfft={cfg.nfft} / stride={cfg.stride} / channels={cfg.channels}")
    return exp


def check_config(cfg: HDemucsConfig) -> None:
    """the structural limits of this implementation, by hyper-parameter"""
    plan = layer_plan(cfg)
    if cfg.audio_channels != 2 or cfg.kernel_size != 2 * cfg.stride:
        raise AlsepError("HDemucs: kernel_size must be 2 * stride and the input stereo")
    if not plan[0].freq or plan[0].last_freq:
        raise AlsepError(f"HDemucs: nfft={cfg.nfft} leaves no full frequency layer before the last one")
    if not any(L.last_freq for L in plan) and not all(L.freq for L in plan):
        raise AlsepError(f"HDemucs: nfft={cfg.nfft} / depth={cfg.depth}: the frequency axis does not end on a last frequency layer")
    for L in plan:
        if L.last_freq and L.ker % 2:
            raise AlsepError(f"HDemucs: the last frequency layer's kernel (freqs = {L.ker}, from nfft={cfg.nfft}) must be even")
        if L.norm and (L.enc_out % cfg.norm_groups or L.dec_out % cfg.norm_groups or L.tdec_out % cfg.norm_groups):
            raise AlsepError(f"HDemucs: norm_groups={cfg.norm_groups} does not divide the widths of layer {L.index}")
        hid = L.enc_out // cfg.dconv_comp
        if L.lstm and (hid % 16 or hid > 512):
            raise AlsepError(f"HDemucs: dconv_comp={cfg.dconv_comp}: the BLSTM hidden size {hid} of layer {L.index} must be a multiple of 16 "
                             f"up to 512")
        if L.attn and hid % LOCAL_HEADS:
            raise AlsepError(f"HDemucs: dconv_comp={cfg.dconv_comp}: LocalState width {hid} of layer {L.index} is not divisible by 4 heads")
    if cfg.dconv_mode not in (1, 2, 3):
        raise AlsepError(f"HDemucs: dconv_mode={cfg.dconv_mode} (1, 2 or 3)")


def blstm_params(ctx: Context, sd: Dict[str, torch.Tensor], p: str) -> dict:
    """demucs BLSTM ``p`` (``p.lstm.*_l{0,1}{,_reverse}``, ``p.linear.*``) in the layouts of DConvOps._blstm: per layer the input projection of
    both directions as one Linear (bias = b_ih + b_hh) and W_hh^T [2, H, 4H]"""
    H = int(sd[p + ".lstm.weight_hh_l0"].shape[1])
    layers = []
    for k in range(2):
        wi = torch.cat([sd[f"{p}.lstm.weight_ih_l{k}"], sd[f"{p}.lstm.weight_ih_l{k}_reverse"]])                        # [8H, in]
        bi = torch.cat([sd[f"{p}.lstm.bias_ih_l{k}"] + sd[f"{p}.lstm.bias_hh_l{k}"],
                        sd[f"{p}.lstm.bias_ih_l{k}_reverse"] + sd[f"{p}.lstm.bias_hh_l{k}_reverse"]])
        whh_t = torch.stack([sd[f"{p}.lstm.weight_hh_l{k}"].t(), sd[f"{p}.lstm.weight_hh_l{k}_reverse"].t()])              # [2, H, 4H]
        layers.append(dict(wih=_Conv(ctx, wi.t()[None, None], bi), whh_t=whh_t.detach().float().contiguous().to(ctx.device)))
    return dict(H=H, layers=layers, linear=_Conv(ctx, sd[p + ".linear.weight"].t()[None, None], sd[p + ".linear.bias"]))


def localstate_params(ctx: Context, sd: Dict[str, torch.Tensor], p: str) -> dict:
    """demucs LocalState ``p`` (heads 4, ndecay 4, no frequency features): query | key | content | query_decay as ONE 1x1 projection, proj"""
    names = ("query", "key", "content", "query_decay")
    w = torch.cat([sd[f"{p}.{n}.weight"][..., 0] for n in names])
    b = torch.cat([sd[f"{p}.{n}.bias"] for n in names])
    return dict(qkvd=_Conv(ctx, w.t()[None, None], b), proj=_Conv(ctx, sd[p + ".proj.weight"][..., 0].t()[None, None], sd[p + ".proj.bias"]))


class DConvOps(_DemucsOps):
    """the operators HDemucs adds to the float32 Demucs building blocks, on one context: GroupNorm(norm_groups), BLSTM, LocalState"""

    norm_groups = 4

    def __init__(self, ctx: Context):
        self.ctx = ctx
        self._plans: Dict[int, object] = {}
        self._ws: Optional[torch.Tensor] = None
        self._gn: Optional[torch.Tensor] = None

    def _group_norm(self, x: torch.Tensor, B: int, R: int, Cn: int, gb, act: int, r0: int = 0, Ro: Optional[int] = None) -> torch.Tensor:
        """GroupNorm(norm_groups) over [B, R, Cn] + act, rows [r0, r0 + Ro) of each sample kept"""
        ctx, G = self.ctx, self.norm_groups
        Ro = R if Ro is None else Ro
        if self._gn is None or self._gn.numel() < 2 * B * G:
            self._gn = ctx.empty((max(2 * B * G, 64),))
        y = ctx.empty((B * Ro, Cn // 2 if act == ACT_GLU else Cn))
        ctx.check(ctx.lib.alsep_nn_group_norm(ctx.handle, _lib.ptr(x), _lib.ptr(y), _lib.ptr(gb[0]), _lib.ptr(gb[1]), B, R, Cn, G, 1e-5, act,
                                              r0, Ro, _lib.ptr(self._gn)), "alsep_nn_group_norm")
        return y

    def _blstm(self, x: torch.Tensor, G: int, T: int, P) -> torch.Tensor:
        """demucs BLSTM(dim, layers=2, max_steps=200, skip=True) over G sequences x [G, T, dim] -> [G, T, dim]"""
        ctx = self.ctx
        lib, h = ctx.lib, ctx.handle
        H = P["H"]
        if T > LSTM_MAX_STEPS:
            width, stride = LSTM_MAX_STEPS, LSTM_MAX_STEPS // 2
            nf = -(-T // stride)
        else:
            width, stride, nf = T, T, 1
        N = G * nf
        fr = ctx.empty((width * N, H))
        ctx.check(lib.alsep_nn_blstm_unfold(h, _lib.ptr(x), _lib.ptr(fr), G, T, H, width, stride, nf), "alsep_nn_blstm_unfold")
        y = fr
        for layer in P["layers"]:
            pre, _, _ = self._conv(y, width * N, 1, layer["wih"])                     # [width, N, 8H]: both directions, one GEMM
            y = ctx.empty((width * N, 2 * H))
            ctx.check(lib.alsep_nn_lstm(h, _lib.ptr(pre), _lib.ptr(layer["whh_t"]), _lib.ptr(y), width, N, H), "alsep_nn_lstm")
        y, _, _ = self._conv(y, width * N, 1, P["linear"])
        out = ctx.empty((G * T, H))
        ctx.check(lib.alsep_nn_blstm_stitch(h, _lib.ptr(y), _lib.ptr(x), _lib.ptr(out), G, T, H, width, stride, nf), "alsep_nn_blstm_stitch")
        return out

    def _local_state(self, x: torch.Tensor, G: int, T: int, Cn: int, P) -> torch.Tensor:
        """demucs LocalState(Cn, heads=4, ndecay=4) over G sequences x [G, T, Cn] -> x + proj(attention) [G, T, Cn]"""
        ctx = self.ctx
        lib, h = ctx.lib, ctx.handle
        Hh, nd = LOCAL_HEADS, LOCAL_NDECAY
        dh = Cn // Hh
        ld = 3 * Cn + Hh * nd
        qkvd, _, _ = self._conv(x, G * T, 1, P["qkvd"])                                  # [G, T, q | k | content | decay]
        Tp = -(-T // 4) * 4
        scores = ctx.empty((G * Hh * T, Tp))
        arr = C.c_int64 * 4
        base = qkvd.data_ptr()
        ctx.check(lib.alsep_nn_bgemm(h, C.c_void_p(base), C.c_void_p(base + 4 * Cn), _lib.ptr(scores), G, Hh, T, T, dh,
                                     arr(T * ld, dh, ld, 1), arr(T * ld, dh, ld, 1), arr(Hh * T * Tp, T * Tp, Tp, 1), 1.0 / math.sqrt(dh)),
                  "alsep_nn_bgemm")
        ctx.check(lib.alsep_nn_localstate_softmax(h, _lib.ptr(scores), C.c_void_p(base + 4 * 3 * Cn), G, Hh, T, Tp, nd, ld),
                  "alsep_nn_localstate_softmax")
        res = ctx.empty((G * T, Cn))
        ctx.check(lib.alsep_nn_bgemm(h, _lib.ptr(scores), C.c_void_p(base + 4 * 2 * Cn), _lib.ptr(res), G, Hh, T, dh, T,
                                     arr(Hh * T * Tp, T * Tp, Tp, 1), arr(T * ld, dh, 1, ld), arr(T * Cn, dh, Cn, 1), 1.0), "alsep_nn_bgemm")
        p, _, _ = self._conv(res, G * T, 1, P["proj"])
        return self._scale_add(x, p, None, G * T, Cn)



class HDemucs(DConvOps):
    precision = "f32"
    pads_to_segment = False      # demucs' apply_model feeds a model without valid_length its chunks as they are

    def __init__(self, cfg: HDemucsConfig, state_dict: Dict[str, torch.Tensor], ctx: Optional[Context] = None):
        DConvOps.__init__(self, ctx if ctx is not None else _lib.default_context(None))
        self.cfg = cfg
        self.norm_groups = cfg.norm_groups
        check_config(cfg)
        self.plan = layer_plan(cfg)
        from .roformer import check_shapes
        check_shapes(state_dict, expected_shapes(cfg), "HDemucs",
                     ((f"encoder.{cfg.depth}.", f"depth={cfg.depth}"), ("encoder.0.dconv.layers.%d." % cfg.dconv_depth, f"dconv_depth={cfg.dconv_depth}")))
        try:
            self._build(state_dict)
        except KeyError as e:
            raise AlsepError(f"state_dict is missing {e} for this HDemucsConfig") from e

    def on_stream(self, ctx: Context) -> "HDemucs":
        """a view that launches on another context of the same device: the weights are shared, the caches are the view's own"""
        import copy
        if ctx.device != self.ctx.device:
            raise AlsepError("HDemucs.on_stream: the other context must be on the same device")
        v = copy.copy(self)
        v.ctx = ctx
        v._plans, v._ws, v._gn = {}, None, None
        return v

    def as_f32(self) -> "HDemucs":
        return self

    # -- parameters ---------------------------------------------------------------------------------------------
    def _build(self, sd) -> None:
        cfg, ctx = self.cfg, self.ctx

        def conv2d(p):          # Conv2d [Cout, Cin, KH, KW] -> [KH][KW][Cin][Cout]
            return _Conv(ctx, sd[p + ".weight"].permute(2, 3, 1, 0), sd.get(p + ".bias"))

        def conv1d(p):          # Conv1d [Cout, Cin, K] along H (time-major rows), W = 1
            return _Conv(ctx, sd[p + ".weight"].permute(2, 1, 0)[:, None], sd.get(p + ".bias"))

        def conv_along_w(p):    # Conv1d along T of [Fr, T, C] (the DConv of the frequency branch)
            return _Conv(ctx, sd[p + ".weight"].permute(2, 1, 0)[None], sd.get(p + ".bias"))

        def tconv(p):           # ConvTranspose [Cin, Cout, K(,1)] -> 1x1 conv to K * Cout columns (k-major), bias kept for the fold
            w = sd[p + ".weight"]
            w = w[..., 0] if w.dim() == 4 else w
            cin, cout, k = w.shape
            return dict(tr=_Conv(ctx, w.permute(0, 2, 1).reshape(cin, k * cout)[None, None], None), bias=self._vec(sd[p + ".bias"]), cout=cout,
                        k=k)

        def norm(p, on):
            return (self._vec(sd[p + ".weight"]), self._vec(sd[p + ".bias"])) if on else None

        def dconv(p, L: _Layer, freq: bool):
            pos = _dconv_index(L.lstm, L.attn)
            layers = []
            for d in range(cfg.dconv_depth):
                q = f"{p}.layers.{d}"
                mk = conv_along_w if freq else conv1d
                D = dict(c1=mk(q + ".0"), g1=self._vec(sd[q + ".1.weight"]), b1=self._vec(sd[q + ".1.bias"]),
                         c2=mk(f"{q}.{pos['conv2']}"), g2=self._vec(sd[f"{q}.{pos['norm2']}.weight"]), b2=self._vec(sd[f"{q}.{pos['norm2']}.bias"]),
                         scale=self._vec(sd[f"{q}.{pos['scale']}.scale"]), dil=2 ** d, lstm=None, attn=None)
                if L.lstm:
                    D["lstm"] = blstm_params(ctx, sd, f"{q}.{pos['lstm']}")
                if L.attn:
                    D["attn"] = localstate_params(ctx, sd, f"{q}.{pos['attn']}")
                layers.append(D)
            return layers

        n_freq = sum(L.freq for L in self.plan)
        self.enc, self.dec, self.tenc, self.tdec = [], [], [], []
        for L in self.plan:
            i, di = L.index, cfg.depth - 1 - L.index
            fr = L.freq
            self.enc.append(dict(conv=conv2d(f"encoder.{i}.conv") if fr else conv1d(f"encoder.{i}.conv"),
                                 rewrite=conv2d(f"encoder.{i}.rewrite") if fr else conv1d(f"encoder.{i}.rewrite"),
                                 norm1=norm(f"encoder.{i}.norm1", L.norm), norm2=norm(f"encoder.{i}.norm2", L.norm),
                                 dconv=dconv(f"encoder.{i}.dconv", L, fr) if cfg.dconv_mode & 1 else None))
            self.dec.append(dict(rewrite=conv2d(f"decoder.{di}.rewrite") if fr else conv1d(f"decoder.{di}.rewrite"),
                                 norm1=norm(f"decoder.{di}.norm1", L.norm), norm2=norm(f"decoder.{di}.norm2", L.norm),
                                 dconv=dconv(f"decoder.{di}.dconv", L, fr) if cfg.dconv_mode & 2 else None, **tconv(f"decoder.{di}.conv_tr")))
            if not fr:
                self.tenc.append(None)
                self.tdec.append(None)
                continue
            ti = n_freq - 1 - i
            te = dict(conv=conv1d(f"tencoder.{i}.conv"))
            td = dict(norm2=norm(f"tdecoder.{ti}.norm2", L.norm), **tconv(f"tdecoder.{ti}.conv_tr"))
            if not L.last_freq:
                te.update(rewrite=conv1d(f"tencoder.{i}.rewrite"), norm1=norm(f"tencoder.{i}.norm1", L.norm),
                          norm2=norm(f"tencoder.{i}.norm2", L.norm), dconv=dconv(f"tencoder.{i}.dconv", L, False) if cfg.dconv_mode & 1 else None)
                td.update(rewrite=conv1d(f"tdecoder.{ti}.rewrite"), norm1=norm(f"tdecoder.{ti}.norm1", L.norm),
                          dconv=dconv(f"tdecoder.{ti}.dconv", L, False) if cfg.dconv_mode & 2 else None)
            self.tenc.append(te)
            self.tdec.append(td)
        self.freq_emb = self._vec(sd["freq_emb.embedding.weight"] * cfg.emb_scale)

    def _dconv(self, y: torch.Tensor, G: int, T: int, Cn: int, layers, freq: bool) -> torch.Tensor:
        """demucs DConv on G sequences of T steps, y [G, T, C] (freq: the (sample, frequency) rows of [B, Fr, T, C]; time: the samples)"""
        rows = G * T
        for L in layers:
            d = L["dil"]
            if freq:
                hh, _, _ = self._conv(y, G, T, L["c1"], pad=(0, d), dil=(1, d))
            else:
                hh, _, _ = self._conv(y, T, 1, L["c1"], pad=(d, 0), dil=(d, 1), B=G)
            hh = self._norm(hh, G, T, L["c1"].cout, L["g1"], L["b1"], ACT_GELU)
            hid = L["c1"].cout
            if L["lstm"] is not None:
                hh = self._blstm(hh, G, T, L["lstm"])
            if L["attn"] is not None:
                hh = self._local_state(hh, G, T, hid, L["attn"])
            hh, _, _ = self._conv(hh, rows, 1, L["c2"])
            hh = self._norm(hh, G, T, L["c2"].cout, L["g2"], L["b2"], ACT_GLU)
            y = self._scale_add(y, hh, L["scale"], rows, Cn)
        return y

    def _pad_rows(self, x: torch.Tensor, B: int, T: int, Tp: int, Cn: int) -> torch.Tensor:
        """[B, T, C] -> [B, Tp, C] with zero rows T .. Tp-1 (HEncLayer's right padding to a multiple of the stride)"""
        if Tp == T:
            return x
        buf = self.ctx.zeros((B, Tp, Cn))
        buf[:, :T] = x.view(B, T, Cn)
        return buf

    def _enc(self, x: torch.Tensor, B: int, Fr: int, T: int, Cin: int, P, L: _Layer, freq: bool, inject: Optional[torch.Tensor] = None,
             empty: bool = False):
        """HEncLayer.forward.  freq: x [B, Fr, T, Cin] -> ([B, Fr', T, C], Fr'); otherwise x [B, T, Cin] -> ([B, T', C], T')"""
        cfg = self.cfg
        cv = P["conv"]
        # GELU straight in the convolution's epilogue unless a norm or the injected time branch comes first
        fused = not empty and inject is None and not P["norm1"]
        act = ACT_GELU if fused else ACT_NONE
        if freq:
            y, Fo, _ = self._conv(x, Fr, T, cv, stride=(L.stri, 1), pad=(L.pad, 0), act=act, B=B)
            H, W = Fo, T
        else:
            ker, stri = (cfg.kernel_size, cfg.stride) if L.freq else (L.ker, L.stri)
            Tp = -(-T // stri) * stri
            x = self._pad_rows(x, B, T, Tp, Cin)
            y, Fo, _ = self._conv(x, Tp, 1, cv, stride=(stri, 1), pad=(ker // 4, 0), act=act, B=B)
            H, W = Fo, 1
        if empty:
            return y, Fo
        rows = B * H * W
        if inject is not None:
            y = self._scale_add(y, inject, None, rows, cv.cout)
        if P["norm1"]:
            y = self._group_norm(y, B, H * W, cv.cout, P["norm1"], ACT_GELU)
        elif not fused:
            y = self._act(y, rows, cv.cout, ACT_GELU)
        if P["dconv"] is not None:
            y = self._dconv(y, B * H, W, cv.cout, P["dconv"], True) if freq else self._dconv(y, B, H, cv.cout, P["dconv"], False)
        ce = cfg.context_enc
        if freq:
            z, _, _ = self._conv(y, H, W, P["rewrite"], pad=(ce, ce), B=B)
        else:
            z, _, _ = self._conv(y, H, 1, P["rewrite"], pad=(ce, 0), B=B)
        z = self._group_norm(z, B, H * W, 2 * cv.cout, P["norm2"], ACT_GLU) if P["norm2"] else self._act(z, rows, 2 * cv.cout, ACT_GLU)
        return z, Fo

    def _dec(self, x: torch.Tensor, skip: Optional[torch.Tensor], B: int, Fr: int, T: int, P, L: _Layer, freq: bool, length: int, last: bool,
             empty: bool = False):
        """HDecLayer.forward.  freq: x [B, Fr, T, C] -> (z [B, Fr', T, Cout], pre); otherwise x [B, T, C] -> (z [B, length, Cout], pre)"""
        ctx, cfg = self.ctx, self.cfg
        cin = P["tr"].cin
        H, W = (Fr, T) if freq else (T, 1)
        rows = B * H * W
        if empty:
            y = x
        else:
            x = x if skip is None else self._scale_add(x, skip, None, rows, cin)
            c = cfg.context
            if freq:
                r, _, _ = self._conv(x, H, W, P["rewrite"], pad=(c, c), B=B)
            else:
                r, _, _ = self._conv(x, H, 1, P["rewrite"], pad=(c, 0), B=B)
            y = self._group_norm(r, B, H * W, 2 * cin, P["norm1"], ACT_GLU) if P["norm1"] else self._act(r, rows, 2 * cin, ACT_GLU)
            if P["dconv"] is not None:
                y = self._dconv(y, B * H, W, cin, P["dconv"], True) if freq else self._dconv(y, B, H, cin, P["dconv"], False)
        g, _, _ = self._conv(y, rows, 1, P["tr"])
        K, cout = P["k"], P["cout"]
        S = K // 2                                       # K = 2 S (or the last frequency layer's K on one bin: the fold's first half-kernel)
        pad = (L.pad if freq else cfg.kernel_size // 4 if L.freq else L.ker // 4)
        Lfull = (H - 1) * S + K
        Lout = Lfull - 2 * pad if freq else length
        act = ACT_NONE if last else ACT_GELU
        norm2 = P.get("norm2")
        if norm2 is None:
            z = ctx.empty((B * Lout * W, cout))
            ctx.check(ctx.lib.alsep_nn_tconv_fold(ctx.handle, _lib.ptr(g), _lib.ptr(P["bias"]), _lib.ptr(z), B, H, W, cout, S, pad, Lout, act),
                      "alsep_nn_tconv_fold")
            return z, y
        full = ctx.empty((B * Lfull * W, cout))
        ctx.check(ctx.lib.alsep_nn_tconv_fold(ctx.handle, _lib.ptr(g), _lib.ptr(P["bias"]), _lib.ptr(full), B, H, W, cout, S, 0, Lfull, ACT_NONE),
                  "alsep_nn_tconv_fold")
        return self._group_norm(full, B, Lfull * W, cout, norm2, act, pad * W, Lout * W), y

    # -- forward ------------------------------------------------------------------------------------------------
    def forward(self, mix: torch.Tensor) -> torch.Tensor:
        """HDemucs.forward (eval): mix [2, L] or [B, 2, L] float32 on the device -> [S, 2, L] / [B, S, 2, L]"""
        ctx, cfg = self.ctx, self.cfg
        lib, h = ctx.lib, ctx.handle
        single = mix.dim() == 2
        if single:
            mix = mix[None]
        if mix.dim() != 3 or mix.shape[1] != 2 or mix.dtype != torch.float32:
            raise AlsepError("HDemucs.forward expects a float32 [2, L] or [B, 2, L] tensor")
        mix = mix.contiguous()
        B, L = int(mix.shape[0]), int(mix.shape[-1])
        hl, nfft, S = cfg.hop, cfg.nfft, cfg.S
        le = -(-L // hl)
        pad = hl // 2 * 3
        right = pad + le * hl - L
        src, n = mix, L
        if n <= max(pad, right):                          # demucs pad1d: zeros first where the input is shorter than the reflection
            extra = max(pad, right) - n + 1
            er = min(right, extra)
            el = extra - er
            src = ctx.zeros((B, 2, n + extra))
            src[..., el:el + n] = mix
            n += extra
            pl, pr = pad - el, right - er
        else:
            pl, pr = pad, right
        Lp = n + pl + pr
        xp = ctx.empty((B, 2, Lp))
        ctx.check(lib.alsep_nn_reflect_pad(h, _lib.ptr(src), _lib.ptr(xp), 2 * B, n, pl, pr), "alsep_nn_reflect_pad")
        Tt, Fq = le + 4, nfft // 2
        plan = self._plan(Tt)
        spec = plan.stft_strided(xp, Lp, 2 * Lp, B, torch.float32, _lib.LAYOUT_REF)            # [B, 4, Fq, Tt]
        nx = Fq * le * 4
        x = ctx.empty((B * Fq * le, 4))
        ctx.check(lib.alsep_demucs_spec_in(h, _lib.ptr(spec), _lib.ptr(x), B, Fq, Tt, le, 2, 1.0 / math.sqrt(nfft)), "alsep_demucs_spec_in")
        stats = self._meanstd_b(x, B, nx)
        xn = torch.empty_like(x)
        ctx.check(lib.alsep_nn_affine_stats(h, _lib.ptr(x), _lib.ptr(xn), _lib.ptr(stats), B, nx, 1e-5, 0), "alsep_nn_affine_stats")
        x = xn
        xt = ctx.empty((B * L, 2))
        ctx.check(lib.alsep_nn_swap_last2(h, _lib.ptr(mix), _lib.ptr(xt), B, 2, L), "alsep_nn_swap_last2")
        stats_t = self._meanstd_b(xt, B, 2 * L)
        xtn = torch.empty_like(xt)
        ctx.check(lib.alsep_nn_affine_stats(h, _lib.ptr(xt), _lib.ptr(xtn), _lib.ptr(stats_t), B, 2 * L, 1e-5, 0), "alsep_nn_affine_stats")
        xt = xtn

        saved, saved_t, lengths, lengths_t = [], [], [], []
        Fr, Tx, Lt = Fq, le, L               # frequency rows and frames of the frequency / merged branch; time-branch length
        cx, ct = 4, 2
        for L_ in self.plan:
            i = L_.index
            inject = None
            if L_.freq:
                lengths.append(Tx)
                lengths_t.append(Lt)
                te = self.tenc[i]
                xt, Lt = self._enc(xt, B, 1, Lt, ct, te, L_, False, empty=L_.last_freq)
                ct = te["conv"].cout
                if L_.last_freq:
                    inject = xt
                else:
                    saved_t.append((xt, Lt))
                x, Fr = self._enc(x, B, Fr, Tx, cx, self.enc[i], L_, True, inject=inject)
            else:
                lengths.append(Tx)
                x, Tx = self._enc(x, B, 1, Tx, cx, self.enc[i], L_, False)
            cx = self.enc[i]["conv"].cout
            if i == 0:
                ctx.check(lib.alsep_nn_add_bcast(h, _lib.ptr(x), _lib.ptr(self.freq_emb), cfg.freq_emb, B * Fr * Tx * cx, Tx * cx, Fr, cx),
                          "alsep_nn_add_bcast")
            saved.append((x, Fr if L_.freq else 1, Tx))
        x = None
        for L_ in reversed(self.plan):
            i = L_.index
            last = i == 0
            skip, Fs, Ts = saved.pop(-1)
            length = lengths.pop(-1)
            P = self.dec[i]
            if L_.freq:
                x, pre = self._dec(skip if x is None else x, None if x is None else skip, B, Fs, Ts, P, L_, True, 0, last)
                length_t = lengths_t.pop(-1)
                td = self.tdec[i]
                if L_.last_freq:
                    xt = self._dec(pre, None, B, 1, Ts, td, L_, False, length_t, last, empty=True)[0]
                else:
                    skip_t, Ls = saved_t.pop(-1)
                    xt = self._dec(xt, skip_t, B, 1, Ls, td, L_, False, length_t, last)[0]
            else:
                x, _ = self._dec(skip if x is None else x, None if x is None else skip, B, 1, Ts, P, L_, False, length, last)
        spec_out = ctx.empty((B * S, 4, Fq, Tt))
        ctx.check(lib.alsep_demucs_spec_out(h, _lib.ptr(x), _lib.ptr(stats), _lib.ptr(spec_out), B, S, Fq, Tt, le, 2, math.sqrt(nfft)),
                  "alsep_demucs_spec_out")
        xs = ctx.empty((B * S, 2, L))
        plan.istft_strided(spec_out, _lib.LAYOUT_REF, xs, L, 2 * L, pad, pad + L, (B * S - 1) * 2 * L + L)
        out = ctx.empty((B, S, 2, L))
        ctx.check(lib.alsep_demucs_mix_out(h, _lib.ptr(xt), _lib.ptr(stats_t), _lib.ptr(xs), _lib.ptr(out), B, S, L), "alsep_demucs_mix_out")
        return out[0] if single else out

    __call__ = forward


# ---- synthetic weights (data only: random-init parameters with demucs' names and shapes; bench / tests, allow_synthetic=True) ----
def synthetic_state_dict(cfg: HDemucsConfig, seed: int = 0) -> Dict[str, torch.Tensor]:
    g = torch.Generator().manual_seed(seed)
    sd: Dict[str, torch.Tensor] = {}
    for name, (shape, _) in expected_shapes(cfg).items():
        if name.endswith(".scale"):                                   # LayerScale: demucs inits 1e-4; larger so the branch matters
            sd[name] = torch.full(shape, 0.2) * (0.5 + torch.rand(shape, generator=g))
        elif len(shape) == 1 and name.endswith(".weight"):            # norms
            sd[name] = 1.0 + 0.1 * (torch.rand(shape, generator=g) * 2 - 1)
        elif ".lstm." in name:                                        # torch.nn.LSTM: U(-1/sqrt(H), 1/sqrt(H))
            sd[name] = (torch.rand(shape, generator=g) * 2 - 1) / math.sqrt(shape[0] // 4)
        elif len(shape) == 1:                                         # biases
            sd[name] = 0.05 * (torch.rand(shape, generator=g) * 2 - 1)
        else:
            fan = int(torch.tensor(shape[1:]).prod())
            sd[name] = (torch.rand(shape, generator=g) * 2 - 1) / math.sqrt(fan)
        if ".query_decay." in name and name.endswith(".bias"):        # demucs: -2 (a wide initial window); spread around it
            sd[name] = -2.0 + 2.0 * (torch.rand(shape, generator=g) * 2 - 1)
    return sd
