"""RMVPE pitch extraction on the GPU: the ``RMVPE`` class of the reference (modules/rvc/infer/lib/rmvpe.py), the f0 tracker behind Clone's
default ``rmvpe+`` method, with the reference's surface so that a ``FeatureExtractor``-style caller takes it unchanged.

  1. log-mel front end (rmvpe.py:475-555, :113-149): 16 kHz, reflect-pad 512, frames of 1024 every 160, periodic Hann, float32 magnitude
     of 513 bins, HTK mel filterbank 30 .. 8000 Hz (128 bands, Slaney area normalisation), log(max(., 1e-5)): one kernel (csrc/rmvpe.h);
  2. the frame axis reflected up to a multiple of 32 (rmvpe.py:608-622), the network's input BatchNorm folded into the same pass;
  3. the U-Net ``E2E(4, 1, (2, 2))`` (rmvpe.py:232-469), channels-last ``[1, frames, 128, C]``: 3x3 / 1x1 convolutions + folded BatchNorm +
     ReLU on ``alsep_nn_conv2d`` in its exact float32 contraction, the 2x2 average pool and the stride-2 transposed convolution on their
     own kernels, the latter writing straight into its half of the concatenation with the skip;
  4. the BiGRU 384 -> 256 (one GEMM for the input projection of both directions, one launch for the recurrence), Linear 512 -> 360, sigmoid;
  5. the decode (rmvpe.py:624-628, :669-687): argmax, the local weighted mean of the cents in float64, f0 = 10 2^(cents / 1200).

Float32 only (``is_half`` and ``onnx`` raise); ``keyshift = 0``, ``speed = 1`` only.  The whole track goes through in one pass, as in the
reference: chunking would change the GRU's result.  The mel filterbank comes from ``librosa.filters.mel`` in the reference; librosa is not
available, so ``mel_filterbank_htk`` is the published formula restated, parity unpinned (tests/test_rmvpe_oracle.py pins it to its closed form).
Tracks too short for torch's reflection (512 samples or fewer) follow numpy's repeated reflection in the front end, but the network needs
at least 17 frames (2560 samples): below that the reference's frame padding cannot be reflected either, and ``mel2hidden`` raises.
"""
from __future__ import annotations

import ctypes as C
import functools
import os
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import AlsepError, Context

SAMPLE_RATE, N_FFT, HOP, N_MELS, N_CLASS = 16000, 1024, 160, 128, 360
BINS = N_FFT // 2 + 1
MEL_FMIN, MEL_FMAX = 30.0, 8000.0
GRU_HIDDEN = 256
BN_EPS = 1e-5
MAX_FRAMES = 1 << 20                                                          # kRvMaxFrames of csrc/rmvpe.h
CENTS_OFFSET = 1997.3794084376191


@dataclass(frozen=True)
class RMVPEConfig:
    """the constructor arguments of the reference's ``E2E``; the default is what ``RMVPE`` builds, ``E2E(4, 1, (2, 2))``"""
    n_blocks: int = 4
    n_gru: int = 1
    kernel_size: Tuple[int, int] = (2, 2)
    en_de_layers: int = 5
    inter_layers: int = 4
    in_channels: int = 1
    en_out_channels: int = 16

    def check(self) -> None:
        if tuple(self.kernel_size) != (2, 2):
            raise AlsepError(f"rmvpe: kernel_size {self.kernel_size} not built (RMVPE uses (2, 2); the stride (1, 2) decoder is not reachable from it)")
        if self.n_gru != 1:
            raise AlsepError(f"rmvpe: n_gru = {self.n_gru} not built (RMVPE uses one BiGRU layer)")
        if self.in_channels != 1:
            raise AlsepError(f"rmvpe: in_channels = {self.in_channels} not built (the input is the one-channel log-mel)")
        if self.n_blocks < 1 or self.en_de_layers < 1 or self.inter_layers < 1 or self.en_out_channels < 4 or self.en_out_channels % 4:
            raise AlsepError(f"rmvpe: configuration {self} not built (channels in multiples of 4, at least one block / level / layer)")
        if N_MELS % (1 << self.en_de_layers):
            raise AlsepError(f"rmvpe: {self.en_de_layers} levels do not divide the {N_MELS} mel bands")


# ---- the state dict of E2E -------------------------------------------------------------------------------------------------------------
def _bn_shapes(out: Dict[str, tuple], p: str, c: int) -> None:
    for k in ("weight", "bias", "running_mean", "running_var"):
        out[f"{p}.{k}"] = (c,)
    out[f"{p}.num_batches_tracked"] = ()


def _block_shapes(out: Dict[str, tuple], p: str, ci: int, co: int) -> None:
    """ConvBlockRes: conv.0 / conv.3 (3x3, no bias), conv.1 / conv.4 (BatchNorm2d), shortcut (1x1, biased) where the channels change"""
    out[f"{p}.conv.0.weight"] = (co, ci, 3, 3)
    _bn_shapes(out, f"{p}.conv.1", co)
    out[f"{p}.conv.3.weight"] = (co, co, 3, 3)
    _bn_shapes(out, f"{p}.conv.4", co)
    if ci != co:
        out[f"{p}.shortcut.weight"] = (co, ci, 1, 1)
        out[f"{p}.shortcut.bias"] = (co,)


def param_shapes(cfg: RMVPEConfig = RMVPEConfig()) -> Dict[str, tuple]:
    """name -> shape of every tensor of ``E2E(...).state_dict()``, in its order"""
    cfg.check()
    out: Dict[str, tuple] = {}
    _bn_shapes(out, "unet.encoder.bn", cfg.in_channels)
    ci, co = cfg.in_channels, cfg.en_out_channels
    for i in range(cfg.en_de_layers):
        for b in range(cfg.n_blocks):
            _block_shapes(out, f"unet.encoder.layers.{i}.conv.{b}", ci if b == 0 else co, co)
        ci, co = co, co * 2
    top = co                                                                 # Encoder.out_channel
    ci = top // 2
    for i in range(cfg.inter_layers):
        for b in range(cfg.n_blocks):
            _block_shapes(out, f"unet.intermediate.layers.{i}.conv.{b}", ci if b == 0 else top, top)
        ci = top
    ci = top
    for i in range(cfg.en_de_layers):
        co = ci // 2
        out[f"unet.decoder.layers.{i}.conv1.0.weight"] = (ci, co, 3, 3)
        _bn_shapes(out, f"unet.decoder.layers.{i}.conv1.1", co)
        for b in range(cfg.n_blocks):
            _block_shapes(out, f"unet.decoder.layers.{i}.conv2.{b}", 2 * co if b == 0 else co, co)
        ci = co
    out["cnn.weight"] = (3, cfg.en_out_channels, 3, 3)
    out["cnn.bias"] = (3,)
    for suffix in ("", "_reverse"):
        out[f"fc.0.gru.weight_ih_l0{suffix}"] = (3 * GRU_HIDDEN, 3 * N_MELS)
        out[f"fc.0.gru.weight_hh_l0{suffix}"] = (3 * GRU_HIDDEN, GRU_HIDDEN)
        out[f"fc.0.gru.bias_ih_l0{suffix}"] = (3 * GRU_HIDDEN,)
        out[f"fc.0.gru.bias_hh_l0{suffix}"] = (3 * GRU_HIDDEN,)
    out["fc.1.weight"] = (N_CLASS, 2 * GRU_HIDDEN)
    out["fc.1.bias"] = (N_CLASS,)
    return out


def synthetic_state_dict(cfg: RMVPEConfig = RMVPEConfig(), seed: int = 0) -> Dict[str, torch.Tensor]:
    """seeded random-init weights for any configuration (tests, benchmarks, ``allow_synthetic``), drawn from ``np.random.default_rng(seed)``
    in the state dict's order.  The draw keeps the network non-degenerate at its full depth: convolutions at He scale, the BatchNorm scale
    of every residual branch around 0.3 (56 residual blocks would double the variance each at 1), the input BatchNorm centred on the log-mel's
    range, the last convolution at a tenth of the unit gain so that the GRU stays out of saturation, and the last Linear at 4 times torch's
    default so that the salience has a clear peak in most frames without saturating the sigmoid."""
    rng = np.random.default_rng(seed)
    sd: Dict[str, torch.Tensor] = {}
    for name, shape in param_shapes(cfg).items():
        leaf = name.rsplit(".", 1)[1]
        tail = tuple(name.split(".")[-3:-1])                                 # (container, index) of the module that owns the tensor
        is_bn = tail in (("conv", "1"), ("conv", "4"), ("conv1", "1"))
        if leaf == "num_batches_tracked":
            sd[name] = torch.tensor(1000, dtype=torch.int64)
            continue
        if name.startswith("unet.encoder.bn."):
            v = {"weight": 1.0, "bias": 0.0, "running_mean": -4.0, "running_var": 9.0}[leaf] + 0.05 * rng.standard_normal(shape)
        elif leaf == "running_var":
            v = rng.uniform(0.8, 1.2, shape)
        elif leaf == "running_mean":
            v = 0.1 * rng.standard_normal(shape)
        elif is_bn:                                                          # BatchNorm weight / bias
            branch = tail == ("conv", "4")                                   # the last BatchNorm of a residual branch
            v = rng.uniform(0.2, 0.4, shape) if (leaf == "weight" and branch) else rng.uniform(0.8, 1.2, shape) if leaf == "weight" else \
                0.05 * rng.standard_normal(shape)
        elif "gru" in name:
            v = rng.uniform(-1.0, 1.0, shape) / np.sqrt(GRU_HIDDEN)
        elif name.startswith("fc.1."):
            v = 4.0 * rng.uniform(-1.0, 1.0, shape) / np.sqrt(2 * GRU_HIDDEN)
        elif leaf == "bias":
            v = 0.05 * rng.standard_normal(shape)
        elif tail == ("conv1", "0"):                                          # ConvTranspose2d [ci, co, 3, 3]: 2.25 taps reach an output pixel
            v = rng.standard_normal(shape) * np.sqrt(2.0 / (2.25 * shape[0]))
        elif name == "cnn.weight":                                           # a tenth of the unit gain: the GRU stays out of saturation
            v = 0.1 * rng.standard_normal(shape) / np.sqrt(shape[1] * 9)
        elif ".shortcut." in name:
            v = rng.standard_normal(shape) / np.sqrt(shape[1])
        else:                                                                # Conv2d [co, ci, 3, 3] in front of a ReLU
            v = rng.standard_normal(shape) * np.sqrt(2.0 / (shape[1] * 9))
        sd[name] = torch.from_numpy(np.asarray(v, dtype=np.float32).reshape(shape))
    return sd


def check_state_dict(sd: Dict[str, torch.Tensor], cfg: RMVPEConfig = RMVPEConfig()) -> None:
    """every tensor's name and shape against the configuration; AlsepError names the first that does not fit"""
    want = param_shapes(cfg)
    for name, shape in want.items():
        if name not in sd:
            raise AlsepError(f"rmvpe: the state dict has no tensor {name}")
        if tuple(sd[name].shape) != tuple(shape):
            raise AlsepError(f"rmvpe: tensor {name} has shape {tuple(sd[name].shape)}, the configuration needs {tuple(shape)}")
    extra = [k for k in sd if k not in want]
    if extra:
        raise AlsepError(f"rmvpe: the state dict has a tensor the configuration does not know: {extra[0]}")


# ---- the front end's tables ---------------------------------------------------------------------------------------------------------------
def hz_to_mel_htk(f):
    return 2595.0 * np.log10(1.0 + np.asarray(f, dtype=np.float64) / 700.0)


def mel_to_hz_htk(m):
    return 700.0 * (10.0 ** (np.asarray(m, dtype=np.float64) / 2595.0) - 1.0)


def mel_points_htk(n_mels: int = N_MELS, fmin: float = MEL_FMIN, fmax: float = MEL_FMAX) -> np.ndarray:
    """the ``n_mels + 2`` triangle corners in Hz: equally spaced on the HTK mel scale"""
    return mel_to_hz_htk(np.linspace(hz_to_mel_htk(fmin), hz_to_mel_htk(fmax), n_mels + 2))


@functools.lru_cache(maxsize=None)
def mel_filterbank_htk(sr: int = SAMPLE_RATE, n_fft: int = N_FFT, n_mels: int = N_MELS, fmin: float = MEL_FMIN, fmax: float = MEL_FMAX) -> np.ndarray:
    """float32 ``[n_mels, n_fft / 2 + 1]``: triangles over neighbouring corners, each scaled by 2 / its width in Hz (what
    ``librosa.filters.mel(htk=True)`` publishes; parity unpinned)"""
    freqs = np.linspace(0.0, sr / 2.0, n_fft // 2 + 1)
    f = mel_points_htk(n_mels, fmin, fmax)
    fb = np.zeros((n_mels, n_fft // 2 + 1), dtype=np.float64)
    for m in range(n_mels):
        rise = (freqs - f[m]) / (f[m + 1] - f[m])
        fall = (f[m + 2] - freqs) / (f[m + 2] - f[m + 1])
        fb[m] = np.maximum(0.0, np.minimum(rise, fall)) * (2.0 / (f[m + 2] - f[m]))
    return fb.astype(np.float32)


def hann_window() -> np.ndarray:
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N_FFT, dtype=np.float64) / N_FFT)).astype(np.float32)


def _twiddle() -> np.ndarray:
    ang = 2.0 * np.pi * np.arange(N_FFT // 2, dtype=np.float64) / N_FFT
    tw = np.stack([np.cos(ang), -np.sin(ang)], axis=1)
    tw[0], tw[N_FFT // 4] = (1.0, 0.0), (0.0, -1.0)
    return np.ascontiguousarray(tw.astype(np.float32))


def _bands(fb: np.ndarray) -> np.ndarray:
    bands = np.zeros((fb.shape[0], 2), dtype=np.int32)
    for m in range(fb.shape[0]):
        nz = np.flatnonzero(fb[m])
        if len(nz):
            bands[m] = (nz[0], nz[-1] - nz[0] + 1)
    return bands


def _dev(ctx: Context, a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a)).to(ctx.device)


def frames_of(n: int) -> int:
    return n // HOP + 1


def pad_frames_of(T: int) -> int:
    """mel2hidden's right padding: up to the next multiple of 32, capped at T; AlsepError where that many frames cannot be reflected"""
    pad = min(32 * ((T - 1) // 32 + 1) - T, T)
    if pad > T - 1:
        raise AlsepError(f"rmvpe: {T} frames need {pad} reflected frames, more than the {T - 1} a reflection can give "
                         f"(at least 17 frames, {16 * HOP} samples)")
    return pad


# ---- stage wrappers -----------------------------------------------------------------------------------------------------------------------
def mel_frontend(ctx: Context, audio: torch.Tensor, want_linear: bool = False):
    """float32 ``[n]`` device tensor at 16 kHz -> the log-mel ``[T, 128]`` (frames major: the network's channels-last input), and with
    ``want_linear`` also the filterbank product before the clamp and the log"""
    n = int(audio.shape[0])
    T = int(ctx.lib.alsep_rmvpe_frames(n))
    if T < 0:
        raise AlsepError(f"rmvpe: {n} samples ({frames_of(max(n, 0))} frames); 1 sample .. {MAX_FRAMES} frames are taken")
    fb = mel_filterbank_htk()
    win, tw, basis, bands = (_dev(ctx, a) for a in (hann_window(), _twiddle(), fb, _bands(fb)))
    logm = ctx.empty((T, N_MELS))
    lin = ctx.empty((T, N_MELS)) if want_linear else None
    ctx.check(ctx.lib.alsep_rmvpe_mel(ctx.handle, _lib.ptr(audio), n, _lib.ptr(win), _lib.ptr(tw), _lib.ptr(basis), _lib.ptr(bands),
                                      _lib.ptr(lin), _lib.ptr(logm)), "alsep_rmvpe_mel")
    return (logm, lin) if want_linear else logm


def pad_frames(ctx: Context, x: torch.Tensor, Tp: int, scale: float = 1.0, shift: float = 0.0) -> torch.Tensor:
    """``[T, C]`` -> ``[Tp, C]``: reflected on the right, times ``scale`` plus ``shift``"""
    T, Cc = int(x.shape[0]), int(x.shape[1])
    y = ctx.empty((Tp, Cc))
    ctx.check(ctx.lib.alsep_rmvpe_pad_frames(ctx.handle, _lib.ptr(x), _lib.ptr(y), T, Tp, Cc, float(scale), float(shift)), "alsep_rmvpe_pad_frames")
    return y


def avgpool2(ctx: Context, x: torch.Tensor, cat: Optional[torch.Tensor] = None, cat_off: int = 0) -> torch.Tensor:
    """``[B, H, W, C]`` -> ``[B, H / 2, W / 2, C]``; ``x`` is also copied into channels ``cat_off ..`` of ``cat [B, H, W, Ct]`` when given"""
    B, H, W, Cc = (int(v) for v in x.shape)
    if H % 2 or W % 2:
        raise AlsepError(f"rmvpe: average pool of an odd image {H} x {W}")
    y = ctx.empty((B, H // 2, W // 2, Cc))
    ctx.check(ctx.lib.alsep_rmvpe_avgpool2(ctx.handle, _lib.ptr(x), _lib.ptr(y), B, H, W, Cc, _lib.ptr(cat), int(cat.shape[3]) if cat is not None else 0,
                                           int(cat_off)), "alsep_rmvpe_avgpool2")
    return y


def tconv3x3s2(ctx: Context, x: torch.Tensor, w: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, y: torch.Tensor, y_off: int = 0,
               act: int = 1) -> torch.Tensor:
    """``x [B, H, W, Cin]``, ``w [3, 3, Cin, Cout]`` -> channels ``y_off .. y_off + Cout`` of ``y [B, 2H, 2W, Ct]``"""
    B, H, W, Cin = (int(v) for v in x.shape)
    Cout = int(w.shape[3])
    if tuple(w.shape) != (3, 3, Cin, Cout) or tuple(y.shape[:3]) != (B, 2 * H, 2 * W):
        raise AlsepError(f"rmvpe: transposed convolution of {tuple(x.shape)} by {tuple(w.shape)} into {tuple(y.shape)}")
    ctx.check(ctx.lib.alsep_rmvpe_tconv3x3s2(ctx.handle, _lib.ptr(x), _lib.ptr(w), _lib.ptr(scale), _lib.ptr(shift), _lib.ptr(y), B, H, W, Cin, Cout,
                                             int(act), int(y.shape[3]), int(y_off)), "alsep_rmvpe_tconv3x3s2")
    return y


def gru(ctx: Context, pre: torch.Tensor, whh_t: torch.Tensor, bhh: torch.Tensor) -> torch.Tensor:
    """``pre [T, N, 6H]``, ``whh_t [2, H, 3H]``, ``bhh [2, 3H]`` -> ``h [T, N, 2H]``"""
    T, N, H6 = (int(v) for v in pre.shape)
    H = H6 // 6
    if tuple(whh_t.shape) != (2, H, 3 * H) or tuple(bhh.shape) != (2, 3 * H):
        raise AlsepError(f"rmvpe: GRU of {tuple(pre.shape)} with weights {tuple(whh_t.shape)}, {tuple(bhh.shape)}")
    h = ctx.empty((T, N, 2 * H))
    ctx.check(ctx.lib.alsep_nn_gru(ctx.handle, _lib.ptr(pre), _lib.ptr(whh_t), _lib.ptr(bhh), _lib.ptr(h), T, N, H), "alsep_nn_gru")
    return h


def decode_salience(ctx: Context, salience: torch.Tensor, thred: float = 0.03) -> torch.Tensor:
    """float32 ``[T, 360]`` on the device -> float64 ``[T]`` f0"""
    T = int(salience.shape[0])
    if salience.dim() != 2 or int(salience.shape[1]) != N_CLASS or T < 1 or T > MAX_FRAMES:
        raise AlsepError(f"rmvpe: salience of shape {tuple(salience.shape)} ([1 .. {MAX_FRAMES}, {N_CLASS}])")
    f0 = ctx.empty((T,), torch.float64)
    ctx.check(ctx.lib.alsep_rmvpe_decode(ctx.handle, _lib.ptr(salience), T, float(np.float32(thred)), _lib.ptr(f0)), "alsep_rmvpe_decode")
    return f0


# ---- the network --------------------------------------------------------------------------------------------------------------------------
def _fold_bn(sd, p: str) -> Tuple[torch.Tensor, torch.Tensor]:
    scale = sd[p + ".weight"].double() / torch.sqrt(sd[p + ".running_var"].double() + BN_EPS)
    shift = sd[p + ".bias"].double() - sd[p + ".running_mean"].double() * scale
    return scale.float(), shift.float()


class _Conv:
    """Conv2d packed ``[KH][KW][Cin][Cout]`` with the scale / shift of its folded BatchNorm, or 1 / its bias"""

    def __init__(self, ctx: Context, sd, key: str, bn: Optional[str], act: int):
        w = sd[key + ".weight"].float()
        self.cout, self.cin, self.k = int(w.shape[0]), int(w.shape[1]), int(w.shape[2])
        self.w = w.permute(2, 3, 1, 0).contiguous().to(ctx.device)
        if bn is not None:
            scale, shift = _fold_bn(sd, bn)
        else:
            scale, shift = torch.ones(self.cout), sd[key + ".bias"].float()
        self.scale, self.shift, self.act = scale.contiguous().to(ctx.device), shift.contiguous().to(ctx.device), act


class _Block:
    def __init__(self, ctx: Context, sd, p: str):
        self.c1 = _Conv(ctx, sd, p + ".conv.0", p + ".conv.1", 1)
        self.c2 = _Conv(ctx, sd, p + ".conv.3", p + ".conv.4", 1)
        self.short = _Conv(ctx, sd, p + ".shortcut", None, 0) if (p + ".shortcut.weight") in sd else None


class RMVPENet:
    """the host mirror of ``E2E``: weights packed on the device at construction, ``forward`` is launches only"""

    def __init__(self, state_dict: Dict[str, torch.Tensor], cfg: RMVPEConfig = RMVPEConfig(), ctx: Optional[Context] = None):
        cfg.check()
        check_state_dict(state_dict, cfg)
        self.cfg, self.ctx = cfg, ctx if ctx is not None else _lib.default_context(None)
        ctx, sd = self.ctx, state_dict
        s, b = _fold_bn(sd, "unet.encoder.bn")
        self.in_scale, self.in_shift = float(s[0]), float(b[0])
        self.encoder = [[_Block(ctx, sd, f"unet.encoder.layers.{i}.conv.{k}") for k in range(cfg.n_blocks)] for i in range(cfg.en_de_layers)]
        self.inter = [[_Block(ctx, sd, f"unet.intermediate.layers.{i}.conv.{k}") for k in range(cfg.n_blocks)] for i in range(cfg.inter_layers)]
        self.decoder = []
        for i in range(cfg.en_de_layers):
            p = f"unet.decoder.layers.{i}"
            w = sd[p + ".conv1.0.weight"].float().permute(2, 3, 0, 1).contiguous().to(ctx.device)      # [ci, co, ky, kx] -> [ky][kx][ci][co]
            scale, shift = (t.contiguous().to(ctx.device) for t in _fold_bn(sd, p + ".conv1.1"))
            self.decoder.append((w, scale, shift, [_Block(ctx, sd, f"{p}.conv2.{k}") for k in range(cfg.n_blocks)]))
        self.cnn = _Conv(ctx, sd, "cnn", None, 0)
        # the GRU reads frame t as [128 mel][3 channels] (channels-last) where the module flattens [3][128]: reorder W_ih's columns
        H = GRU_HIDDEN
        wih, bih, whh, bhh = [], [], [], []
        for suffix in ("", "_reverse"):
            w = sd[f"fc.0.gru.weight_ih_l0{suffix}"].float().reshape(3 * H, 3, N_MELS).permute(0, 2, 1).reshape(3 * H, 3 * N_MELS)
            wih.append(w)
            bih.append(sd[f"fc.0.gru.bias_ih_l0{suffix}"].float())
            whh.append(sd[f"fc.0.gru.weight_hh_l0{suffix}"].float().t())
            bhh.append(sd[f"fc.0.gru.bias_hh_l0{suffix}"].float())
        self.wih, self.bih = torch.cat(wih).contiguous().to(ctx.device), torch.cat(bih).contiguous().to(ctx.device)
        self.whh_t, self.bhh = torch.stack(whh).contiguous().to(ctx.device), torch.stack(bhh).contiguous().to(ctx.device)
        self.wfc, self.bfc = sd["fc.1.weight"].float().contiguous().to(ctx.device), sd["fc.1.bias"].float().contiguous().to(ctx.device)

    # -- launches --
    def _conv(self, L: _Conv, x: torch.Tensor) -> torch.Tensor:
        ctx = self.ctx
        B, H, W, ci = (int(v) for v in x.shape)
        y = ctx.empty((B, H, W, L.cout))
        pad = L.k // 2
        ctx.check(ctx.lib.alsep_nn_conv2d(ctx.handle, _lib.ptr(x), _lib.ptr(L.w), _lib.ptr(L.scale), _lib.ptr(L.shift), _lib.ptr(y), B, H, W, ci, L.cout,
                                          L.k, L.k, 1, 1, pad, pad, 1, 1, L.act, L.cout, 0), "alsep_nn_conv2d")
        return y

    def _block(self, blk: _Block, x: torch.Tensor) -> torch.Tensor:
        ctx = self.ctx
        t = self._conv(blk.c2, self._conv(blk.c1, x))
        res = self._conv(blk.short, x) if blk.short is not None else x
        y = ctx.empty(tuple(t.shape))
        ctx.check(ctx.lib.alsep_nn_scale_add(ctx.handle, _lib.ptr(t), _lib.ptr(res), None, _lib.ptr(y), t.numel() // int(t.shape[3]), int(t.shape[3])),
                  "alsep_nn_scale_add")
        return y

    def _gemm(self, a: torch.Tensor, rows: int, w: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
        ctx, arr = self.ctx, C.c_int64 * 4
        n, k = int(w.shape[0]), int(w.shape[1])
        y = ctx.empty((rows, n))
        ctx.check(ctx.lib.alsep_nn_bgemm_bias(ctx.handle, _lib.ptr(a), _lib.ptr(w), _lib.ptr(y), 1, 1, rows, n, k, arr(0, 0, k, 1), arr(0, 0, k, 1),
                                              arr(0, 0, n, 1), 1.0, _lib.ptr(bias), 0), "alsep_nn_bgemm_bias")
        return y

    def unet(self, x: torch.Tensor) -> torch.Tensor:
        """``[1, Tp, 128, 1]`` (after the input BatchNorm) -> ``[1, Tp, 128, 3]``, the output of ``cnn``"""
        ctx = self.ctx
        cats: List[torch.Tensor] = []
        for blocks in self.encoder:
            for blk in blocks:
                x = self._block(blk, x)
            B, H, W, c = (int(v) for v in x.shape)
            cat = ctx.empty((B, H, W, 2 * c))                                 # [transposed convolution | skip], as torch.cat((x, skip), 1)
            cats.append(cat)
            x = avgpool2(ctx, x, cat, c)
        for blocks in self.inter:
            for blk in blocks:
                x = self._block(blk, x)
        for (w, scale, shift, blocks), cat in zip(self.decoder, reversed(cats)):
            x = tconv3x3s2(ctx, x, w, scale, shift, cat, 0, 1)
            for blk in blocks:
                x = self._block(blk, x)
        return self._conv(self.cnn, x)

    def head(self, feat: torch.Tensor, T: int) -> torch.Tensor:
        """``[Tp, 384]`` (mel major, channel minor) -> the salience of the first ``T`` frames ``[T, 360]``; the GRU runs over all ``Tp``"""
        ctx = self.ctx
        Tp = int(feat.shape[0])
        pre = self._gemm(feat, Tp, self.wih, self.bih)
        h = gru(ctx, pre.view(Tp, 1, 6 * GRU_HIDDEN), self.whh_t, self.bhh)
        sal = self._gemm(h, T, self.wfc, self.bfc)
        ctx.check(ctx.lib.alsep_rmvpe_sigmoid(ctx.handle, _lib.ptr(sal), sal.numel()), "alsep_rmvpe_sigmoid")
        return sal

    def forward(self, logmel: torch.Tensor) -> torch.Tensor:
        """the log-mel ``[T, 128]`` on the device -> the salience ``[T, 360]`` (``mel2hidden`` in the network's own layout)"""
        T = int(logmel.shape[0])
        if logmel.dim() != 2 or int(logmel.shape[1]) != N_MELS or T < 1 or T > MAX_FRAMES:
            raise AlsepError(f"rmvpe: a log-mel of shape {tuple(logmel.shape)} ([1 .. {MAX_FRAMES} frames, {N_MELS}]: the kernels index "
                             f"up to {MAX_FRAMES} frames)")
        Tp = T + pad_frames_of(T)
        if Tp % (1 << self.cfg.en_de_layers):
            raise AlsepError(f"rmvpe: {Tp} padded frames are not a multiple of {1 << self.cfg.en_de_layers}")
        x = pad_frames(self.ctx, logmel.contiguous(), Tp, self.in_scale, self.in_shift).view(1, Tp, N_MELS, 1)
        y = self.unet(x)
        return self.head(y.view(Tp, 3 * N_MELS), T)


# ---- the reference's class ------------------------------------------------------------------------------------------------------------------
class RMVPE:
    """``RMVPE(model_path, is_half, onnx, device)`` of the reference, float32.  ``allow_synthetic``: a missing ``model_path`` gives seeded
    random-init weights (benchmarks and tests); ``config`` / ``seed``: the network and the seed of that draw."""

    def __init__(self, model_path, is_half: bool = False, onnx: bool = False, device=None, *, ctx: Optional[Context] = None,
                 allow_synthetic: bool = False, config: RMVPEConfig = RMVPEConfig(), seed: int = 0):
        if is_half:
            raise AlsepError("rmvpe: is_half=True not built (float32 only)")
        if onnx:
            raise AlsepError("rmvpe: onnx=True not built (the network runs on the HIP kernels)")
        if ctx is None:
            ctx = _lib.default_context(None) if device is None else Context(device)
        self.ctx, self.device, self.is_half, self.onnx = ctx, ctx.device, False, False
        if model_path is not None and os.path.exists(str(model_path)):
            sd = torch.load(str(model_path), map_location="cpu", weights_only=True)
        elif allow_synthetic:
            sd = synthetic_state_dict(config, seed)
        else:
            raise FileNotFoundError(f"rmvpe: {model_path} not found (allow_synthetic=True runs seeded random weights)")
        self.model = RMVPENet(sd, config, ctx)

    def _audio(self, audio) -> torch.Tensor:
        x = torch.as_tensor(audio)
        if x.dim() != 1:
            raise AlsepError(f"rmvpe: audio of shape {tuple(x.shape)}; mono [n] at {SAMPLE_RATE} Hz is taken")
        return x.to(self.ctx.device, torch.float32).contiguous()

    def mel_extractor(self, audio, keyshift=0, speed=1, center=True) -> torch.Tensor:
        """``[1, n]`` or ``[n]`` -> the log-mel ``[1, 128, T]`` as the reference's ``MelSpectrogram`` returns it"""
        if keyshift != 0 or speed != 1 or not center:
            raise AlsepError(f"rmvpe: keyshift = {keyshift}, speed = {speed}, center = {center} not built (0, 1, True only)")
        x = torch.as_tensor(audio)
        return mel_frontend(self.ctx, self._audio(x[0] if x.dim() == 2 else x)).t().unsqueeze(0)

    def mel2hidden(self, mel) -> torch.Tensor:
        """the log-mel ``[1, 128, T]`` (or ``[128, T]``) -> the salience ``[1, T, 360]`` on the device"""
        m = torch.as_tensor(mel).to(self.ctx.device, torch.float32)
        m = m[0] if m.dim() == 3 else m
        if m.dim() != 2 or int(m.shape[0]) != N_MELS:
            raise AlsepError(f"rmvpe: a mel of shape {tuple(torch.as_tensor(mel).shape)} ([1, {N_MELS}, T])")
        return self.model.forward(m.t().contiguous()).unsqueeze(0)

    def decode(self, hidden, thred: float = 0.03) -> np.ndarray:
        """the salience ``[T, 360]`` (array or tensor) -> float64 numpy f0 ``[T]``"""
        h = torch.as_tensor(hidden).to(self.ctx.device, torch.float32).contiguous()
        return decode_salience(self.ctx, h, thred).cpu().numpy()

    def _hidden(self, audio) -> torch.Tensor:
        return self.model.forward(mel_frontend(self.ctx, self._audio(audio)))

    def infer_from_audio(self, audio, thred: float = 0.03) -> np.ndarray:
        return decode_salience(self.ctx, self._hidden(audio), thred).cpu().numpy()

    def infer_from_audio_with_pitch(self, audio, thred: float = 0.03, f0_min=50, f0_max=1100) -> np.ndarray:
        f0 = self.infer_from_audio(audio, thred)
        f0[(f0 < f0_min) | (f0 > f0_max)] = 0
        return f0
