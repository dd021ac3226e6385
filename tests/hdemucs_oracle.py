"""torch-CPU restatement of demucs 4.0.1's ``demucs.hdemucs.HDemucs`` in eval mode (hybrid, cac, no multi_freqs, no Wiener filter) and
of ``demucs.apply.apply_model`` for a model that is not HTDemucs (a chunk is not padded to a training length) -- the twin the GPU network
is checked against.  PARITY UNPINNED as for HTDemucs; the BLSTM is ``torch.nn.LSTM``, an independent implementation of the recurrence.
Runs in the dtype of its input (float32 or float64).  The STFT / iSTFT helpers and the shift / segment plan come from
oracle/htdemucs_oracle.py."""
from __future__ import annotations

import math
from typing import Dict

import torch
import torch.nn.functional as F

from oracle.htdemucs_oracle import ispec as _ispec, segment_plan, shift_offsets, spec as _spec


def _plan(cfg):
    """HDemucs.__init__'s loop: per encoder index (freq, last_freq, ker, stride, pad, norm, lstm, attn)"""
    freqs = cfg.nfft // 2
    out = []
    for index in range(cfg.depth):
        freq = freqs > 1
        ker, stri = (cfg.kernel_size, cfg.stride) if freq else (2 * cfg.time_stride, cfg.time_stride)
        pad, last = ker // 4, False
        if freq and freqs <= cfg.kernel_size:
            ker, pad, last = freqs, 0, True
        out.append(dict(freq=freq, last=last, ker=ker, stri=stri, pad=pad, norm=index >= cfg.norm_starts, lstm=index >= cfg.dconv_lstm,
                        attn=index >= cfg.dconv_attn))
        if freq:
            freqs = 1 if freqs <= cfg.kernel_size else freqs // cfg.stride
    return out


def blstm(w: Dict[str, torch.Tensor], p: str, x: torch.Tensor, max_steps: int = 200) -> torch.Tensor:
    """demucs.demucs.BLSTM(dim, layers=2, max_steps=200, skip=True) on x [B, C, T], the recurrence by torch.nn.LSTM"""
    B, C, T = x.shape
    H = w[p + ".lstm.weight_hh_l0"].shape[1]
    lstm = torch.nn.LSTM(input_size=C, hidden_size=H, num_layers=2, bidirectional=True).to(x.dtype)
    lstm.load_state_dict({k[len(p) + 6:]: v.to(x.dtype) for k, v in w.items() if k.startswith(p + ".lstm.")})
    y = x
    framed = False
    if T > max_steps:
        width, stride = max_steps, max_steps // 2
        nf = math.ceil(T / stride)
        tgt = (nf - 1) * stride + width
        a = F.pad(x, (0, tgt - T))
        frames = a.as_strided([B, C, nf, width], [a.stride(0), a.stride(1), stride, 1])
        framed = True
        x = frames.permute(0, 2, 1, 3).reshape(-1, C, width)
    with torch.no_grad():
        z = lstm(x.permute(2, 0, 1))[0]
    z = F.linear(z, w[p + ".linear.weight"], w[p + ".linear.bias"]).permute(1, 2, 0)
    if framed:
        frames = z.reshape(B, -1, C, width)
        lim = stride // 2
        out = []
        for k in range(nf):
            if k == 0:
                out.append(frames[:, k, :, :-lim])
            elif k == nf - 1:
                out.append(frames[:, k, :, lim:])
            else:
                out.append(frames[:, k, :, lim:-lim])
        z = torch.cat(out, -1)[..., :T]
    return z + y


def local_state(w: Dict[str, torch.Tensor], p: str, x: torch.Tensor, heads: int = 4, ndecay: int = 4) -> torch.Tensor:
    """demucs.demucs.LocalState(channels, heads=4, nfreqs=0, ndecay=4) on x [B, C, T]"""
    B, C, T = x.shape
    idx = torch.arange(T, dtype=x.dtype)
    delta = idx[:, None] - idx[None, :]
    queries = F.conv1d(x, w[p + ".query.weight"], w[p + ".query.bias"]).view(B, heads, -1, T)
    keys = F.conv1d(x, w[p + ".key.weight"], w[p + ".key.bias"]).view(B, heads, -1, T)
    dots = torch.einsum("bhct,bhcs->bhts", keys, queries) / keys.shape[2] ** 0.5
    decays = torch.arange(1, ndecay + 1, dtype=x.dtype)
    decay_q = torch.sigmoid(F.conv1d(x, w[p + ".query_decay.weight"], w[p + ".query_decay.bias"]).view(B, heads, -1, T)) / 2
    decay_kernel = -decays.view(-1, 1, 1) * delta.abs() / ndecay ** 0.5
    dots = dots + torch.einsum("fts,bhfs->bhts", decay_kernel, decay_q)
    dots = dots.masked_fill(torch.eye(T, dtype=torch.bool), -100)
    weights = torch.softmax(dots, dim=2)
    content = F.conv1d(x, w[p + ".content.weight"], w[p + ".content.bias"]).view(B, heads, -1, T)
    result = torch.einsum("bhts,bhct->bhcs", weights, content).reshape(B, -1, T)
    return x + F.conv1d(result, w[p + ".proj.weight"], w[p + ".proj.bias"])


def _dconv(cfg, w, p: str, x: torch.Tensor, lstm: bool, attn: bool) -> torch.Tensor:
    """demucs.demucs.DConv(gelu, GroupNorm(1)) on [N, C, T] with the optional BLSTM (.3) and LocalState"""
    for d in range(cfg.dconv_depth):
        q = f"{p}.layers.{d}"
        dil = 2 ** d
        y = F.conv1d(x, w[q + ".0.weight"], w[q + ".0.bias"], dilation=dil, padding=dil)
        y = F.gelu(F.group_norm(y, 1, w[q + ".1.weight"], w[q + ".1.bias"], eps=1e-5))
        i = 3
        if lstm:
            y = blstm(w, f"{q}.{i}", y)
            i += 1
        if attn:
            y = local_state(w, f"{q}.{i}", y)
            i += 1
        y = F.conv1d(y, w[f"{q}.{i}.weight"], w[f"{q}.{i}.bias"])
        y = F.glu(F.group_norm(y, 1, w[f"{q}.{i + 1}.weight"], w[f"{q}.{i + 1}.bias"], eps=1e-5), dim=1)
        x = x + w[f"{q}.{i + 3}.scale"][:, None] * y
    return x


def _norm(cfg, w, p: str, x: torch.Tensor, on: bool) -> torch.Tensor:
    return F.group_norm(x, cfg.norm_groups, w[p + ".weight"], w[p + ".bias"], eps=1e-5) if on else x


def _enc(cfg, w, p: str, x: torch.Tensor, inject, L, freq: bool, empty: bool, ker: int, stri: int, pad: int) -> torch.Tensor:
    """demucs.hdemucs.HEncLayer.forward"""
    if not freq and x.dim() == 4:
        x = x.view(x.shape[0], -1, x.shape[-1])
    if freq:
        y = F.conv2d(x, w[p + ".conv.weight"], w[p + ".conv.bias"], stride=(stri, 1), padding=(pad, 0))
    else:
        le = x.shape[-1]
        if le % stri:
            x = F.pad(x, (0, stri - le % stri))
        y = F.conv1d(x, w[p + ".conv.weight"], w[p + ".conv.bias"], stride=stri, padding=pad)
    if empty:
        return y
    if inject is not None:
        y = y + (inject[:, :, None] if inject.dim() == 3 and y.dim() == 4 else inject)
    y = F.gelu(_norm(cfg, w, p + ".norm1", y, L["norm"]))
    if cfg.dconv_mode & 1:
        if freq:
            b, c, fr, t = y.shape
            y = _dconv(cfg, w, p + ".dconv", y.permute(0, 2, 1, 3).reshape(-1, c, t), L["lstm"], L["attn"]).view(b, fr, c, t).permute(0, 2, 1, 3)
        else:
            y = _dconv(cfg, w, p + ".dconv", y, L["lstm"], L["attn"])
    ce = cfg.context_enc
    z = F.conv2d(y, w[p + ".rewrite.weight"], w[p + ".rewrite.bias"], padding=ce) if freq else \
        F.conv1d(y, w[p + ".rewrite.weight"], w[p + ".rewrite.bias"], padding=ce)
    return F.glu(_norm(cfg, w, p + ".norm2", z, L["norm"]), dim=1)


def _dec(cfg, w, p: str, x: torch.Tensor, skip, length: int, L, freq: bool, empty: bool, last: bool, stri: int, pad: int):
    """demucs.hdemucs.HDecLayer.forward -> (z, pre)"""
    if freq and x.dim() == 3:
        B, C, T = x.shape
        x = x.view(B, w[p + ".conv_tr.weight"].shape[0], -1, T)
    if not empty:
        x = x + skip
        c = cfg.context
        r = F.conv2d(x, w[p + ".rewrite.weight"], w[p + ".rewrite.bias"], padding=c) if freq else \
            F.conv1d(x, w[p + ".rewrite.weight"], w[p + ".rewrite.bias"], padding=c)
        y = F.glu(_norm(cfg, w, p + ".norm1", r, L["norm"]), dim=1)
        if cfg.dconv_mode & 2:
            if freq:
                b, ch, fr, t = y.shape
                y = _dconv(cfg, w, p + ".dconv", y.permute(0, 2, 1, 3).reshape(-1, ch, t), L["lstm"], L["attn"]).view(b, fr, ch, t).permute(0, 2, 1, 3)
            else:
                y = _dconv(cfg, w, p + ".dconv", y, L["lstm"], L["attn"])
    else:
        y = x
    if freq:
        z = F.conv_transpose2d(y, w[p + ".conv_tr.weight"], w[p + ".conv_tr.bias"], stride=(stri, 1))
    else:
        z = F.conv_transpose1d(y, w[p + ".conv_tr.weight"], w[p + ".conv_tr.bias"], stride=stri)
    z = _norm(cfg, w, p + ".norm2", z, L["norm"])
    if freq:
        if pad:
            z = z[..., pad:-pad, :]
    else:
        z = z[..., pad:pad + length]
        assert z.shape[-1] == length, (z.shape, length)
    if not last:
        z = F.gelu(z)
    return z, y


@torch.no_grad()
def forward(cfg, w: Dict[str, torch.Tensor], mix: torch.Tensor) -> torch.Tensor:
    """HDemucs.forward in eval mode: mix [B, 2, L] (any L) -> [B, S, 2, L], in mix's dtype"""
    w = {k: v.to(mix.dtype) for k, v in w.items()}
    length = mix.shape[-1]
    z = _spec(cfg, mix)
    m = torch.view_as_real(z).permute(0, 1, 4, 2, 3)
    B, C, _, Fq, T = m.shape
    x = m.reshape(B, C * 2, Fq, T)
    mean = x.mean(dim=(1, 2, 3), keepdim=True)
    std = x.std(dim=(1, 2, 3), keepdim=True)
    x = (x - mean) / (1e-5 + std)
    xt = mix
    meant = xt.mean(dim=(1, 2), keepdim=True)
    stdt = xt.std(dim=(1, 2), keepdim=True)
    xt = (xt - meant) / (1e-5 + stdt)
    plan = _plan(cfg)
    n_freq = sum(L["freq"] for L in plan)
    saved, saved_t, lengths, lengths_t = [], [], [], []
    for idx, L in enumerate(plan):
        lengths.append(x.shape[-1])
        inject = None
        if L["freq"]:
            lengths_t.append(xt.shape[-1])
            xt = _enc(cfg, w, f"tencoder.{idx}", xt, None, L, False, L["last"], cfg.kernel_size, cfg.stride, cfg.kernel_size // 4)
            if not L["last"]:
                saved_t.append(xt)
            else:
                inject = xt
        x = _enc(cfg, w, f"encoder.{idx}", x, inject, L, L["freq"], False, L["ker"], L["stri"], L["pad"])
        if idx == 0:
            emb = (w["freq_emb.embedding.weight"] * cfg.emb_scale).t()[None, :, :, None].expand_as(x)
            x = x + cfg.freq_emb * emb
        saved.append(x)
    x = torch.zeros_like(x)
    for di in range(cfg.depth):
        idx = cfg.depth - 1 - di
        L = plan[idx]
        x, pre = _dec(cfg, w, f"decoder.{di}", x, saved.pop(-1), lengths.pop(-1), L, L["freq"], False, idx == 0, L["stri"], L["pad"])
        if L["freq"]:
            ti = n_freq - 1 - idx
            length_t = lengths_t.pop(-1)
            if L["last"]:
                xt, _ = _dec(cfg, w, f"tdecoder.{ti}", pre[:, :, 0], None, length_t, L, False, True, idx == 0, cfg.stride, cfg.kernel_size // 4)
            else:
                xt, _ = _dec(cfg, w, f"tdecoder.{ti}", xt, saved_t.pop(-1), length_t, L, False, False, idx == 0, cfg.stride,
                             cfg.kernel_size // 4)
    S = cfg.S
    x = x.view(B, S, -1, Fq, T) * std[:, None] + mean[:, None]
    zout = torch.view_as_complex(x.view(B, S, -1, 2, Fq, T).permute(0, 1, 2, 4, 5, 3).contiguous())
    x = _ispec(cfg, zout, length)
    xt = xt.view(B, S, -1, length) * stdt[:, None] + meant[:, None]
    return xt + x


def _run_split(cfg, root: torch.Tensor, base: int, length: int, overlap: float, fwd) -> torch.Tensor:
    """split=True over root[..., base : base + length] for a model without valid_length: every chunk is TensorChunk(view, offset, segment)
    as it is -- the last one shorter, the others with the real samples of the view -- and the output weighed by the triangle"""
    B, C, _ = root.shape
    seg = cfg.segment_samples
    offsets, weight = segment_plan(length, seg, overlap)
    out = torch.zeros(B, cfg.S, C, length, dtype=root.dtype)
    sum_weight = torch.zeros(length, dtype=root.dtype)
    for off in offsets:
        cl = min(length - off, seg)
        y = fwd(root[..., base + off: base + off + cl])
        out[..., off:off + cl] += weight[:cl].to(root.dtype) * y
        sum_weight[off:off + cl] += weight[:cl].to(root.dtype)
    return out / sum_weight


@torch.no_grad()
def apply_model(cfg, w: Dict[str, torch.Tensor], mix: torch.Tensor, shifts: int = 2, overlap: float = 0.25, seed: int = 0,
                fwd=None) -> torch.Tensor:
    """demucs.apply.apply_model(model, mix, shifts, split=True, overlap) for an HDemucs: mix [B, 2, L] -> [B, S, 2, L]"""
    fwd = fwd or (lambda x: forward(cfg, w, x))
    length = mix.shape[-1]
    if not shifts:
        return _run_split(cfg, mix, 0, length, overlap, fwd)
    max_shift = int(0.5 * cfg.samplerate)
    padded = F.pad(mix, (max_shift, max_shift))
    out = 0.0
    for offset in shift_offsets(shifts, max_shift, seed):
        res = _run_split(cfg, padded, offset, length + max_shift - offset, overlap, fwd)
        out = out + res[..., max_shift - offset:]
    return out / shifts


def separate(cfg, w: Dict[str, torch.Tensor], mix: torch.Tensor, shifts: int = 2, overlap: float = 0.25, seed: int = 0,
             fwd=None) -> torch.Tensor:
    """DemucsSeparator's whole-track normalisation around apply_model: mix [2, L] -> [S, 2, L]"""
    ref = mix.mean(0)
    m, s = ref.mean(), ref.std()
    out = apply_model(cfg, w, ((mix - m) / s)[None], shifts=shifts, overlap=overlap, seed=seed, fwd=fwd)[0]
    return out * s + m


def lstm_reference(pre_w: Dict[str, torch.Tensor], x: torch.Tensor, H: int, num_layers: int = 1) -> torch.Tensor:
    """torch.nn.LSTM (bidirectional) with the given parameters on x [T, N, C] -> [T, N, 2H], in x's dtype"""
    lstm = torch.nn.LSTM(input_size=x.shape[-1], hidden_size=H, num_layers=num_layers, bidirectional=True).to(x.dtype)
    lstm.load_state_dict({k: v.to(x.dtype) for k, v in pre_w.items()})
    with torch.no_grad():
        return lstm(x)[0]

