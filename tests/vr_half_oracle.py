"""The VR networks' half-precision mode (``VRNet`` / ``VRNetNew(precision="f16")``) restated in float64 on the CPU (torch), from a
state_dict and the layer list of audiolab_amd/vrnet.py.  Values are rounded to IEEE half at exactly the points the half mode rounds:
the convolution and depthwise weights; the input; each conv + BatchNorm + activation result (except the two float32 ones: the logits
and the LSTM module's 1x1 convolution); depthwise, resize and mean results; the LSTM module's output.  Everything else is float64.

The layer functions take and return channels-last double tensors [B, H, W, C], so a test can recompute ONE layer from the inputs the
device network itself had.  Each ``*_bound`` is the derived distance a correct kernel may have from the float64 value: half a spacing of
IEEE half at the result (for a half output) plus the float32 arithmetic of the kernel.  It does not import the reference."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

EPS32 = 2.0 ** -24                                      # unit roundoff of float32


def r16(t: torch.Tensor) -> torch.Tensor:
    """round to IEEE half (one rounding, straight from double), back as double"""
    return torch.from_numpy(t.detach().cpu().double().numpy().astype(np.float16).astype(np.float64))


def half_ulp(v) -> np.ndarray:
    """the spacing of IEEE half at |v| (subnormal spacing below 2^-14): tests/test_htdemucs_half.py's helper"""
    e = np.floor(np.log2(np.maximum(np.abs(np.asarray(v, dtype=np.float64)), 2.0 ** -14)))
    return 2.0 ** (e - 10)


def out_bound(ref, arith, y_f16: bool = True) -> np.ndarray:
    """|device - ref| allowed: the kernel computes v' with |v' - ref| <= arith in float32 and rounds it to half, an error of at most half
    the spacing at v' -- which lies within arith of ref, possibly in the next binade."""
    ref, arith = np.abs(np.asarray(ref, dtype=np.float64)), np.asarray(arith, dtype=np.float64)
    return (0.5 * half_ulp(ref + arith) if y_f16 else 0.0) + arith


def rel(a, b) -> float:
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).norm() / b.norm())


# ---- layers ----------------------------------------------------------------------------------------------------------------------------
class Conv:
    """Conv2d(bias=False) [+ BatchNorm2d eval]: half weights, the float32 scale / shift the device computes (same torch expression)"""

    def __init__(self, sd, conv_key, bn_prefix, act, stride=1, pad=0, dil=1, eps=1e-5):
        w = sd[conv_key].float()
        self.name = conv_key[:-len(".weight")]
        self.w = r16(w)                                  # [Cout, Cin, KH, KW]
        if bn_prefix is not None:
            gamma, beta = sd[bn_prefix + ".weight"].float(), sd[bn_prefix + ".bias"].float()
            mean, var = sd[bn_prefix + ".running_mean"].float(), sd[bn_prefix + ".running_var"].float()
            scale = gamma / torch.sqrt(var + eps)
            shift = beta - mean * scale
        else:
            scale, shift = torch.ones(w.shape[0]), torch.zeros(w.shape[0])
        self.scale, self.shift = scale.double(), shift.double()
        pair = lambda v: tuple(v) if isinstance(v, (tuple, list)) else (v, v)
        self.act, self.stride, self.pad, self.dil = act, stride, pair(pad), pair(dil)

    def raw(self, x, w=None):
        w = self.w if w is None else w
        return F.conv2d(x.permute(0, 3, 1, 2), w, None, stride=self.stride, padding=self.pad, dilation=self.dil).permute(0, 2, 3, 1)

    def value(self, x):
        """float64 value of act(conv(x) * scale + shift) on the half operands x, w"""
        v = self.raw(x.double()) * self.scale + self.shift
        if self.act == "relu":
            v = torch.relu(v)
        elif self.act == "leaky":
            v = torch.where(v > 0, v, 0.01 * v)
        return v

    def __call__(self, x, out_f32=False):
        v = self.value(x)
        return v if out_f32 else r16(v)

    def arith(self, x):
        """float32 arithmetic of the kernel: K products accumulated in float32 (K 2^-24 sum |a b|, scaled by |scale|), then one fused
        multiply-add and the activation's multiply (a few 2^-24 of |scale| sum |a b| + |shift|)"""
        k = self.w.shape[1] * self.w.shape[2] * self.w.shape[3]
        mag = self.raw(x.double().abs(), self.w.abs()) * self.scale.abs()
        return ((k * EPS32) * mag + 4 * EPS32 * (mag + self.shift.abs())).numpy()


def _src(n_out, n_in):
    """align_corners source index / weight along one axis, in float32 as the kernels compute them"""
    s = np.float32(n_in - 1) / np.float32(n_out - 1) if n_out > 1 else np.float32(0)
    o = np.arange(n_out, dtype=np.float32)
    i0 = np.minimum((s * o).astype(np.float32).astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    # the weight is one fused multiply-add, s o - i0: the product of two float32 is exact in double
    return i0, i1, (np.float64(s) * o.astype(np.float64) - i0).astype(np.float32)


def _f32(a):
    return a.astype(np.float32).astype(np.float64)


def resize_device(x, ho, wo):
    """Bilinear resize (align_corners) with the kernels' float32 operation order -- hy (hx v00 + lx v01) + ly (hx v10 + lx v11), each
    inner sum and the outer one a fused multiply-add -- evaluated in float64 and rounded to float32 after every operation: products of a
    24-bit weight and an 11-bit half value are exact in double, so this gives the kernel's float32 value, then its rounding to half.
    Used where the result is an OPERAND (the decoder's interpolated channels), so that the comparison sees the convolution alone."""
    a = x.double().numpy()
    y0, y1, ly = _src(ho, a.shape[1])
    x0, x1, lx = _src(wo, a.shape[2])
    ly, lx = ly.astype(np.float64)[None, :, None, None], lx.astype(np.float64)[None, None, :, None]
    hy, hx = _f32(1.0 - ly), _f32(1.0 - lx)
    v00, v01 = a[:, y0][:, :, x0], a[:, y0][:, :, x1]
    v10, v11 = a[:, y1][:, :, x0], a[:, y1][:, :, x1]
    t0 = _f32(lx * v01 + _f32(hx * v00))
    t1 = _f32(lx * v11 + _f32(hx * v10))
    v = _f32(ly * t1 + _f32(hy * t0))
    return torch.from_numpy(v.astype(np.float16).astype(np.float64))


def resize_value(x, ho, wo):
    """the float64 value of the interpolation with the float32 weights (not rounded), and its float32 arithmetic term"""
    a = x.double().numpy()
    y0, y1, ly = _src(ho, a.shape[1])
    x0, x1, lx = _src(wo, a.shape[2])
    ly, lx = ly.astype(np.float64)[None, :, None, None], lx.astype(np.float64)[None, None, :, None]
    v00, v01 = a[:, y0][:, :, x0], a[:, y0][:, :, x1]
    v10, v11 = a[:, y1][:, :, x0], a[:, y1][:, :, x1]
    v = (1 - ly) * ((1 - lx) * v00 + lx * v01) + ly * ((1 - lx) * v10 + lx * v11)
    mag = (1 - ly) * ((1 - lx) * np.abs(v00) + lx * np.abs(v01)) + ly * ((1 - lx) * np.abs(v10) + lx * np.abs(v11))
    return torch.from_numpy(v), 8 * EPS32 * mag           # 1 - l, three multiplies, three fused multiply-adds: below 8 roundings


def crop(skip, wo):
    off = (skip.shape[2] - wo) // 2
    return skip[:, :, off:off + wo]


def decoder_input(x, skip):
    """what the decoder's convolution reads: cat(upsample x2 of x as the device rounds it, skip centre-cropped along frames)"""
    ho, wo = 2 * x.shape[1], 2 * x.shape[2]
    return torch.cat([resize_device(x, ho, wo), crop(skip.double(), wo)], dim=3)


def depthwise_value(x, w, d):
    """x [B,H,W,C], w [C,3,3] (half values), dilation = padding = d -> (float64 value, float32 arithmetic term: nine fused multiply-adds)"""
    c = x.shape[3]
    xx, ww = x.double().permute(0, 3, 1, 2), w.double().reshape(c, 1, 3, 3)
    v = F.conv2d(xx, ww, None, padding=d, dilation=d, groups=c).permute(0, 2, 3, 1)
    mag = F.conv2d(xx.abs(), ww.abs(), None, padding=d, dilation=d, groups=c).permute(0, 2, 3, 1)
    return v, (9 * EPS32 * mag).numpy()


def mean_value(x):
    """mean over bins -> [B,1,W,C]; float32: H additions and a division"""
    h = x.shape[1]
    v = x.double().mean(dim=1, keepdim=True)
    mag = x.double().abs().mean(dim=1, keepdim=True)
    return v, ((h + 1) * EPS32 * mag).numpy()


def lstm_value(sd, p, conv_out):
    """LSTMModule after its 1x1 convolution (layers_new.py:117-125): conv_out [N, bins, frames, 1] -> [N, bins, frames, 1], float64"""
    n, nbins, nframes, _ = conv_out.shape
    hd = sd[f"{p}.lstm_dec2.lstm.weight_hh_l0"].shape[1]
    lstm = torch.nn.LSTM(nbins, hd, bidirectional=True).double()
    with torch.no_grad():
        for k in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0"):
            for sfx in ("", "_reverse"):
                getattr(lstm, k + sfx).copy_(sd[f"{p}.lstm_dec2.lstm.{k}{sfx}"].double())
        seq = conv_out.double()[..., 0].permute(2, 0, 1)                   # [frames, N, bins]
        h, _ = lstm(seq)
        wd, bd = sd[f"{p}.lstm_dec2.dense.0.weight"].double(), sd[f"{p}.lstm_dec2.dense.0.bias"].double()
        gamma, beta = sd[f"{p}.lstm_dec2.dense.1.weight"].double(), sd[f"{p}.lstm_dec2.dense.1.bias"].double()
        mean, var = sd[f"{p}.lstm_dec2.dense.1.running_mean"].double(), sd[f"{p}.lstm_dec2.dense.1.running_var"].double()
        o = F.linear(h.reshape(nframes * n, 2 * hd), wd, bd)
        o = torch.relu((o - mean) / torch.sqrt(var + 1e-5) * gamma + beta)
    return o.reshape(nframes, n, nbins).permute(1, 2, 0).unsqueeze(-1)


# the float32 LSTM module against float64: products of up to 512 terms (K 2^-24 relative to sum |a b|, here O(1) values) through
# sigmoid / tanh recurrences whose derivatives are <= 1 -- 1e-4 absolute is what the float32 kernels of this module are pinned to
# against torch (tests/test_emul_vrnet.py), two orders above what they do and a tenth of half's spacing at 1
LSTM_ARITH = 1e-4


def mask_value(logit, mix, aggr):
    """alsep_vr_mask: sigmoid, replicate-pad along bins, aggressiveness powers, * mix"""
    m = torch.sigmoid(logit.double())
    hm, hout = m.shape[1], mix.shape[1]
    if hout > hm:
        m = torch.cat([m, m[:, -1:].expand(-1, hout - hm, -1, -1)], dim=1)
    if aggr:
        split, v = int(aggr["split_bin"]), float(np.float32(aggr["value"]))
        m = torch.cat([m[:, :split] ** (1 + v / 3), m[:, split:] ** (1 + v)], dim=1)
    return m * mix.double()


# ---- CascadedASPPNet (VRNet) -------------------------------------------------------------------------------------------------------------
def _aspp_pool(convs, p, x):
    pooled = r16(mean_value(x)[0])
    t = convs[f"{p}.aspp.conv1.1.conv.0"](pooled)
    return r16(resize_value(t, x.shape[1], x.shape[2])[0])


def build_vrnet(sd, widths):
    """every Conv of a CascadedASPPNet by its name, and the depthwise weights"""
    w1, b2, w2, b3, w3 = widths
    convs, dws = {}, {}

    def mk(key, bn, act, stride=1, pad=0, dil=1):
        c = Conv(sd, key, bn, act, stride, pad, dil)
        convs[c.name] = c
    for p in ("stg1_low_band_net", "stg1_high_band_net", "stg2_full_band_net", "stg3_full_band_net"):
        for i in (1, 2, 3, 4):
            mk(f"{p}.enc{i}.conv1.conv.0.weight", f"{p}.enc{i}.conv1.conv.1", "leaky", 1, 1)
            mk(f"{p}.enc{i}.conv2.conv.0.weight", f"{p}.enc{i}.conv2.conv.1", "leaky", 2, 1)
        mk(f"{p}.aspp.conv1.1.conv.0.weight", f"{p}.aspp.conv1.1.conv.1", "relu")
        mk(f"{p}.aspp.conv2.conv.0.weight", f"{p}.aspp.conv2.conv.1", "relu")
        for j, d in zip((3, 4, 5), (4, 8, 16)):
            dw = sd[f"{p}.aspp.conv{j}.conv.0.weight"].float()
            dws[f"{p}.aspp.conv{j}.conv.0"] = (r16(dw.reshape(dw.shape[0], 3, 3)), d)
            mk(f"{p}.aspp.conv{j}.conv.1.weight", f"{p}.aspp.conv{j}.conv.2", "relu")
        mk(f"{p}.aspp.bottleneck.0.conv.0.weight", f"{p}.aspp.bottleneck.0.conv.1", "relu")
        for i in (4, 3, 2, 1):
            mk(f"{p}.dec{i}.conv.conv.0.weight", f"{p}.dec{i}.conv.conv.1", "relu", 1, 1)
    mk("stg2_bridge.conv.0.weight", "stg2_bridge.conv.1", "relu")
    mk("stg3_bridge.conv.0.weight", "stg3_bridge.conv.1", "relu")
    mk("out.weight", None, "none")
    return convs, dws


def vrnet_forward(sd, widths, n_fft, x_nchw, aggr=None):
    """``VRNet(precision="f16").forward``: [B, 2, bins, frames] -> [B, 2, n_fft / 2 + 1, frames] (double)"""
    convs, dws = build_vrnet(sd, widths)
    max_bin, output_bin = n_fft // 2, n_fft // 2 + 1
    x = torch.as_tensor(x_nchw).float().permute(0, 2, 3, 1)
    mix = x[:, :output_bin].double()
    xin = r16(x[:, :max_bin])

    def base(p, h):
        skips = []
        for i in (1, 2, 3, 4):
            s = convs[f"{p}.enc{i}.conv1.conv.0"](h)
            h = convs[f"{p}.enc{i}.conv2.conv.0"](s)
            skips.append(s)
        parts = [_aspp_pool(convs, p, h), convs[f"{p}.aspp.conv2.conv.0"](h)]
        for j in (3, 4, 5):
            dw, d = dws[f"{p}.aspp.conv{j}.conv.0"]
            parts.append(convs[f"{p}.aspp.conv{j}.conv.1"](r16(depthwise_value(h, dw, d)[0])))
        h = convs[f"{p}.aspp.bottleneck.0.conv.0"](torch.cat(parts, dim=3))
        for i in (4, 3, 2, 1):
            h = convs[f"{p}.dec{i}.conv.conv.0"](decoder_input(h, skips[i - 1]))
        return h
    bandw = xin.shape[1] // 2
    aux1 = torch.cat([base("stg1_low_band_net", xin[:, :bandw]), base("stg1_high_band_net", xin[:, bandw:])], dim=1)
    h1 = torch.cat([xin, aux1], dim=3)
    aux2 = base("stg2_full_band_net", convs["stg2_bridge.conv.0"](h1))
    h2 = torch.cat([h1, aux2], dim=3)
    h3 = base("stg3_full_band_net", convs["stg3_bridge.conv.0"](h2))
    logit = convs["out"](h3, out_f32=True)
    return mask_value(logit, mix, aggr).permute(0, 3, 1, 2)


# ---- CascadedNet (VRNetNew) ----------------------------------------------------------------------------------------------------------------
NEW_BASES = ("stg1_low_band_net.0", "stg1_high_band_net", "stg2_low_band_net.0", "stg2_high_band_net", "stg3_full_band_net")


def build_vrnet_new(sd):
    convs = {}

    def mk(key, bn, act, stride=1, pad=0, dil=1):
        c = Conv(sd, key, bn, act, stride, pad, dil)
        convs[c.name] = c
    for p in NEW_BASES:
        mk(f"{p}.enc1.conv.0.weight", f"{p}.enc1.conv.1", "relu", 1, 1)
        for i in (2, 3, 4, 5):
            mk(f"{p}.enc{i}.conv1.conv.0.weight", f"{p}.enc{i}.conv1.conv.1", "leaky", 2, 1)
            mk(f"{p}.enc{i}.conv2.conv.0.weight", f"{p}.enc{i}.conv2.conv.1", "leaky", 1, 1)
        mk(f"{p}.aspp.conv1.1.conv.0.weight", f"{p}.aspp.conv1.1.conv.1", "relu")
        mk(f"{p}.aspp.conv2.conv.0.weight", f"{p}.aspp.conv2.conv.1", "relu")
        for j, d in zip((3, 4, 5), ((4, 2), (8, 4), (12, 6))):
            mk(f"{p}.aspp.conv{j}.conv.0.weight", f"{p}.aspp.conv{j}.conv.1", "relu", 1, d, d)
        mk(f"{p}.aspp.bottleneck.conv.0.weight", f"{p}.aspp.bottleneck.conv.1", "relu")
        for i in (4, 3, 2, 1):
            mk(f"{p}.dec{i}.conv1.conv.0.weight", f"{p}.dec{i}.conv1.conv.1", "relu", 1, 1)
        mk(f"{p}.lstm_dec2.conv.conv.0.weight", f"{p}.lstm_dec2.conv.conv.1", "relu")
    mk("stg1_low_band_net.1.conv.0.weight", "stg1_low_band_net.1.conv.1", "relu")
    mk("stg2_low_band_net.1.conv.0.weight", "stg2_low_band_net.1.conv.1", "relu")
    mk("out.weight", None, "none")
    return convs


def vrnet_new_forward(sd, n_fft, x_nchw):
    """``VRNetNew(precision="f16").forward``"""
    convs = build_vrnet_new(sd)
    max_bin, output_bin = n_fft // 2, n_fft // 2 + 1
    x = torch.as_tensor(x_nchw).float().permute(0, 2, 3, 1)
    mix = x[:, :output_bin].double()
    xin = r16(x[:, :max_bin])

    def base(p, h):
        es = [convs[f"{p}.enc1.conv.0"](h)]
        h = es[0]
        for i in (2, 3, 4, 5):
            h = convs[f"{p}.enc{i}.conv2.conv.0"](convs[f"{p}.enc{i}.conv1.conv.0"](h))
            es.append(h)
        e1, e2, e3, e4, e5 = es
        parts = [_aspp_pool(convs, p, e5), convs[f"{p}.aspp.conv2.conv.0"](e5)]
        parts += [convs[f"{p}.aspp.conv{j}.conv.0"](e5) for j in (3, 4, 5)]
        h = convs[f"{p}.aspp.bottleneck.conv.0"](torch.cat(parts, dim=3))
        for i, e in ((4, e4), (3, e3), (2, e2)):
            h = convs[f"{p}.dec{i}.conv1.conv.0"](decoder_input(h, e))
        lo = r16(lstm_value(sd, p, convs[f"{p}.lstm_dec2.conv.conv.0"](h, out_f32=True)))
        return convs[f"{p}.dec1.conv1.conv.0"](decoder_input(torch.cat([h, lo], dim=3), e1))
    bandw = xin.shape[1] // 2
    l1_in, h1_in = xin[:, :bandw], xin[:, bandw:]
    l1 = convs["stg1_low_band_net.1.conv.0"](base("stg1_low_band_net.0", l1_in))
    h1 = base("stg1_high_band_net", h1_in)
    aux1 = torch.cat([l1, h1], dim=1)
    l2 = convs["stg2_low_band_net.1.conv.0"](base("stg2_low_band_net.0", torch.cat([l1_in, l1], dim=3)))
    h2 = base("stg2_high_band_net", torch.cat([h1_in, h1], dim=3))
    aux2 = torch.cat([l2, h2], dim=1)
    f3 = base("stg3_full_band_net", torch.cat([xin, aux1, aux2], dim=3))
    logit = convs["out"](f3, out_f32=True)
    return mask_value(logit, mix, None).permute(0, 3, 1, 2)


# ---- the runner ----------------------------------------------------------------------------------------------------------------------------
def inference(forward, x_spec, window_size, offset, tta=False):
    """``vrnet.vr_inference`` (utils.py:25-100) around ``forward([1, 2, bins, window]) -> [1, 2, bins, window]``: pred * coef in double"""
    x_mag = torch.as_tensor(x_spec).abs().float()
    coef = x_mag.max()
    pre = x_mag / coef
    n_frame = pre.shape[2]

    def padding(width):
        roi = window_size - 2 * offset
        roi = roi if roi != 0 else window_size
        return offset, roi - (width % roi) + offset, roi

    def execute(pad_l, pad_r, roi, n_window):
        padded = F.pad(pre, (pad_l, pad_r))
        preds = []
        for i in range(n_window):
            out = forward(padded[None, :, :, i * roi:i * roi + window_size])[0]
            preds.append(out[:, :, offset:window_size - offset] if offset > 0 else out)
        return torch.cat(preds, dim=2)
    pad_l, pad_r, roi = padding(n_frame)
    n_window = -(-n_frame // roi)
    pred = execute(pad_l, pad_r, roi, n_window)[:, :, :n_frame]
    if tta:
        pred_t = execute(pad_l + roi // 2, pad_r + roi // 2, roi, n_window + 1)[:, :, roi // 2:][:, :, :n_frame]
        pred = (pred + pred_t) * 0.5
    return pred * coef.double()
