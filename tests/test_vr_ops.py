"""Direct tests of the small fp32 kernels of the VR networks (csrc/vrnet.hip: depthwise convolution, bilinear resize, crop-and-concatenate,
mean over bins, mask, LSTM recurrence for every hidden size it is built for) and of the VR multi-band front / back end (csrc/nn.hip: band
crop, phase split, mirroring, band spectrogram).  References: the torch function or the few lines of spec_utils.py / vr.py that the kernel's
comment names, in float64 on the CPU.  Shapes have pairwise different extents and non-zero offsets; destinations are pre-filled with a
sentinel that must survive wherever the kernel has no business.  Data movement is bit-exact, element-wise kernels are held to
1e-6 * max(1, max|want|), kernels with a reduction to 2e-5 * max(1, max|want|)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from audiolab_amd import _lib
from audiolab_amd._lib import AlsepError
from tests.conftest import host, on

SENT = 7.25
EW, RED = 1e-6, 2e-5


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _out(dev, n, tail=5):
    return on(dev, torch.full((n + tail,), SENT))


def _close(got, want, tol, what):
    want = want.detach().numpy() if isinstance(want, torch.Tensor) else np.asarray(want)
    got = np.asarray(got, dtype=np.float64).reshape(want.shape)
    err, bound = float(np.max(np.abs(got - want))), tol * max(1.0, float(np.max(np.abs(want))))
    assert np.all(np.isfinite(got)) and err < bound, f"{what}: max|delta| {err:.3e} >= {bound:.3e}"


def _cplx(t):
    """float tensor [..., 2] -> complex128 numpy"""
    a = t.double().numpy()
    return a[..., 0] + 1j * a[..., 1]


def _pairs(z):
    return np.stack([z.real, z.imag], -1)


# ------------------------------------------------------------------------------------------ network kernels (vrnet.hip)
@pytest.mark.parametrize("KH,dil,pad", [(3, 1, 1), (3, 4, 4), (3, 8, 8)])
def test_depthwise_vs_torch(dev, KH, dil, pad):
    """nn.Conv2d(groups = C, dilation, same-size padding); H = 10, W = 13: with dilation 8 every output loses taps beyond some edge"""
    B, H, W, Cn = 2, 10, 13, 5
    g = _gen(dil)
    x = torch.randn(B, H, W, Cn, generator=g) + 0.3
    w = torch.randn(Cn, KH, KH, generator=g) * 0.5 + 0.1
    want = F.conv2d(x.double().permute(0, 3, 1, 2), w.double()[:, None], padding=pad, dilation=dil, groups=Cn).permute(0, 2, 3, 1)
    xd, wd, y = on(dev, x.clone()), on(dev, w.clone()), _out(dev, x.numel())
    dev.check(dev.lib.alsep_vr_depthwise(dev.handle, _lib.ptr(xd), _lib.ptr(wd), _lib.ptr(y), B, H, W, Cn, KH, KH, pad, dil), "alsep_vr_depthwise")
    got = host(y)
    assert np.all(got[x.numel():] == SENT)
    _close(got[:x.numel()], want, RED, "alsep_vr_depthwise")


@pytest.mark.parametrize("H,W,Ho,Wo", [(5, 7, 10, 14), (6, 9, 11, 4), (4, 6, 1, 11)])
def test_resize_bilinear_vs_torch(dev, H, W, Ho, Wo):
    """F.interpolate(mode="bilinear", align_corners=True) into a channel slice.  Against torch's own float32 result the kernel performs the
    same operations (a contracted multiply-add at the most: 1e-6); against float64 the source coordinate dst * ((in - 1) / (out - 1)) carries
    two float32 roundings, 2^-23 * max(H, W) pixels at the most, and a pixel's step changes the result by at most 2 max|x|."""
    B, Cn, ct, c0 = 2, 3, 8, 4
    x = torch.randn(B, H, W, Cn, generator=_gen(H * 10 + Wo)) * 0.5 + 0.3
    xn = x.permute(0, 3, 1, 2)
    want32 = F.interpolate(xn, size=(Ho, Wo), mode="bilinear", align_corners=True).permute(0, 2, 3, 1).numpy()
    want64 = F.interpolate(xn.double(), size=(Ho, Wo), mode="bilinear", align_corners=True).permute(0, 2, 3, 1).numpy()
    xd, y = on(dev, x.clone()), _out(dev, B * Ho * Wo * ct)
    dev.check(dev.lib.alsep_vr_resize_bilinear(dev.handle, _lib.ptr(xd), _lib.ptr(y), B, H, W, Cn, Ho, Wo, ct, c0), "alsep_vr_resize_bilinear")
    got = host(y)
    assert np.all(got[B * Ho * Wo * ct:] == SENT)
    got = got[:B * Ho * Wo * ct].reshape(B, Ho, Wo, ct)
    assert np.all(got[..., :c0] == SENT) and np.all(got[..., c0 + Cn:] == SENT)
    got = got[..., c0:c0 + Cn]
    e32, e64 = float(np.max(np.abs(got - want32))), float(np.max(np.abs(got.astype(np.float64) - want64)))
    bound64 = max(H, W) * 2.0 ** -22 * float(x.abs().max()) + 1e-6
    assert e32 <= 1e-6 and e64 < bound64, f"vs float32 {e32:.3e}, vs float64 {e64:.3e} (bound {bound64:.3e})"


def test_copy_slice(dev):
    """spec_utils.crop_center + torch.cat: y[bh, wq, c0 + c] = x[bh, w_off + wq, c]"""
    BH, Wx, Cn, w_off, Wy, ct, c0 = 6, 11, 3, 2, 7, 8, 4
    x = torch.randn(BH, Wx, Cn, generator=_gen(3)) + 0.3
    want = np.full((BH, Wy, ct), SENT, np.float32)
    want[:, :, c0:c0 + Cn] = x[:, w_off:w_off + Wy].numpy()
    xd, y = on(dev, x.clone()), _out(dev, want.size)
    dev.check(dev.lib.alsep_vr_copy_slice(dev.handle, _lib.ptr(xd), _lib.ptr(y), BH, Wx, Cn, w_off, Wy, ct, c0), "alsep_vr_copy_slice")
    got = host(y)
    assert np.all(got[want.size:] == SENT) and np.array_equal(got[:want.size].reshape(want.shape), want)


def test_mean_over_bins(dev):
    B, H, W, Cn = 2, 10, 7, 3
    x = torch.randn(B, H, W, Cn, generator=_gen(4)) + 0.6
    want = x.double().mean(1)                                                                # nn.AdaptiveAvgPool2d((1, None)) on [B, C, H, W]
    xd, y = on(dev, x.clone()), _out(dev, want.numel())
    dev.check(dev.lib.alsep_vr_mean_h(dev.handle, _lib.ptr(xd), _lib.ptr(y), B, H, W, Cn), "alsep_vr_mean_h")
    got = host(y)
    assert np.all(got[want.numel():] == SENT)
    _close(got[:want.numel()], want, RED, "alsep_vr_mean_h")


@pytest.mark.parametrize("aggr", [-1.0, 0.2])
def test_mask(dev, aggr):
    """sigmoid(logit) replicate-padded from Hm to Hout bins, raised to 1 + a / 3 below split_bin and to 1 + a from it on (a >= 0), times mix"""
    B, Hm, Hout, W, Cn, split = 2, 9, 12, 5, 3, 4
    g = _gen(5)
    logit, mix = torch.randn(B, Hm, W, Cn, generator=g) * 2 + 0.4, torch.randn(B, Hout, W, Cn, generator=g) + 0.3
    m = F.pad(torch.sigmoid(logit.double()).permute(0, 3, 2, 1), (0, Hout - Hm, 0, 0), mode="replicate").permute(0, 3, 2, 1)      # pad the bins
    if aggr >= 0:
        a = float(np.float32(aggr))
        m = torch.cat([m[:, :split] ** (1 + a / 3), m[:, split:] ** (1 + a)], 1)
    want = m * mix.double()
    ld, md, y = on(dev, logit.clone()), on(dev, mix.clone()), _out(dev, want.numel())
    dev.check(dev.lib.alsep_vr_mask(dev.handle, _lib.ptr(ld), _lib.ptr(md), _lib.ptr(y), B, Hm, Hout, W, Cn, split, aggr), "alsep_vr_mask")
    got = host(y)
    assert np.all(got[want.numel():] == SENT)
    _close(got[:want.numel()], want, EW, "alsep_vr_mask")


_LSTM_REF = {}


def _lstm_ref(hidden):
    """(x W_ih^T + b_ih + b_hh, W_hh, output) of both directions of a float64 nn.LSTM; computed once per hidden size"""
    if hidden not in _LSTM_REF:
        T, N, n_in = 9, 3, 5
        torch.manual_seed(hidden)
        net = torch.nn.LSTM(n_in, hidden, bidirectional=True).double()
        x = torch.randn(T, N, n_in, dtype=torch.float64) + 0.3
        with torch.no_grad():
            out = net(x)[0]                                                                  # [T, N, 2 hidden]
            dirs = []
            for d, sfx in enumerate(("", "_reverse")):
                w_ih, w_hh = getattr(net, "weight_ih_l0" + sfx), getattr(net, "weight_hh_l0" + sfx)
                pre = x @ w_ih.t() + getattr(net, "bias_ih_l0" + sfx) + getattr(net, "bias_hh_l0" + sfx)
                dirs.append((pre.float(), w_hh.float().clone(), out[..., d * hidden:(d + 1) * hidden].clone()))
        _LSTM_REF[hidden] = dirs
    return _LSTM_REF[hidden]


@pytest.mark.parametrize("hidden", [16, 32, 64])
@pytest.mark.parametrize("reverse", [0, 1])
def test_lstm_direction_vs_torch(dev, hidden, reverse):
    T, N = 9, 3
    pre, whh, want = _lstm_ref(hidden)[reverse]
    stride, off = 2 * hidden + 3, hidden
    pd, wd, y = on(dev, pre.clone()), on(dev, whh.clone()), _out(dev, T * N * stride)
    dev.check(dev.lib.alsep_vr_lstm(dev.handle, _lib.ptr(pd), _lib.ptr(wd), _lib.ptr(y), T, N, hidden, stride, off, reverse), "alsep_vr_lstm")
    got = host(y)
    assert np.all(got[T * N * stride:] == SENT)
    got = got[:T * N * stride].reshape(T, N, stride)
    assert np.all(got[..., :off] == SENT) and np.all(got[..., off + hidden:] == SENT)
    _close(got[..., off:off + hidden], want, RED, "alsep_vr_lstm")


def test_lstm_unsupported_hidden_size(dev):
    t = dev.zeros((9 * 3 * 4 * 48,))
    with pytest.raises(AlsepError, match="hidden size 48"):
        dev.check(dev.lib.alsep_vr_lstm(dev.handle, _lib.ptr(t), _lib.ptr(t), _lib.ptr(t), 9, 3, 48, 96, 0, 0), "alsep_vr_lstm")


# ------------------------------------------------------------------------------------------ multi-band front / back end (nn.hip)
@pytest.mark.parametrize("with_gain", [False, True])
def test_band_crop(dev, with_gain):
    """out[c, o0 + i, t] = gain[i] * band[(2 c, 2 c + 1), f0 + i, t0 + t] as interleaved complex values"""
    Fb, Tb, f0, t0, hh, l, bins, o0 = 13, 11, 2, 3, 5, 7, 9, 3
    g = _gen(6)
    band, gain = torch.randn(4, Fb, Tb, generator=g) + 0.3, torch.rand(hh, generator=g) + 0.2
    src = band.double()[:, f0:f0 + hh, t0:t0 + l].reshape(2, 2, hh, l).permute(0, 2, 3, 1)   # [c, i, t, (re, im)]
    want = np.full((2, bins, l, 2), SENT, np.float64)
    want[:, o0:o0 + hh] = (src * (gain.double().reshape(1, hh, 1, 1) if with_gain else 1.0)).numpy()
    bd, gd, y = on(dev, band.clone()), on(dev, gain.clone()) if with_gain else None, _out(dev, want.size)
    dev.check(dev.lib.alsep_vr_band_crop(dev.handle, _lib.ptr(bd), _lib.ptr(y), _lib.ptr(gd), Fb, Tb, f0, t0, hh, l, bins, o0), "alsep_vr_band_crop")
    got = host(y)
    assert np.all(got[want.size:] == SENT)
    got = got[:want.size].reshape(want.shape)
    assert np.all(got[:, :o0] == SENT) and np.all(got[:, o0 + hh:] == SENT)
    if with_gain:
        _close(got, want, EW, "alsep_vr_band_crop")
    else:
        assert np.array_equal(got, want.astype(np.float32))


def test_split_pred(dev):
    """y = pred * exp(i angle(X)), v = X - y; angle(0) = 0"""
    n = 37
    g = _gen(7)
    pred, X = torch.rand(n, generator=g) + 0.1, torch.randn(n, 2, generator=g) + 0.3
    X[[0, 5, 36]] = 0.0
    X[7, 1] = 0.0
    yw = pred.double().numpy() * np.exp(1j * np.angle(_cplx(X)))
    vw = _cplx(X) - yw
    pd, xd, y, v = on(dev, pred.clone()), on(dev, X.clone()), _out(dev, 2 * n), _out(dev, 2 * n)
    dev.check(dev.lib.alsep_vr_split_pred(dev.handle, _lib.ptr(pd), _lib.ptr(xd), _lib.ptr(y), _lib.ptr(v), n), "alsep_vr_split_pred")
    gy, gv = host(y), host(v)
    assert np.all(gy[2 * n:] == SENT) and np.all(gv[2 * n:] == SENT)
    _close(gy[:2 * n], _pairs(yw), EW, "y")
    _close(gv[:2 * n], _pairs(vw), EW, "v")
    assert np.array_equal(gy[:2 * n].reshape(n, 2)[[0, 5, 36]], np.stack([pred[[0, 5, 36]].numpy(), np.zeros(3, np.float32)], 1))


def test_mirror(dev):
    """spec_utils.mirroring("mirroring"): mirror = flip(|spec_m[:, lo : lo + hh]|, bins) * exp(i angle(he)); out = he where |he| <= |mirror|"""
    bins, hh, l, lo = 17, 5, 7, 4
    g = _gen(8)
    spec_m, he = torch.randn(2, bins, l, 2, generator=g) + 0.3, torch.randn(2, hh, l, 2, generator=g) * 1.3 - 0.2
    he[1, 2, 3] = 0.0
    hz = _cplx(he)
    mag = np.abs(_cplx(spec_m))[:, lo:lo + hh][:, ::-1]
    mirror = mag * np.exp(1j * np.angle(hz))
    keep = np.abs(hz) <= mag
    assert keep.any() and (~keep).any() and np.min(np.abs(np.abs(hz) - mag)) > 1e-5          # both branches, no tie float32 could flip
    want = np.where(keep, hz, mirror)
    sd, hd, y = on(dev, spec_m.clone()), on(dev, he.clone()), _out(dev, he.numel())
    dev.check(dev.lib.alsep_vr_mirror(dev.handle, _lib.ptr(sd), _lib.ptr(hd), _lib.ptr(y), bins, hh, l, lo), "alsep_vr_mirror")
    got = host(y)
    assert np.all(got[he.numel():] == SENT)
    got = got[:he.numel()].reshape(2, hh, l, 2)
    assert np.array_equal(got[keep], he.numpy()[keep]) and np.all(got[1, 2, 3] == 0.0)       # he itself, bit for bit
    _close(got, _pairs(want), EW, "alsep_vr_mirror")


@pytest.mark.parametrize("with_extra", [True, False])
def test_band_spec(dev, with_extra):
    """bins [o0, o0 + h) of spec_m at [f0, f0 + h), then `extra` at [e0, e0 + eh) over it (it overlaps the last two bins of the main
    window), everything times gain[f], zero elsewhere"""
    bins, l, Fb, f0, hh, o0, e0, eh = 17, 7, 13, 2, 6, 5, 6, 4
    g = _gen(9)
    spec_m, extra = torch.randn(2, bins, l, 2, generator=g) + 0.3, torch.randn(2, eh, l, 2, generator=g) - 0.4
    gain = torch.rand(Fb, generator=g) + 0.2
    z = np.zeros((2, Fb, l), np.complex128)
    z[:, f0:f0 + hh] = _cplx(spec_m)[:, o0:o0 + hh]
    if with_extra:
        z[:, e0:e0 + eh] = _cplx(extra)
    z *= gain.double().numpy()[None, :, None]
    want = np.stack([z[0].real, z[0].imag, z[1].real, z[1].imag])                            # [4, Fb, l]
    sd, ed, gd, y = on(dev, spec_m.clone()), on(dev, extra.clone()) if with_extra else None, on(dev, gain.clone()), _out(dev, want.size)
    dev.check(dev.lib.alsep_vr_band_spec(dev.handle, _lib.ptr(sd), _lib.ptr(ed), _lib.ptr(gd), _lib.ptr(y), bins, l, Fb, f0, hh, o0,
                                         e0 if with_extra else 0, eh if with_extra else 0), "alsep_vr_band_spec")
    got = host(y)
    assert np.all(got[want.size:] == SENT)
    got = got[:want.size].reshape(want.shape)
    assert np.all(got[want == 0.0] == 0.0)
    _close(got, want, EW, "alsep_vr_band_spec")


# ------------------------------------------------------------------------------------------ argument guards
def test_bad_arguments_are_rejected(dev):
    lib, h = dev.lib, dev.handle
    t = dev.zeros((256,))
    p = _lib.ptr(t)
    calls = {
        "alsep_vr_depthwise": lambda: lib.alsep_vr_depthwise(h, p, p, p, 1, 4, 4, 2, 3, 3, 2, 1),              # pad 2 with a 3 x 3 kernel grows the image
        "alsep_vr_resize_bilinear": lambda: lib.alsep_vr_resize_bilinear(h, p, p, 1, 2, 2, 3, 4, 4, 4, 2),      # slice past the last channel
        "alsep_vr_copy_slice": lambda: lib.alsep_vr_copy_slice(h, p, p, 2, 5, 2, 3, 3, 2, 0),                   # w_off + Wy > Wx
        "alsep_vr_mean_h": lambda: lib.alsep_vr_mean_h(h, p, p, 1, 0, 4, 2),
        "alsep_vr_mask": lambda: lib.alsep_vr_mask(h, p, p, p, 1, 5, 4, 2, 2, 1, 0.1),                          # Hout < Hm
        "alsep_vr_lstm": lambda: lib.alsep_vr_lstm(h, p, p, p, 2, 1, 16, 20, 8, 0),                             # out_off + hidden > out_stride
        "alsep_vr_band_crop": lambda: lib.alsep_vr_band_crop(h, p, p, None, 5, 4, 3, 0, 3, 2, 4, 0),            # f0 + h > Fb
        "alsep_vr_split_pred": lambda: lib.alsep_vr_split_pred(h, p, p, p, p, 0),
        "alsep_vr_mirror": lambda: lib.alsep_vr_mirror(h, p, p, p, 6, 3, 2, 4),                                 # lo + hh > bins
        "alsep_vr_band_spec": lambda: lib.alsep_vr_band_spec(h, p, None, p, p, 6, 2, 5, 3, 3, 0, 0, 0),         # f0 + h > Fb
    }
    for name, call in calls.items():
        with pytest.raises(AlsepError, match=name):
            dev.check(call(), name)
    dev.synchronize()
    assert float(t.abs().max()) == 0.0
