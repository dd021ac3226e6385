"""The entry points of csrc/nsf.h one at a time, each body on the CPU emulation and on the GPU through ``dev``, against torch.nn.functional in
float64 (the source against tests/nsf_oracle.py).

Bounds.  Convolution, transposed convolution, conv_post: max |delta| < 1e-5 of the output's peak, the bound of test_rmvpe_kernels.py.  For
every listed shape torch's own float32 result on the CPU was checked against float64 first; ``_f32_discrepancy`` below does it again on
every run and hands back the bound: 1e-5, or 4 x that discrepancy where it is above a third of 1e-5.  The largest seen, on two different
hosts: 1.3e-6 of the peak for the convolutions ((9, 192, 32, 7, 1): 1344 products an output), 2.5e-7 for the transposed ones
((7, 32, 16, 24, 12, 200)), 1.3e-6 for conv_post ((1, 16)).  All are inside a third of 1e-5 (3.3e-6), so every shape ran at 1e-5 there.
The kernels themselves measured 1.2e-6, 4.6e-7 and 3.5e-7 on the MI355X.  Source: 1e-5 absolute on |har| < 1; the kernel and the oracle
share the float32 steps and the float64 sum, what differs is the order of the float64 additions (1e-13), the float64 sine and the float32
tanh (1e-7); measured 2.6e-8.

The written tensor sits inside a larger buffer of 7.0: nothing outside [0, L) may change."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from audiolab_amd import nsf
from audiolab_amd._lib import AlsepError
from tests import nsf_oracle as o
from tests.conftest import host, on

GUARD = 7.0


def _guarded(dev, rows, cols, pad_rows=3):
    """a [rows, cols] view (16-byte aligned for cols % 4 == 0) in the middle of a buffer of 7.0"""
    buf = on(dev, torch.full(((rows + 2 * pad_rows) * cols,), GUARD))
    return buf, buf[pad_rows * cols:(pad_rows + rows) * cols].view(rows, cols)


def _surround_untouched(buf, rows, cols, pad_rows=3):
    b = host(buf)
    return bool(np.all(b[:pad_rows * cols] == GUARD) and np.all(b[(pad_rows + rows) * cols:] == GUARD))


def _f32_discrepancy(fn, *args):
    """-> (the float64 result, d = max |f32 - f64| / peak of torch's own float32 result on this CPU, the kernels' bound: 1e-5 of the peak
    where d stays within a third of it, 4 d where it does not)"""
    want = fn(*[a.double() if a is not None else None for a in args])
    got = fn(*[a.float() if a is not None else None for a in args])
    d = float((got.double() - want).abs().max() / want.abs().max())
    return want, d, (1e-5 if d < 1e-5 / 3 else 4 * d)


# ---- source ---------------------------------------------------------------------------------------------------------------------------------
def _f0_track(T, kind, seed):
    rng = np.random.default_rng(seed)
    if kind == "unvoiced":
        return np.zeros(T, dtype=np.float32)
    f0 = rng.uniform(60.0, 1100.0, T).astype(np.float32)                      # f0 / sr * upp up to 11 cycles at upp = 400: the step wraps
    if kind == "mixed":
        f0[rng.random(T) < 0.3] = 0.0
        if T > 8:
            f0[T // 2:T // 2 + 5] = 0.0
            f0[-1] = 440.0
    return f0


SOURCE_CASES = [(T, upp, "mixed") for T in (1, 2, 65, 1025) for upp in (6, 400)] + \
    [(T, upp, kind) for T in (2, 1025) for upp in (6, 400) for kind in ("voiced", "unvoiced")]


@pytest.mark.parametrize("T,upp,kind", SOURCE_CASES)
def test_source_matches_the_oracle(dev, T, upp, kind):
    sr = 40000
    f0 = _f0_track(T, kind, T * 7 + upp)
    if upp == 6 and kind != "unvoiced":
        f0 = f0 * np.float32(8.0)                                            # up to 8800 Hz: f0 / sr * 6 passes 0.5 and the step wraps
    noise = np.random.default_rng(T + upp).standard_normal(T * upp).astype(np.float32)
    lw, lb = 1.03, -0.02
    want = o.source(f0, noise, upp, sr, np.float32(lw), np.float32(lb))
    steps = o.steps(f0, sr, upp)
    if kind == "voiced":
        assert np.any(np.float64(f0) / sr * upp > 0.5) and np.all(np.abs(steps) <= 0.5)
    buf, har = _guarded(dev, T * upp, 1, pad_rows=8)
    nbytes = int(dev.lib.alsep_nsf_source_workspace_bytes(T))
    ws = dev.empty((nbytes // 8,), torch.float64)
    from audiolab_amd import _lib
    f0_d, noise_d = on(dev, f0), on(dev, noise)
    dev.check(dev.lib.alsep_nsf_source(dev.handle, _lib.ptr(f0_d), T, upp, sr, _lib.ptr(noise_d), lw, lb, _lib.ptr(har), _lib.ptr(ws), nbytes),
              "alsep_nsf_source")
    got = host(har).reshape(-1)
    err = float(np.max(np.abs(got - want)))
    print(f"source T={T} upp={upp} {kind}: max |delta| = {err:.3e}")
    assert err < 1e-5
    assert _surround_untouched(buf, T * upp, 1, pad_rows=8)
    assert np.array_equal(host(nsf.source(dev, f0_d, noise_d, upp, sr, lw, lb)), got)   # the wrapper, and bit-identical again


def test_source_phase_is_continuous_across_the_scan_chunk(dev):
    """a constant f0 whose step is not zero: the sine must run on without a jump from frame 1023 to 1024 (the scan's chunk edge)"""
    T, upp, sr = 1030, 6, 40000
    f0 = np.full(T, 1234.5, dtype=np.float32)
    noise = np.zeros(T * upp, dtype=np.float32)
    got = host(nsf.source(dev, on(dev, f0), on(dev, noise), upp, sr, 1.0, 0.0)).astype(np.float64)
    n = np.arange(1, T * upp + 1, dtype=np.float64)
    want = np.tanh(0.1 * np.sin(2.0 * np.pi * (np.float64(np.float32(1234.5) / np.float32(sr)) * n)))
    # the reference's per-frame step is float32: its rounding (6e-8 cycles a frame) adds up along the track; 1030 frames stay below 1e-4
    assert float(np.max(np.abs(got - want))) < 1e-4


@pytest.mark.parametrize("bad", ["frames", "upp", "sr", "workspace"])
def test_source_refusals(dev, bad):
    from audiolab_amd import _lib
    T, upp, sr = 4, 6, 40000
    f0, noise, har = dev.zeros((T,)), dev.zeros((T * upp,)), dev.zeros((T * upp,))
    ws = dev.empty((64,), torch.float64)
    args = dict(T=T, upp=upp, sr=sr, nbytes=512)
    args.update({"frames": dict(T=0), "upp": dict(upp=1025), "sr": dict(sr=0), "workspace": dict(nbytes=8)}[bad])
    rc = dev.lib.alsep_nsf_source(dev.handle, _lib.ptr(f0), args["T"], args["upp"], args["sr"], _lib.ptr(noise), 1.0, 0.0, _lib.ptr(har), _lib.ptr(ws),
                                  args["nbytes"])
    assert rc != 0
    assert int(dev.lib.alsep_nsf_source_workspace_bytes(0)) == -1 and int(dev.lib.alsep_nsf_source_workspace_bytes((1 << 20) + 1)) == -1


# ---- the pre-activation convolution --------------------------------------------------------------------------------------------------------
CONV_SHAPES = [(1, 16, 16, 3, 1), (17, 16, 32, 7, 3), (130, 32, 16, 11, 5), (9, 192, 32, 7, 1), (257, 64, 64, 3, 5)]


def _conv_ref(x, w, bias, res, acc, d, slope, post, scale):
    def fn(x, w, bias, res, acc):
        K = w.shape[2]
        y = F.conv1d(F.leaky_relu(x, slope) if slope != 1.0 else x, w, bias, dilation=d, padding=d * (K - 1) // 2)
        if res is not None:
            y = y + res
        if post:
            y = torch.tanh(y)
        if acc is not None:
            y = y + acc
        return y * scale
    return _f32_discrepancy(fn, x, w, bias, res, acc)


@pytest.mark.parametrize("extras", ["none", "bias", "bias+res", "bias+res+acc"])
@pytest.mark.parametrize("slope", [1.0, 0.1])
@pytest.mark.parametrize("L,Cin,Cout,K,d", CONV_SHAPES)
def test_conv1d_matches_torch(dev, L, Cin, Cout, K, d, slope, extras):
    g = torch.Generator().manual_seed(L * 1000 + Cin + K)
    x = torch.randn(1, Cin, L, generator=g)
    w = torch.randn(Cout, Cin, K, generator=g) / np.sqrt(Cin * K)
    bias = torch.randn(Cout, generator=g) * 0.1 if "bias" in extras else None
    res = torch.randn(1, Cout, L, generator=g) if "res" in extras else None
    acc = torch.randn(1, Cout, L, generator=g) if "acc" in extras else None
    scale = 1.0 / 3.0 if "acc" in extras else 1.0
    want, d32, bound = _conv_ref(x, w, bias, res, acc, d, slope, 0, scale)
    want = want[0].t().numpy()
    cl = lambda t: on(dev, t[0].t().contiguous()) if t is not None else None   # noqa: E731
    buf, y = _guarded(dev, L, Cout)
    nsf.conv1d(dev, cl(x), on(dev, w.permute(2, 1, 0).contiguous()), on(dev, bias) if bias is not None else None, cl(res), cl(acc), d, slope, 0,
               scale, out=y)
    got = host(y)
    err = float(np.max(np.abs(got - want))) / float(np.max(np.abs(want)))
    print(f"conv1d L={L} {Cin}->{Cout} K={K} d={d} slope={slope} {extras}: max |delta| / peak = {err:.3e} (torch float32: {d32:.3e})")
    assert err < bound
    assert _surround_untouched(buf, L, Cout)


def test_conv1d_tanh_and_in_place_residual(dev):
    L, Cc, K = 40, 16, 3
    g = torch.Generator().manual_seed(9)
    x, res = torch.randn(1, Cc, L, generator=g), torch.randn(1, Cc, L, generator=g)
    w = torch.randn(Cc, Cc, K, generator=g) / np.sqrt(Cc * K)
    want, _, bound = _conv_ref(x, w, None, res, None, 1, 0.1, 1, 1.0)
    y = on(dev, res[0].t().contiguous())                                     # the output over its own residual
    nsf.conv1d(dev, on(dev, x[0].t().contiguous()), on(dev, w.permute(2, 1, 0).contiguous()), res=y, pre_slope=0.1, post=1, out=y)
    assert float(np.max(np.abs(host(y) - want[0].t().numpy()))) < bound                  # |tanh| < 1: of a peak near 1


@pytest.mark.parametrize("post,with_acc,with_res", [(0, False, False), (1, False, False), (1, True, False), (1, True, True), (0, False, True)])
def test_conv1d_scale_and_tanh_combinations(dev, post, with_acc, with_res):
    """out_scale without acc, tanh with acc and scale, tanh with scale alone: y = out_scale (acc + post(conv + bias + res))"""
    L, Cin, Cout, K = 37, 16, 32, 5
    g = torch.Generator().manual_seed(17 + post + 2 * with_acc + 4 * with_res)
    x = torch.randn(1, Cin, L, generator=g)
    w = torch.randn(Cout, Cin, K, generator=g) / np.sqrt(Cin * K)
    bias = torch.randn(Cout, generator=g) * 0.1
    res = torch.randn(1, Cout, L, generator=g) if with_res else None
    acc = torch.randn(1, Cout, L, generator=g) if with_acc else None
    want, _, bound = _conv_ref(x, w, bias, res, acc, 2, 0.1, post, 1.0 / 3.0)
    want = want[0].t().numpy()
    cl = lambda t: on(dev, t[0].t().contiguous()) if t is not None else None   # noqa: E731
    buf, y = _guarded(dev, L, Cout)
    nsf.conv1d(dev, cl(x), on(dev, w.permute(2, 1, 0).contiguous()), on(dev, bias), cl(res), cl(acc), 2, 0.1, post, 1.0 / 3.0, out=y)
    assert float(np.max(np.abs(host(y) - want))) / float(np.max(np.abs(want))) < bound
    assert _surround_untouched(buf, L, Cout)


def test_conv1d_channels_in_eights(dev):
    """8 channels, the last stage of the reduced network: the tile's missing channels are masked"""
    L, Cin, Cout, K = 21, 8, 24, 5
    g = torch.Generator().manual_seed(3)
    x, w = torch.randn(1, Cin, L, generator=g), torch.randn(Cout, Cin, K, generator=g) / np.sqrt(Cin * K)
    want, _, bound = _conv_ref(x, w, None, None, None, 2, 0.1, 0, 1.0)
    buf, y = _guarded(dev, L, Cout)
    nsf.conv1d(dev, on(dev, x[0].t().contiguous()), on(dev, w.permute(2, 1, 0).contiguous()), dilation=2, pre_slope=0.1, out=y)
    want = want[0].t().numpy()
    assert float(np.max(np.abs(host(y) - want))) / float(np.max(np.abs(want))) < bound
    assert _surround_untouched(buf, L, Cout)


@pytest.mark.parametrize("Cin,Cout,K,d,post", [(12, 16, 3, 1, 0), (16, 20, 3, 1, 0), (16, 16, 4, 1, 0), (16, 16, 13, 1, 0), (16, 16, 3, 0, 0), (16, 16, 3, 6, 0),
                                                (16, 16, 3, 1, 2)])
def test_conv1d_refusals(dev, Cin, Cout, K, d, post):
    with pytest.raises(AlsepError):
        nsf.conv1d(dev, dev.zeros((4, Cin)), dev.zeros((K, Cin, Cout)), dilation=d, post=post)


def test_conv1d_refuses_output_over_input(dev):
    x = dev.zeros((4, 16))
    with pytest.raises(AlsepError):
        nsf.conv1d(dev, x, dev.zeros((3, 16, 16)), out=x)


# ---- conv_post ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,Cc", [(1, 16), (130, 32)])
def test_conv_post_matches_torch(dev, L, Cc):
    g = torch.Generator().manual_seed(L + Cc)
    x = torch.randn(1, Cc, L, generator=g)
    w = torch.randn(1, Cc, 7, generator=g) / np.sqrt(Cc * 7 / 2)
    want, d32, bound = _f32_discrepancy(lambda x, w: torch.tanh(F.conv1d(F.leaky_relu(x, 0.01), w, padding=3)), x, w)
    want = want.reshape(-1).numpy()
    buf, y = _guarded(dev, L, 1, pad_rows=8)
    from audiolab_amd import _lib
    x_d, w_d = on(dev, x[0].t().contiguous()), on(dev, w[0].t().contiguous())
    dev.check(dev.lib.alsep_nsf_conv_post(dev.handle, _lib.ptr(x_d), _lib.ptr(w_d), _lib.ptr(y), L, Cc), "alsep_nsf_conv_post")
    err = float(np.max(np.abs(host(y).reshape(-1) - want))) / float(np.max(np.abs(want)))
    print(f"conv_post L={L} C={Cc}: max |delta| / peak = {err:.3e} (torch float32: {d32:.3e})")
    assert err < bound
    assert _surround_untouched(buf, L, 1, pad_rows=8)
    assert np.array_equal(host(nsf.conv_post(dev, x_d, w_d)), host(y).reshape(-1))


def test_conv_post_refuses_odd_channels(dev):
    with pytest.raises(AlsepError):
        nsf.conv_post(dev, dev.zeros((4, 12)), dev.zeros((7, 12)))


# ---- the upsampling stage --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,Cin,Cout,K,u,s", [(1, 32, 16, 4, 2, 1), (5, 32, 16, 7, 3, 2), (13, 64, 32, 16, 10, 40), (7, 32, 16, 24, 12, 200),
                                              (140, 16, 16, 16, 6, 2), (5, 32, 16, 16, 4, 8), (131, 16, 16, 16, 2, 1)])
def test_tconv1d_matches_torch(dev, L, Cin, Cout, K, u, s):
    g = torch.Generator().manual_seed(L * 100 + K)
    ks = 2 * s if s > 1 else 1
    x = torch.randn(1, Cin, L, generator=g)
    w = torch.randn(Cin, Cout, K, generator=g) * np.sqrt(u / (Cin * K))
    bias = torch.randn(Cout, generator=g) * 0.1
    har = torch.tanh(torch.randn(1, 1, L * u * s, generator=g))
    nw = torch.randn(Cout, 1, ks, generator=g) / np.sqrt(ks)
    nb = torch.randn(Cout, generator=g) * 0.1

    def fn(x, w, bias, har, nw, nb):
        return F.conv_transpose1d(F.leaky_relu(x, 0.1), w, bias, stride=u, padding=(K - u) // 2) + \
            F.conv1d(har, nw, nb, stride=s, padding=s // 2 if s > 1 else 0)
    want, d32, bound = _f32_discrepancy(fn, x, w, bias, har, nw, nb)
    want = want[0].t().numpy()
    assert want.shape == (L * u, Cout)
    buf, y = _guarded(dev, L * u, Cout)
    nsf.tconv1d(dev, on(dev, x[0].t().contiguous()), on(dev, w.permute(2, 0, 1).contiguous()), on(dev, bias), on(dev, har.reshape(-1)),
                on(dev, nw[:, 0, :].t().contiguous()), on(dev, nb), u, s, out=y)
    err = float(np.max(np.abs(host(y) - want))) / float(np.max(np.abs(want)))
    print(f"tconv1d L={L} {Cin}->{Cout} K={K} u={u} s={s}: max |delta| / peak = {err:.3e} (torch float32: {d32:.3e})")
    assert err < bound
    assert _surround_untouched(buf, L * u, Cout)


@pytest.mark.parametrize("Cin,Cout,K,u,s", [(32, 16, 5, 2, 1), (32, 16, 2, 4, 1), (32, 16, 18, 2, 1), (32, 16, 4, 2, 3), (12, 16, 4, 2, 1), (32, 20, 4, 2, 1)])
def test_tconv1d_refusals(dev, Cin, Cout, K, u, s):
    """K - u odd; K < u; K > 8 u (more than 8 taps a phase); an odd source stride; channels not in eights"""
    from audiolab_amd import _lib
    L, ks = 3, 2 * s if s > 1 else 1
    z = lambda *shape: dev.zeros(shape)                                      # noqa: E731
    t = [z(L, Cin), z(K, Cin, Cout), z(Cout), z(L * u * s), z(ks, Cout), z(Cout), z(L * u, Cout)]
    rc = dev.lib.alsep_nsf_tconv1d(dev.handle, *[_lib.ptr(v) for v in t], L, Cin, Cout, K, u, s)
    assert rc != 0
    with pytest.raises(AlsepError):
        nsf.tconv1d(dev, z(L, Cin), z(K, Cin, Cout), z(Cout), z(L * u * s), z(ks, Cout), z(Cout), u, s)


# ---- alignment and length rules: refused before any launch -----------------------------------------------------------------------------------
def _misaligned(dev, n):
    """n floats 4 bytes off a 16-byte boundary"""
    return dev.zeros((n + 4,))[1:n + 1]


@pytest.mark.parametrize("which", ["x", "w", "y"])
def test_conv1d_refuses_a_misaligned_pointer(dev, which):
    from audiolab_amd import _lib
    L, Cc, K = 4, 16, 3
    t = {"x": dev.zeros((L * Cc,)), "w": dev.zeros((K * Cc * Cc,)), "y": dev.zeros((L * Cc,))}
    t[which] = _misaligned(dev, t[which].numel())
    assert t[which].data_ptr() % 16 == 4
    rc = dev.lib.alsep_nsf_conv1d(dev.handle, _lib.ptr(t["x"]), _lib.ptr(t["w"]), None, None, None, _lib.ptr(t["y"]), L, Cc, Cc, K, 1, 1.0, 0, 1.0)
    assert rc != 0
    assert b"16-byte aligned" in dev.lib.alsep_last_error(dev.handle)


def test_conv_post_refuses_a_misaligned_pointer(dev):
    from audiolab_amd import _lib
    L, Cc = 4, 16
    x, w, y = _misaligned(dev, L * Cc), dev.zeros((7 * Cc,)), dev.zeros((L,))
    assert dev.lib.alsep_nsf_conv_post(dev.handle, _lib.ptr(x), _lib.ptr(w), _lib.ptr(y), L, Cc) != 0
    x, w = dev.zeros((L * Cc,)), _misaligned(dev, 7 * Cc)
    assert dev.lib.alsep_nsf_conv_post(dev.handle, _lib.ptr(x), _lib.ptr(w), _lib.ptr(y), L, Cc) != 0


@pytest.mark.parametrize("which", [0, 1, 2, 4, 5, 6])
def test_tconv1d_refuses_a_misaligned_pointer(dev, which):
    """x, w, bias, noise_w, noise_b, y (the source har is read one float at a time and may sit anywhere)"""
    from audiolab_amd import _lib
    L, Cin, Cout, K, u, s = 3, 32, 16, 4, 2, 1
    t = [dev.zeros((L * Cin,)), dev.zeros((K * Cin * Cout,)), dev.zeros((Cout,)), dev.zeros((L * u * s,)), dev.zeros((Cout,)), dev.zeros((Cout,)),
         dev.zeros((L * u * Cout,))]
    t[which] = _misaligned(dev, t[which].numel())
    rc = dev.lib.alsep_nsf_tconv1d(dev.handle, *[_lib.ptr(v) for v in t], L, Cin, Cout, K, u, s)
    assert rc != 0
    assert b"16-byte aligned" in dev.lib.alsep_last_error(dev.handle)
    t[which], t[3] = dev.zeros((t[which].numel(),)), _misaligned(dev, L * u * s)
    assert dev.lib.alsep_nsf_tconv1d(dev.handle, *[_lib.ptr(v) for v in t], L, Cin, Cout, K, u, s) == 0


def test_lengths_beyond_the_index_range_are_refused(dev):
    """L >= 2^31 for the convolutions, L u >= 2^31 for the upsampling stage: refused on the host, nothing is launched or read"""
    from audiolab_amd import _lib
    a, b = dev.zeros((64,)), dev.zeros((64,))
    p, q = _lib.ptr(a), _lib.ptr(b)
    assert dev.lib.alsep_nsf_conv1d(dev.handle, p, p, None, None, None, q, 1 << 31, 16, 16, 3, 1, 1.0, 0, 1.0) != 0
    assert dev.lib.alsep_nsf_conv1d(dev.handle, p, p, None, None, None, q, 0, 16, 16, 3, 1, 1.0, 0, 1.0) != 0
    assert dev.lib.alsep_nsf_conv_post(dev.handle, p, p, q, 1 << 31, 16) != 0
    assert dev.lib.alsep_nsf_tconv1d(dev.handle, p, p, p, p, p, p, q, 1 << 30, 16, 16, 4, 2, 1) != 0
    assert b"too long" in dev.lib.alsep_last_error(dev.handle)
