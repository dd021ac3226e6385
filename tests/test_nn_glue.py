"""Direct tests of the small fp32 kernels of csrc/nn.hip and csrc/nn_hdemucs.h that the model tests reach only inside a whole network:
normalisation (both apply arms, every statistics-slab count), mean / std, activations, the residual adds, the overlap-add helpers, padding,
the transposed-convolution fold, RMSNorm, rotary embedding and the gates.  Every reference is the operation's own definition evaluated in
float64 on the CPU (the torch function the kernel's comment names); the same bodies run on the emulation and on cuda:0.

Tolerances: data movement is bit-exact; one-rounding / transcendental element-wise kernels 1e-6 * max(1, max|want|); anything with a
statistic or a reduction 2e-5 * max(1, max|want|); the rotary embedding has a bound derived in its test.  Where a launch site chooses between
a four-wide and a scalar kernel, both are run on the same data (a view one float into a larger allocation is not 16-byte aligned) and must
agree bit for bit, since they perform the same float32 operations per element."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from audiolab_amd import _lib
from audiolab_amd._lib import AlsepError
from tests.conftest import host, on

SENT = 7.25                 # pre-fill of every destination: whatever a kernel must not touch still holds it afterwards
EW, RED = 1e-6, 2e-5


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _mis(dev, t):
    """a copy of t on the device that starts one float into a larger allocation (data_ptr() % 16 == 4)"""
    buf = dev.empty((t.numel() + 7,), t.dtype)
    v = buf[1:1 + t.numel()]
    v.copy_(t.reshape(-1))
    assert buf.data_ptr() % 16 == 0 and v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def _put(dev, t, mis=False):
    """t on the device in an allocation of its own (never the host tensor's memory: several kernels work in place)"""
    return _mis(dev, t) if mis else on(dev, t.clone().reshape(-1))


def _out(dev, n, mis=False, tail=5):
    """n floats followed by `tail` more, all holding the sentinel"""
    t = torch.full((n + tail,), SENT)
    return _mis(dev, t) if mis else on(dev, t)


def _close(got, want, tol, what=""):
    want = want.detach().numpy() if isinstance(want, torch.Tensor) else np.asarray(want)
    got = np.asarray(got, dtype=np.float64).reshape(want.shape)
    err, bound = float(np.max(np.abs(got - want))), tol * max(1.0, float(np.max(np.abs(want))))
    assert np.all(np.isfinite(got)) and err < bound, f"{what}: max|delta| {err:.3e} >= {bound:.3e}"


def _act64(w, act, dim=-1):
    if act == 1:
        return torch.relu(w)
    if act == 3:
        return 0.5 * w * (1.0 + torch.erf(w / 2 ** 0.5))       # nn.GELU() (erf form)
    if act == 4:
        return F.glu(w, dim)
    if act == 5:
        return torch.tanh(w)
    return w


def _ws(dev, G, per_group):
    return dev.empty((int(dev.lib.alsep_nn_stats_workspace_bytes(G, per_group)),), torch.uint8)


# ------------------------------------------------------------------------------------------ alsep_nn_norm
def _norm_want(x, gamma, beta, G, R, C, act):
    g64, b64 = (gamma.double(), beta.double()) if gamma is not None else (None, None)
    if R == 1:                                                   # nn.LayerNorm(C)
        return _act64(F.layer_norm(x.double().reshape(G, 1, C), (C,), g64, b64, 1e-5), act)
    w = F.group_norm(x.double().reshape(G, R, C).permute(0, 2, 1), 1, g64, b64, 1e-5)      # nn.GroupNorm(1, C) on [G, C, R]
    return _act64(w, act, 1).permute(0, 2, 1)


def _norm_run(dev, x, gamma, beta, G, R, C, act, mis_x=False, mis_y=False, mis_gb=False):
    n_out = G * R * (C // 2 if act == 4 else C)
    xd, y = _put(dev, x, mis_x), _out(dev, n_out, mis_y)
    gd = _put(dev, gamma, mis_gb) if gamma is not None else None
    bd = _put(dev, beta, mis_gb) if gamma is not None else None
    ws = _ws(dev, G, R * C)
    dev.check(dev.lib.alsep_nn_norm(dev.handle, _lib.ptr(xd), _lib.ptr(y), _lib.ptr(gd), _lib.ptr(bd), G, R, C, 1e-5, act, _lib.ptr(ws)),
              "alsep_nn_norm")
    got = host(y)
    assert np.all(got[n_out:] == SENT)
    return got[:n_out]


def _norm_data(G, R, C, affine, seed):
    g = _gen(seed)
    x = torch.randn(G, R, C, generator=g) * 1.5 + 0.4
    if not affine:
        return x, None, None
    return x, 1 + 0.3 * torch.randn(C, generator=g), 0.2 + 0.3 * torch.randn(C, generator=g)


@pytest.mark.parametrize("G,R,C,act,affine", [
    (5, 7, 12, 0, True),          # four-wide apply
    (5, 7, 12, 0, False),         # ... without gamma / beta
    (5, 7, 12, 4, True),          # GLU, Co = 6: the scalar apply although C % 4 == 0
    (3, 9, 8, 4, True),           # GLU, Co = 4: four-wide
    (3, 9, 8, 4, False),
    (3, 9, 8, 3, True),           # GELU, four-wide
    (4, 11, 6, 3, True),          # C % 4 != 0
    (4, 11, 6, 0, False),
    (37, 1, 48, 0, True),         # LayerNorm form
    (2, 1, 70001, 0, True),       # 3 slabs per group, scalar statistics
    (3, 16385, 4, 0, True),       # 3 slabs with quad-rounded edges: 16385 quads in chunks of 5462, 5462, 5461
    (300, 1, 40000, 0, False),    # G >= 256: one slab although the group has more than 32768 elements
])
def test_norm_vs_float64(dev, G, R, C, act, affine):
    x, gamma, beta = _norm_data(G, R, C, affine, G * 1000 + C + act)
    want = _norm_want(x, gamma, beta, G, R, C, act)
    _close(_norm_run(dev, x, gamma, beta, G, R, C, act), want, RED, "alsep_nn_norm")


@pytest.mark.parametrize("G,R,C,act", [(5, 7, 12, 0), (5, 7, 12, 3), (3, 9, 8, 4), (3, 16385, 4, 0)])
def test_norm_four_wide_and_scalar_arms_agree(dev, G, R, C, act):
    """any pointer off a 16-byte boundary selects the scalar apply kernel; with x aligned both runs share the statistics kernel, so the
    results are the same bits.  x itself misaligned also moves the statistics to the scalar kernel, whose summation order differs: that
    run is held to float64 only."""
    x, gamma, beta = _norm_data(G, R, C, True, G + R + C)
    want = _norm_want(x, gamma, beta, G, R, C, act)
    aligned = _norm_run(dev, x, gamma, beta, G, R, C, act)
    _close(aligned, want, RED, "aligned")
    for kw in (dict(mis_y=True), dict(mis_gb=True)):
        got = _norm_run(dev, x, gamma, beta, G, R, C, act, **kw)
        assert np.array_equal(got, aligned), kw
    _close(_norm_run(dev, x, gamma, beta, G, R, C, act, mis_x=True), want, RED, "x misaligned")
    _close(_norm_run(dev, x, gamma, beta, G, R, C, act, mis_x=True, mis_y=True), want, RED, "x, y misaligned")


@pytest.mark.parametrize("G,R,C", [(5, 7, 12), (4, 11, 6)])
def test_norm_of_data_far_from_zero(dev, G, R, C):
    """mean 50, std 0.01: var = q / n - mean^2 cancels eleven digits in fp64 and the mean itself does not fit a float32 to better than
    2e-6, which is 2e-4 standard deviations.  The normalised output is still held to 2e-5 * max(1, max|want|)."""
    g = _gen(G)
    x = 50.0 + 0.01 * torch.randn(G, R, C, generator=g)
    gamma, beta = 1 + 0.3 * torch.randn(C, generator=g), 0.2 + 0.3 * torch.randn(C, generator=g)
    want = _norm_want(x, gamma, beta, G, R, C, 0)
    _close(_norm_run(dev, x, gamma, beta, G, R, C, 0), want, RED, "aligned")
    _close(_norm_run(dev, x, gamma, beta, G, R, C, 0, mis_x=True, mis_y=True), want, RED, "misaligned")


# ------------------------------------------------------------------------------------------ alsep_nn_meanstd / alsep_nn_affine_stats
def _meanstd(dev, x_ptr, nsamples, per, stats_ptr, ws):
    dev.check(dev.lib.alsep_nn_meanstd(dev.handle, x_ptr, nsamples, per, stats_ptr, _lib.ptr(ws)), "alsep_nn_meanstd")


def _stats_want(x):
    x64 = x.double()
    return torch.stack([x64.mean(1), x64.std(1)], 1)            # torch.std: unbiased


@pytest.mark.parametrize("nsamples,per", [
    (3, 7), (1, 1001), (3, 1000),     # scalar and four-wide, one slab
    (1, 70001),                       # 3 slabs, scalar
    (3, 65540),                       # 3 slabs of 5462, 5462, 5461 quads
])
def test_meanstd_vs_torch_std(dev, nsamples, per):
    x = torch.randn(nsamples, per, generator=_gen(per)) * 1.3 + 0.7
    want = _stats_want(x)
    xd, st = _put(dev, x), _out(dev, 2 * nsamples)
    _meanstd(dev, _lib.ptr(xd), nsamples, per, _lib.ptr(st), _ws(dev, nsamples, per))
    got = host(st)
    assert np.all(got[2 * nsamples:] == SENT)
    _close(got[:2 * nsamples], want, RED, "alsep_nn_meanstd")


def test_meanstd_of_single_values(dev):
    x = torch.randn(3, 1, generator=_gen(1)) + 0.5
    xd, st = _put(dev, x), _out(dev, 6)
    _meanstd(dev, _lib.ptr(xd), 3, 1, _lib.ptr(st), _ws(dev, 3, 1))
    got = host(st)[:6].reshape(3, 2)
    assert np.array_equal(got[:, 0], x[:, 0].numpy()) and np.all(got[:, 1] == 0.0)


@pytest.mark.parametrize("n,mis", [(1001, False), (1000, False), (1000, True)])
def test_meanstd_item_by_item(dev, n, mis):
    """one call per batch item at x + b * n, the way HTDemucs normalises a batch: with n % 4 == 1 the items start at every residue of
    16 bytes, with n % 4 == 0 the base pointer alone decides between the four-wide and the scalar statistics kernel"""
    B = 3
    x = torch.randn(B, n, generator=_gen(n + mis)) * 0.8 - 0.6
    want = _stats_want(x)
    xd, st, ws = _put(dev, x, mis), _out(dev, 2 * B), _ws(dev, 1, n)
    for b in (2, 0, 1):
        _meanstd(dev, C.c_void_p(xd.data_ptr() + 4 * b * n), 1, n, C.c_void_p(st.data_ptr() + 8 * b), ws)
        dev.synchronize()
    got = host(st)
    assert np.all(got[2 * B:] == SENT)
    _close(got[:2 * B], want, RED, "alsep_nn_meanstd per item")


@pytest.mark.parametrize("nsamples,per", [(1, 1000), (3, 1001)])
def test_affine_stats_round_trip(dev, nsamples, per):
    """y = (x - mean) / (eps + std) with the statistics alsep_nn_meanstd produced, and back: both against float64"""
    x = torch.randn(nsamples, per, generator=_gen(per + 1)) * torch.tensor([[1.7], [0.4], [3.0]])[:nsamples] + 0.9
    eps = 1e-5
    m64, s64 = x.double().mean(1, keepdim=True), x.double().std(1, keepdim=True)
    want = (x.double() - m64) / (eps + s64)
    xd, st, y, z = _put(dev, x), _out(dev, 2 * nsamples), _out(dev, x.numel()), _out(dev, x.numel())
    _meanstd(dev, _lib.ptr(xd), nsamples, per, _lib.ptr(st), _ws(dev, nsamples, per))
    dev.check(dev.lib.alsep_nn_affine_stats(dev.handle, _lib.ptr(xd), _lib.ptr(y), _lib.ptr(st), nsamples, per, eps, 0), "alsep_nn_affine_stats")
    dev.check(dev.lib.alsep_nn_affine_stats(dev.handle, _lib.ptr(y), _lib.ptr(z), _lib.ptr(st), nsamples, per, eps, 1), "alsep_nn_affine_stats")
    gy, gz = host(y), host(z)
    assert np.all(gy[x.numel():] == SENT) and np.all(gz[x.numel():] == SENT)
    _close(gy[:x.numel()], want, RED, "forward")
    _close(gz[:x.numel()], want * s64 + m64, RED, "inverse")     # x * std + mean of the forward result (eps apart from x itself)


# ------------------------------------------------------------------------------------------ alsep_nn_group_norm
@pytest.mark.parametrize("G", [1, 4])
@pytest.mark.parametrize("act", [0, 3, 4])
def test_group_norm_row_window_vs_torch(dev, G, act):
    B, R, Cn, r0 = 2, 9, 12, 2
    Ro, Co = R - 3, Cn // 2 if act == 4 else Cn
    g = _gen(G * 10 + act)
    x = torch.randn(B, R, Cn, generator=g) * 1.4 + torch.arange(Cn) * 0.1
    gamma, beta = 1 + 0.3 * torch.randn(Cn, generator=g), 0.2 + 0.3 * torch.randn(Cn, generator=g)
    w = F.group_norm(x.double().permute(0, 2, 1), G, gamma.double(), beta.double(), 1e-5)     # nn.GroupNorm(G, C) on [B, C, R]
    want = _act64(w, act, 1).permute(0, 2, 1)[:, r0:r0 + Ro]
    xd, gd, bd, y, st = _put(dev, x), _put(dev, gamma), _put(dev, beta), _out(dev, B * Ro * Co), _out(dev, 2 * B * G)
    dev.check(dev.lib.alsep_nn_group_norm(dev.handle, _lib.ptr(xd), _lib.ptr(y), _lib.ptr(gd), _lib.ptr(bd), B, R, Cn, G, 1e-5, act, r0, Ro,
                                          _lib.ptr(st)), "alsep_nn_group_norm")
    got = host(y)
    assert np.all(got[B * Ro * Co:] == SENT) and np.all(host(st)[2 * B * G:] == SENT)
    _close(got[:B * Ro * Co], want, RED, "alsep_nn_group_norm")


# ------------------------------------------------------------------------------------------ alsep_nn_act / alsep_nn_scale_add
@pytest.mark.parametrize("Cn,act", [(8, 1), (8, 3), (8, 5), (8, 4), (16, 4), (6, 1), (6, 3), (6, 5), (6, 4), (12, 4)])
def test_act_both_arms(dev, Cn, act):
    """C = 8 / 16 take the four-wide kernel (GLU: Co = 4 / 8), C = 6 and GLU over C = 12 (Co = 6) the scalar one; off a 16-byte boundary
    everything takes the scalar one"""
    rows, Co = 7, Cn // 2 if act == 4 else Cn
    x = torch.randn(rows, Cn, generator=_gen(Cn * 10 + act)) * 1.5 + 0.3
    want = _act64(x.double(), act)
    res = []
    for mis in (False, True):
        xd, y = _put(dev, x, mis), _out(dev, rows * Co, mis)
        dev.check(dev.lib.alsep_nn_act(dev.handle, _lib.ptr(xd), _lib.ptr(y), rows, Cn, act), "alsep_nn_act")
        got = host(y)
        assert np.all(got[rows * Co:] == SENT)
        _close(got[:rows * Co], want, EW, f"alsep_nn_act mis={mis}")
        res.append(got)
    assert np.array_equal(res[0], res[1])


@pytest.mark.parametrize("Cn", [8, 6, 12])
@pytest.mark.parametrize("scaled", [False, True])
def test_scale_add_both_arms(dev, Cn, scaled):
    rows = 7
    g = _gen(Cn + scaled)
    a, b = torch.randn(rows, Cn, generator=g) + 0.5, torch.randn(rows, Cn, generator=g) * 2 - 0.3
    scale = 0.4 + torch.randn(Cn, generator=g) if scaled else None
    want = a.double() + (scale.double() * b.double() if scaled else b.double())
    res = []
    for mis in ((False,) * 4, (True,) * 4, (False, False, True, False), (False, False, False, True)):      # a, b, scale, y
        if mis[2] and not scaled:
            continue
        ad, bd, y = _put(dev, a, mis[0]), _put(dev, b, mis[1]), _out(dev, rows * Cn, mis[3])
        sd = _put(dev, scale, mis[2]) if scaled else None
        dev.check(dev.lib.alsep_nn_scale_add(dev.handle, _lib.ptr(ad), _lib.ptr(bd), _lib.ptr(sd), _lib.ptr(y), rows, Cn), "alsep_nn_scale_add")
        got = host(y)
        assert np.all(got[rows * Cn:] == SENT)
        _close(got[:rows * Cn], want, EW, f"alsep_nn_scale_add mis={mis}")
        res.append(got)
    assert all(np.array_equal(r, res[0]) for r in res[1:])


def test_mul(dev):
    n = 1003
    g = _gen(n)
    a, b = torch.randn(n, generator=g) + 0.5, torch.randn(n, generator=g) - 0.2
    ad, bd, y = _put(dev, a), _put(dev, b), _out(dev, n)
    dev.check(dev.lib.alsep_nn_mul(dev.handle, _lib.ptr(ad), _lib.ptr(bd), _lib.ptr(y), n), "alsep_nn_mul")
    got = host(y)
    assert np.all(got[n:] == SENT)
    _close(got[:n], a.double() * b.double(), EW, "alsep_nn_mul")


# ------------------------------------------------------------------------------------------ grid-stride wrap (65536 workgroups of 256)
@pytest.mark.gpu
def test_mul_beyond_one_grid(gpu_ctx):
    """more elements than 65536 workgroups x 256 threads: the tail is reached only by the grid-stride loop"""
    dev, n = gpu_ctx, 65536 * 256 + 1000
    g = torch.Generator(device=dev.device).manual_seed(1)
    a, b = torch.randn(n, generator=g, device=dev.device) + 0.5, torch.randn(n, generator=g, device=dev.device) - 0.2
    y = torch.full((n + 5,), SENT, device=dev.device)
    dev.check(dev.lib.alsep_nn_mul(dev.handle, _lib.ptr(a), _lib.ptr(b), _lib.ptr(y), n), "alsep_nn_mul")
    want = a.double() * b.double()
    err, bound = float((y[:n].double() - want).abs().max()), EW * max(1.0, float(want.abs().max()))
    assert err < bound and bool((y[n:] == SENT).all()), f"{err:.3e} >= {bound:.3e}"


@pytest.mark.gpu
def test_scale_add_beyond_one_grid_of_quads(gpu_ctx):
    """C = 8 and 2^24 + 334 quads (rows * C / 4 is even for C = 8): the four-wide kernel's unsigned grid-stride loop wraps once"""
    dev, Cn = gpu_ctx, 8
    rows = ((1 << 24) + 334) * 4 // Cn
    g = torch.Generator(device=dev.device).manual_seed(2)
    a, b = torch.randn(rows, Cn, generator=g, device=dev.device) + 0.5, torch.randn(rows, Cn, generator=g, device=dev.device) - 0.2
    scale = 0.4 + torch.randn(Cn, generator=g, device=dev.device)
    y = torch.full((rows * Cn + 8,), SENT, device=dev.device)
    dev.check(dev.lib.alsep_nn_scale_add(dev.handle, _lib.ptr(a), _lib.ptr(b), _lib.ptr(scale), _lib.ptr(y), rows, Cn), "alsep_nn_scale_add")
    want = torch.addcmul(a.double(), scale.double(), b.double())
    err, bound = float((y[:rows * Cn].double().reshape(rows, Cn) - want).abs().max()), EW * max(1.0, float(want.abs().max()))
    assert err < bound and bool((y[rows * Cn:] == SENT).all()), f"{err:.3e} >= {bound:.3e}"


# ------------------------------------------------------------------------------------------ broadcast add, overlap-add helpers
@pytest.mark.parametrize("shape,axis", [((2, 5, 3, 7), 1), ((3, 5, 7), 1)])
def test_add_bcast(dev, shape, axis):
    """frequency embedding over [B, F, T, C] (inner = T C, period = F) and positional embedding over [B, N, C] (inner = C, period = N)"""
    g = _gen(len(shape))
    y0 = torch.randn(*shape, generator=g) + 0.3
    period, Cn = shape[axis], shape[-1]
    e = torch.randn(period, Cn, generator=g) - 0.4
    inner = int(np.prod(shape[axis + 1:]))
    ev = e.double().reshape((1, period) + (1,) * (len(shape) - 3) + (Cn,))
    want = y0.double() + 0.3 * ev
    yd, ed = _put(dev, y0), _put(dev, e)
    dev.check(dev.lib.alsep_nn_add_bcast(dev.handle, _lib.ptr(yd), _lib.ptr(ed), 0.3, y0.numel(), inner, period, Cn), "alsep_nn_add_bcast")
    _close(host(yd), want, EW, "alsep_nn_add_bcast")


def test_vec_fma_with_row_strides(dev):
    rows, n, ys, xs = 3, 10, 13, 12
    g = _gen(7)
    y0, x = torch.randn(rows, ys, generator=g) + 0.2, torch.randn(rows, xs, generator=g) - 0.5
    w = torch.rand(n, generator=g) + 0.1
    want = y0.double().clone()
    want[:, :n] += w.double() * x.double()[:, :n]
    yd, xd, wd = _put(dev, y0), _put(dev, x), _put(dev, w)
    dev.check(dev.lib.alsep_nn_vec_fma(dev.handle, _lib.ptr(yd), _lib.ptr(xd), _lib.ptr(wd), rows, n, ys, xs), "alsep_nn_vec_fma")
    got = host(yd).reshape(rows, ys)
    assert np.array_equal(got[:, n:], y0[:, n:].numpy())         # the columns between the rows are not touched
    _close(got, want, EW, "alsep_nn_vec_fma")


def test_vec_div_zero_weights_give_zero(dev):
    rows, n = 3, 11
    g = _gen(8)
    y0 = torch.randn(rows, n, generator=g) + 0.4
    w = torch.rand(n, generator=g) + 0.2
    w[[0, 4, 10]] = 0.0
    want = torch.where(w.double() != 0, y0.double() / w.double(), torch.zeros((), dtype=torch.float64))
    yd, wd = _put(dev, torch.cat([y0.reshape(-1), torch.full((5,), SENT)])), _put(dev, w)
    dev.check(dev.lib.alsep_nn_vec_div(dev.handle, _lib.ptr(yd), _lib.ptr(wd), rows, n), "alsep_nn_vec_div")
    got = host(yd)
    assert np.all(got[rows * n:] == SENT)
    got = got[:rows * n].reshape(rows, n)
    assert np.all(got[:, [0, 4, 10]] == 0.0)
    _close(got, want, EW, "alsep_nn_vec_div")


# ------------------------------------------------------------------------------------------ data movement: bit-exact
@pytest.mark.parametrize("left,right", [(5, 5), (2, 0), (0, 3)])
def test_reflect_pad_vs_torch(dev, left, right):
    rows, n = 3, 6                                               # (5, 5): the longest reflection F.pad allows, n - 1 on both sides
    x = torch.randn(rows, n, generator=_gen(left)) + 0.3
    want = F.pad(x[None], (left, right), mode="reflect")[0].numpy()
    xd, y = _put(dev, x), _out(dev, want.size)
    dev.check(dev.lib.alsep_nn_reflect_pad(dev.handle, _lib.ptr(xd), _lib.ptr(y), rows, n, left, right), "alsep_nn_reflect_pad")
    got = host(y)
    assert np.all(got[want.size:] == SENT) and np.array_equal(got[:want.size].reshape(want.shape), want)


def test_swap_last2(dev):
    B, Cn, L = 2, 3, 5
    x = torch.randn(B, Cn, L, generator=_gen(9)) + 0.3
    xd, y = _put(dev, x), _out(dev, x.numel())
    dev.check(dev.lib.alsep_nn_swap_last2(dev.handle, _lib.ptr(xd), _lib.ptr(y), B, Cn, L), "alsep_nn_swap_last2")
    got = host(y)
    assert np.all(got[x.numel():] == SENT) and np.array_equal(got[:x.numel()].reshape(B, L, Cn), x.transpose(1, 2).numpy())


def test_depth_to_space2_into_a_channel_slice(dev):
    H, W, Co, ct, c0 = 3, 5, 2, 7, 4
    gsrc = torch.randn(H, W, 4 * Co, generator=_gen(10)) + 0.3
    want = np.full((2 * H, 2 * W, ct), SENT, np.float32)
    for dy in range(2):
        for dx in range(2):                                      # ConvTranspose2d(kernel = stride = 2): tap (dy, dx) lands on pixel (2 h + dy, 2 w + dx)
            want[dy::2, dx::2, c0:c0 + Co] = gsrc[:, :, (dy * 2 + dx) * Co:(dy * 2 + dx + 1) * Co].numpy()
    gd, y = _put(dev, gsrc), _out(dev, want.size)
    dev.check(dev.lib.alsep_nn_depth_to_space2(dev.handle, _lib.ptr(gd), _lib.ptr(y), H, W, Co, ct, c0), "alsep_nn_depth_to_space2")
    got = host(y)
    assert np.all(got[want.size:] == SENT) and np.array_equal(got[:want.size].reshape(want.shape), want)


# ------------------------------------------------------------------------------------------ alsep_nn_tconv_fold
@pytest.mark.parametrize("S,pad,short,bias,act,J", [
    (2, 0, False, True, 0, 5), (2, 1, True, False, 3, 1), (2, 3, False, True, 3, 5),
    (4, 0, True, True, 0, 1), (4, 2, False, False, 0, 5), (4, 3, True, True, 3, 5),
])
def test_tconv_fold_vs_conv_transpose(dev, S, pad, short, bias, act, J):
    """ConvTranspose2d([2 S, 1], stride [S, 1]) cropped by `pad`: the per-tap products g are computed on the host (float64, rounded to
    float32 once), the kernel adds the two taps that meet at an output row.  Two float32 additions of values rounded once: within
    1e-6 * max(1, max|want|)."""
    B, I, Cin, Co, K = 2, 3, 4, 7, 2 * S
    Lout = (I + 1) * S - pad - (3 if short else 0)
    g = _gen(S * 100 + pad * 10 + J)
    x = torch.randn(B, Cin, I, J, generator=g, dtype=torch.float64) + 0.3
    w = torch.randn(Cin, Co, K, 1, generator=g, dtype=torch.float64) * 0.5 + 0.1
    bv = torch.randn(Co, generator=g) - 0.2 if bias else None
    full = F.conv_transpose2d(x, w, bv.double() if bias else None, stride=(S, 1))          # [B, Co, (I + 1) S, J]
    want = _act64(full[:, :, pad:pad + Lout].permute(0, 2, 3, 1), act)                      # [B, Lout, J, Co]
    gh = torch.einsum("bcij,cok->bijko", x, w[..., 0]).reshape(B, I, J, K * Co).float()     # g[b, i, j, k * Co + co]
    gd, y = _put(dev, gh), _out(dev, want.numel())
    bd = _put(dev, bv) if bias else None
    dev.check(dev.lib.alsep_nn_tconv_fold(dev.handle, _lib.ptr(gd), _lib.ptr(bd), _lib.ptr(y), B, I, J, Co, S, pad, Lout, act), "alsep_nn_tconv_fold")
    got = host(y)
    assert np.all(got[want.numel():] == SENT)
    _close(got[:want.numel()], want, EW, "alsep_nn_tconv_fold")


# ------------------------------------------------------------------------------------------ Roformer blocks
@pytest.mark.parametrize("rows,Cn", [(9, 10), (5, 70)])
def test_rmsnorm_strided_and_in_place(dev, rows, Cn):
    """F.normalize(x, dim=-1) * sqrt(C) * gamma.  First from rows 3 floats wider than C into rows 5 floats wider, then in place on the
    columns [4, 4 + C) of a wider matrix; one row is all zero (0 / max(0, 1e-12) = 0)."""
    g = _gen(rows)
    gamma = 1 + 0.3 * torch.randn(Cn, generator=g)
    xs, ys = Cn + 3, Cn + 5
    x = torch.randn(rows, xs, generator=g) * 1.3 + 0.4
    x[2] = 0.0
    want = F.normalize(x.double()[:, :Cn], dim=-1) * Cn ** 0.5 * gamma.double()
    xd, gd, y = _put(dev, x), _put(dev, gamma), _out(dev, rows * ys)
    dev.check(dev.lib.alsep_nn_rmsnorm(dev.handle, _lib.ptr(xd), _lib.ptr(y), _lib.ptr(gd), rows, Cn, xs, ys), "alsep_nn_rmsnorm")
    got = host(y)[:rows * ys].reshape(rows, ys)
    assert np.all(got[:, Cn:] == SENT) and np.all(host(y)[rows * ys:] == SENT) and np.all(got[2, :Cn] == 0.0)
    _close(got[:, :Cn], want, RED, "alsep_nn_rmsnorm")
    width, c0 = Cn + 9, 4
    m = torch.randn(rows, width, generator=g) * 0.7 - 0.5
    m[1, c0:c0 + Cn] = 0.0
    want = F.normalize(m.double()[:, c0:c0 + Cn], dim=-1) * Cn ** 0.5 * gamma.double()
    md = _put(dev, m)
    p = C.c_void_p(md.data_ptr() + 4 * c0)
    dev.check(dev.lib.alsep_nn_rmsnorm(dev.handle, p, p, _lib.ptr(gd), rows, Cn, width, width), "alsep_nn_rmsnorm")
    got = host(md).reshape(rows, width)
    assert np.array_equal(got[:, :c0], m[:, :c0].numpy()) and np.array_equal(got[:, c0 + Cn:], m[:, c0 + Cn:].numpy())
    _close(got[:, c0:c0 + Cn], want, RED, "alsep_nn_rmsnorm in place")


@pytest.mark.parametrize("rows,stride,c0,heads,d,pos_div,pos_mod", [
    (45, 29, 5, 3, 6, 3, 7),          # positions 0 .. 6: the bound below is about 1e-5
    (803, 23, 3, 2, 8, 1, 801),       # positions up to 800
])
def test_rotary_vs_float64(dev, rows, stride, c0, heads, d, pos_div, pos_mod):
    """rotary_embedding_torch, interleaved pairs, theta 10000: pair j of a head turns by pos * 10000^(-2 j / d).  The kernel forms the
    angle in float32: powf, the reciprocal and the product are each good to about an ulp, so the angle is off by at most
    4 * 2^-23 * pos (relative 4 ulp, |angle| <= pos); a rotation by a wrong angle moves (a, b) by that angle times |(a, b)| <= sqrt(2) max|x|.
    The float32 sin / cos and the four products and two sums add about 1e-6 for |x| of a few units."""
    x = torch.randn(rows, stride, generator=_gen(rows)) * 1.2 + 0.3
    pos = ((torch.arange(rows) // pos_div) % pos_mod).double()
    inv = 10000.0 ** (-torch.arange(0, d, 2).double() / d)
    ang = pos[:, None] * inv[None, :]                            # [rows, d / 2]
    v = x.double()[:, c0:c0 + heads * d].reshape(rows, heads, d // 2, 2)
    cs, sn = torch.cos(ang)[:, None, :], torch.sin(ang)[:, None, :]
    want = torch.stack([v[..., 0] * cs - v[..., 1] * sn, v[..., 1] * cs + v[..., 0] * sn], -1).reshape(rows, heads * d)
    xd = _put(dev, x)
    dev.check(dev.lib.alsep_nn_rotary(dev.handle, _lib.ptr(xd), rows, stride, c0, heads, d, pos_div, pos_mod), "alsep_nn_rotary")
    got = host(xd).reshape(rows, stride)
    assert np.array_equal(got[:, :c0], x[:, :c0].numpy()) and np.array_equal(got[:, c0 + heads * d:], x[:, c0 + heads * d:].numpy())
    bound = 4 * 2.0 ** -23 * float(pos.max()) * 2 ** 0.5 * float(x.abs().max()) + 1e-6
    err = float(np.max(np.abs(got[:, c0:c0 + heads * d].astype(np.float64) - want.numpy())))
    assert err < bound, f"alsep_nn_rotary: max|delta| {err:.3e} >= {bound:.3e}"
    assert float((want - x.double()[:, c0:c0 + heads * d]).abs().max()) > 0.5       # the rotation is not a no-op at these positions


def test_gate(dev):
    rows, heads, d = 11, 3, 5
    g = _gen(11)
    o, gates = torch.randn(rows, heads * d, generator=g) + 0.3, torch.randn(rows, heads, generator=g) * 2 + 0.5
    want = o.double() * torch.sigmoid(gates.double()).repeat_interleave(d, dim=1)
    od, gd = _put(dev, torch.cat([o.reshape(-1), torch.full((5,), SENT)])), _put(dev, gates)
    dev.check(dev.lib.alsep_nn_gate(dev.handle, _lib.ptr(od), _lib.ptr(gd), rows, heads, d), "alsep_nn_gate")
    got = host(od)
    assert np.all(got[rows * heads * d:] == SENT)
    _close(got[:rows * heads * d], want, EW, "alsep_nn_gate")


# ------------------------------------------------------------------------------------------ argument guards
def test_bad_arguments_are_rejected(dev):
    """one representative bad argument per entry point: nothing is launched, AlsepError carries the entry point's name"""
    lib, h = dev.lib, dev.handle
    t = dev.zeros((256,))
    p = _lib.ptr(t)
    calls = {
        "alsep_nn_norm": lambda: lib.alsep_nn_norm(h, p, p, None, None, 2, 3, 5, 1e-5, 4, p),                  # GLU over an odd channel count
        "alsep_nn_meanstd": lambda: lib.alsep_nn_meanstd(h, p, 2, 0, p, p),
        "alsep_nn_affine_stats": lambda: lib.alsep_nn_affine_stats(h, p, p, p, 0, 8, 1e-5, 0),
        "alsep_nn_group_norm": lambda: lib.alsep_nn_group_norm(h, p, p, p, p, 1, 3, 10, 4, 1e-5, 0, 0, 3, p),  # C % G != 0
        "alsep_nn_act": lambda: lib.alsep_nn_act(h, p, p, 4, 8, 0),                                            # act 0 is not an activation
        "alsep_nn_scale_add": lambda: lib.alsep_nn_scale_add(h, p, p, None, p, 4, 0),
        "alsep_nn_add_bcast": lambda: lib.alsep_nn_add_bcast(h, p, p, 1.0, 64, 8, 0, 4),
        "alsep_nn_vec_fma": lambda: lib.alsep_nn_vec_fma(h, p, p, p, 2, 8, 7, 8),                              # y rows overlap
        "alsep_nn_vec_div": lambda: lib.alsep_nn_vec_div(h, p, p, 2, 0),
        "alsep_nn_reflect_pad": lambda: lib.alsep_nn_reflect_pad(h, p, p, 2, 6, 6, 0),                         # left = n
        "alsep_nn_tconv_fold": lambda: lib.alsep_nn_tconv_fold(h, p, None, p, 1, 3, 1, 2, 2, 1, 8, 0),         # Lout + pad > (I + 1) S
        "alsep_nn_swap_last2": lambda: lib.alsep_nn_swap_last2(h, p, p, 2, 3, 0),
        "alsep_nn_rmsnorm": lambda: lib.alsep_nn_rmsnorm(h, p, p, p, 2, 8, 7, 8),
        "alsep_nn_rotary": lambda: lib.alsep_nn_rotary(h, p, 4, 16, 0, 2, 5, 1, 4),                            # odd d
        "alsep_nn_gate": lambda: lib.alsep_nn_gate(h, p, p, 4, 2, 0),
        "alsep_nn_mul": lambda: lib.alsep_nn_mul(h, p, p, p, 0),
        "alsep_nn_depth_to_space2": lambda: lib.alsep_nn_depth_to_space2(h, p, p, 2, 2, 3, 4, 2),              # slice past the last channel
    }
    for name, call in calls.items():
        with pytest.raises(AlsepError, match=name):
            dev.check(call(), name)
    dev.synchronize()
    assert float(t.abs().max()) == 0.0
