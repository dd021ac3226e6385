"""Direct tests of the layout kernels between the FFT and the networks (csrc/nn.hip): HTDemucs / HDemucs spectrogram in and out and the final
mix, the Roformer band gather and mask, the MDX23C sub-band packing.  Each kernel decomposes a flat index into 4 to 6 coordinates; the
shapes here have pairwise different extents and non-zero offsets, so that two swapped extents or a dropped offset change the result.  Every
reference is a few lines of indexing taken from the comment above the kernel, in float64 on the CPU.  Pure data movement is bit-exact,
the kernels with arithmetic are held to 1e-6 * max(1, max|want|)."""
import numpy as np
import pytest
import torch

from audiolab_amd import _lib
from audiolab_amd._lib import AlsepError
from tests.conftest import host, on

SENT = 7.25
EW = 1e-6


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _out(dev, n, tail=5):
    return on(dev, torch.full((n + tail,), SENT))


def _close(got, want, what):
    want = want.detach().numpy() if isinstance(want, torch.Tensor) else np.asarray(want)
    got = np.asarray(got, dtype=np.float64).reshape(want.shape)
    err, bound = float(np.max(np.abs(got - want))), EW * max(1.0, float(np.max(np.abs(want))))
    assert np.all(np.isfinite(got)) and err < bound, f"{what}: max|delta| {err:.3e} >= {bound:.3e}"


# ------------------------------------------------------------------------------------------ Demucs
@pytest.mark.parametrize("t_off,scale", [(3, 1.0), (5, 0.37), (0, 1.0)])
def test_demucs_spec_in(dev, t_off, scale):
    B, Fq, Tt, T = 2, 13, 14, 9
    spec = torch.randn(B, 4, Fq, Tt, generator=_gen(t_off)) + 0.3
    want = scale * spec.double()[..., t_off:t_off + T].permute(0, 2, 3, 1)                   # [B, F, T, 4]
    sd, y = on(dev, spec.clone()), _out(dev, want.numel())
    dev.check(dev.lib.alsep_demucs_spec_in(dev.handle, _lib.ptr(sd), _lib.ptr(y), B, Fq, Tt, T, t_off, scale), "alsep_demucs_spec_in")
    got = host(y)
    assert np.all(got[want.numel():] == SENT)
    if scale == 1.0:
        assert np.array_equal(got[:want.numel()].reshape(want.shape), want.float().numpy())
    else:
        _close(got[:want.numel()], want, "alsep_demucs_spec_in")


@pytest.mark.parametrize("t_off", [3, 0, 5])
def test_demucs_spec_out(dev, t_off):
    """frames [t_off, t_off + T) = scale * (x * std + mean) per batch item, every other frame exactly zero"""
    B, S, Fq, Tt, T, scale = 2, 3, 13, 14, 9, 1.7
    g = _gen(t_off + 20)
    x = torch.randn(B, Fq, T, S * 4, generator=g) + 0.3
    stats = torch.tensor([[0.4, 1.3], [-0.7, 0.6]])                                          # (mean, std) of each item
    v = x.double().reshape(B, Fq, T, S, 4).permute(0, 3, 4, 1, 2)                            # [B, S, 4, F, T]
    want = torch.zeros(B, S, 4, Fq, Tt, dtype=torch.float64)
    want[..., t_off:t_off + T] = scale * (v * stats.double()[:, 1].reshape(B, 1, 1, 1, 1) + stats.double()[:, 0].reshape(B, 1, 1, 1, 1))
    xd, sd, y = on(dev, x.clone()), on(dev, stats.clone()), _out(dev, want.numel())
    dev.check(dev.lib.alsep_demucs_spec_out(dev.handle, _lib.ptr(xd), _lib.ptr(sd), _lib.ptr(y), B, S, Fq, Tt, T, t_off, scale),
              "alsep_demucs_spec_out")
    got = host(y)
    assert np.all(got[want.numel():] == SENT)
    got = got[:want.numel()].reshape(want.shape)
    assert np.all(got[..., :t_off] == 0.0) and np.all(got[..., t_off + T:] == 0.0)
    _close(got, want, "alsep_demucs_spec_out")


def test_demucs_mix_out(dev):
    """out [B, S, 2, L] = (xt [B, L, S * 2] * std + mean) + xs [B * S, 2, L]"""
    B, S, L = 2, 3, 11
    g = _gen(30)
    xt, xs = torch.randn(B, L, S * 2, generator=g) + 0.3, torch.randn(B * S, 2, L, generator=g) - 0.4
    stats = torch.tensor([[0.2, 1.6], [-0.5, 0.7]])
    t = xt.double().reshape(B, L, S, 2).permute(0, 2, 3, 1)                                  # [B, S, 2, L]
    want = t * stats.double()[:, 1].reshape(B, 1, 1, 1) + stats.double()[:, 0].reshape(B, 1, 1, 1) + xs.double().reshape(B, S, 2, L)
    td, sd, xd, y = on(dev, xt.clone()), on(dev, stats.clone()), on(dev, xs.clone()), _out(dev, want.numel())
    dev.check(dev.lib.alsep_demucs_mix_out(dev.handle, _lib.ptr(td), _lib.ptr(sd), _lib.ptr(xd), _lib.ptr(y), B, S, L), "alsep_demucs_mix_out")
    got = host(y)
    assert np.all(got[want.numel():] == SENT)
    _close(got[:want.numel()], want, "alsep_demucs_mix_out")


# ------------------------------------------------------------------------------------------ Roformer
def test_roformer_gather(dev):
    """feat[t, 2 i + c] = spec[s * 2 + c, f, t] for midx[i] = 2 f + s: bins out of order, some taken twice, some never"""
    Fq, T, n_idx = 13, 9, 17
    g = _gen(40)
    spec = torch.randn(4, Fq, T, generator=g) + 0.3
    midx = torch.randint(0, 2 * Fq, (n_idx,), generator=g, dtype=torch.int32)
    midx[0], midx[1], midx[2] = 2 * Fq - 1, 0, 2 * Fq - 1
    want = np.empty((T, 2 * n_idx), np.float32)
    for i, m in enumerate(midx.tolist()):
        f, s = m >> 1, m & 1
        for c in range(2):
            want[:, 2 * i + c] = spec[s * 2 + c, f].numpy()
    sd, md, y = on(dev, spec.clone()), on(dev, midx.clone()), _out(dev, want.size)
    dev.check(dev.lib.alsep_roformer_gather(dev.handle, _lib.ptr(sd), _lib.ptr(md), _lib.ptr(y), n_idx, Fq, T), "alsep_roformer_gather")
    got = host(y)
    assert np.all(got[want.size:] == SENT) and np.array_equal(got[:want.size].reshape(want.shape), want)


def test_roformer_mask(dev):
    """bins covered by no band (mask 0), by one and by three (the mean of the three GLU outputs); out = spec * mask as complex numbers"""
    Fq, T, H = 6, 9, 23
    g = _gen(50)
    spec, h = torch.randn(4, Fq, T, generator=g) + 0.3, torch.randn(T, H, generator=g) * 1.2 + 0.2
    counts = [(0, 1, 3, 1, 3, 0)[m % 6] for m in range(2 * Fq)]
    counts[1], counts[2] = 3, 0                                                              # ... not in step with the channel either
    occ_start = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32)
    n_occ = int(occ_start[-1])
    col_a = torch.randint(0, H - 1, (n_occ,), generator=g, dtype=torch.int32)
    col_g = torch.randint(0, H - 1, (n_occ,), generator=g, dtype=torch.int32)
    h64, s64 = h.double(), spec.double()
    want = torch.zeros(4, Fq, T, dtype=torch.float64)
    for m in range(2 * Fq):
        f, s = m >> 1, m & 1
        mask = torch.zeros(T, dtype=torch.complex128)
        for o in range(int(occ_start[m]), int(occ_start[m + 1])):
            a, q = int(col_a[o]), int(col_g[o])
            mask += torch.complex(h64[:, a] * torch.sigmoid(h64[:, q]), h64[:, a + 1] * torch.sigmoid(h64[:, q + 1]))
        mask /= max(counts[m], 1)
        z = torch.complex(s64[2 * s, f], s64[2 * s + 1, f]) * mask
        want[2 * s, f], want[2 * s + 1, f] = z.real, z.imag
    sd, hd, od, ad, gd = on(dev, spec.clone()), on(dev, h.clone()), on(dev, occ_start), on(dev, col_a), on(dev, col_g)
    y = _out(dev, want.numel())
    dev.check(dev.lib.alsep_roformer_mask(dev.handle, _lib.ptr(sd), _lib.ptr(hd), _lib.ptr(od), _lib.ptr(ad), _lib.ptr(gd), _lib.ptr(y), Fq, T, H),
              "alsep_roformer_mask")
    got = host(y)
    assert np.all(got[want.numel():] == SENT)
    got = got[:want.numel()].reshape(4, Fq, T)
    for m in range(2 * Fq):
        if counts[m] == 0:
            assert np.all(got[2 * (m & 1):2 * (m & 1) + 2, m >> 1] == 0.0)
    _close(got, want, "alsep_roformer_mask")


# ------------------------------------------------------------------------------------------ MDX23C
def test_mdx23c_spec_in(dev):
    """x[t, ff, c2 * k + kk] = spec[c2, kk * f + ff, t]"""
    f, k, T = 5, 3, 7
    spec = torch.randn(4, f * k, T, generator=_gen(60)) + 0.3
    want = spec.reshape(4, k, f, T).permute(3, 2, 0, 1).reshape(T, f, 4 * k).numpy()
    sd, y = on(dev, spec.clone()), _out(dev, want.size)
    dev.check(dev.lib.alsep_mdx23c_spec_in(dev.handle, _lib.ptr(sd), _lib.ptr(y), f, k, T), "alsep_mdx23c_spec_in")
    got = host(y)
    assert np.all(got[want.size:] == SENT) and np.array_equal(got[:want.size].reshape(want.shape), want)


def test_mdx23c_spec_out(dev):
    """spec[s, c2, kk * f + ff, t] = y[t, ff, (s * 4 + c2) * k + kk]"""
    S, f, k, T = 2, 5, 3, 7
    yv = torch.randn(T, f, S * 4 * k, generator=_gen(61)) + 0.3
    want = yv.reshape(T, f, S, 4, k).permute(2, 3, 4, 1, 0).reshape(S, 4, k * f, T).numpy()
    yd, out = on(dev, yv.clone()), _out(dev, want.size)
    dev.check(dev.lib.alsep_mdx23c_spec_out(dev.handle, _lib.ptr(yd), _lib.ptr(out), S, f, k, T), "alsep_mdx23c_spec_out")
    got = host(out)
    assert np.all(got[want.size:] == SENT) and np.array_equal(got[:want.size].reshape(want.shape), want)


# ------------------------------------------------------------------------------------------ argument guards
def test_bad_arguments_are_rejected(dev):
    lib, h = dev.lib, dev.handle
    t = dev.zeros((256,))
    p = _lib.ptr(t)
    calls = {
        "alsep_demucs_spec_in": lambda: lib.alsep_demucs_spec_in(h, p, p, 1, 3, 5, 4, 2, 1.0),                 # t_off + T > Tt
        "alsep_demucs_spec_out": lambda: lib.alsep_demucs_spec_out(h, p, p, p, 1, 1, 3, 5, 4, 2, 1.0),
        "alsep_demucs_mix_out": lambda: lib.alsep_demucs_mix_out(h, p, p, p, p, 1, 2, 0),
        "alsep_roformer_gather": lambda: lib.alsep_roformer_gather(h, p, p, p, 0, 3, 4),
        "alsep_roformer_mask": lambda: lib.alsep_roformer_mask(h, p, p, p, p, p, p, 3, 4, 0),
        "alsep_mdx23c_spec_in": lambda: lib.alsep_mdx23c_spec_in(h, p, p, 3, 0, 4),
        "alsep_mdx23c_spec_out": lambda: lib.alsep_mdx23c_spec_out(h, p, p, 0, 3, 2, 4),
    }
    for name, call in calls.items():
        with pytest.raises(AlsepError, match=name):
            dev.check(call(), name)
    dev.synchronize()
    assert float(t.abs().max()) == 0.0
