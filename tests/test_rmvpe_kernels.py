"""The kernels of csrc/rmvpe.h one at a time, each body on the CPU emulation and on the GPU through ``dev``: the GRU recurrence against
torch.nn.GRU, the stride-2 transposed convolution against F.conv_transpose2d, the average pool against F.avg_pool2d, the log-mel front end
and the decode against tests/rmvpe_oracle.py, the frame padding against F.pad.

Bounds.  GRU: max |h - h_ref| < 1e-5 (float32 recurrence, |h| < 1).  Transposed convolution: 1e-5 of the output's peak (at most 4 x 16
float32 products of O(1) values per output).  Average pool: 1e-6 absolute on O(1) values (three float32 additions).  Mel: 1e-5 of the peak
before the log; after the log the same relative bound, 2e-5 absolute to leave room for the float32 logarithm, where the oracle's mel is
above 1e-4 (below it the clamp at 1e-5 magnifies float32 noise).  Decode: 1e-12 relative, zeros exact."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from audiolab_amd import rmvpe
from audiolab_amd._lib import AlsepError
from tests import rmvpe_oracle as o
from tests.conftest import host, on


# ---- GRU ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,N,H", [(1, 1, 16), (3, 1, 16), (37, 2, 256)])
def test_gru_matches_torch(dev, T, N, H):
    torch.manual_seed(T * 1000 + H)
    ref = torch.nn.GRU(H, H, num_layers=1, bidirectional=True).eval()
    with torch.no_grad():
        for name, prm in ref.named_parameters():
            if "bias_hh" in name:
                prm.copy_(torch.rand_like(prm) - 0.5)                         # clearly non-zero b_hh: b_hn sits inside the reset product
        x = torch.randn(T, N, H)
        want = ref(x)[0].numpy()
        sd = dict(ref.named_parameters())
        wih = torch.cat([sd["weight_ih_l0"], sd["weight_ih_l0_reverse"]]).double()
        bih = torch.cat([sd["bias_ih_l0"], sd["bias_ih_l0_reverse"]]).double()
        pre = (x.double().reshape(T * N, H) @ wih.t() + bih).float().reshape(T, N, 6 * H).contiguous()
        whh_t = torch.stack([sd["weight_hh_l0"].t(), sd["weight_hh_l0_reverse"].t()]).contiguous()
        bhh = torch.stack([sd["bias_hh_l0"], sd["bias_hh_l0_reverse"]]).contiguous()
    got = host(rmvpe.gru(dev, on(dev, pre), on(dev, whh_t.detach()), on(dev, bhh.detach())))
    err = float(np.max(np.abs(got - want)))
    print(f"gru T={T} N={N} H={H}: max |delta| = {err:.3e}")
    assert got.shape == (T, N, 2 * H)
    assert err < 1e-5


def test_gru_refuses_bad_sizes(dev):
    with pytest.raises(AlsepError):
        rmvpe.gru(dev, dev.zeros((2, 1, 6 * 24)), dev.zeros((2, 24, 72)), dev.zeros((2, 72)))     # H % 16 != 0


# ---- transposed convolution ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,Cin,Cout", [(1, 2, 8, 4), (3, 4, 16, 8)])
def test_tconv_into_a_slice(dev, H, W, Cin, Cout):
    g = torch.Generator().manual_seed(H * 100 + Cin)
    x = torch.randn(1, Cin, H, W, generator=g)
    w = torch.randn(Cin, Cout, 3, 3, generator=g) / np.sqrt(Cin)
    scale, shift = torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g) * 0.1
    want = F.relu(F.conv_transpose2d(x, w, stride=2, padding=1, output_padding=1) * scale[None, :, None, None] + shift[None, :, None, None])
    want = want.permute(0, 2, 3, 1).numpy()
    total, off = Cout + 6, 2                                                  # a wider tensor: channels outside the slice must not change
    y = torch.full((1, 2 * H, 2 * W, total), 7.0)
    y_d = on(dev, y)
    rmvpe.tconv3x3s2(dev, on(dev, x.permute(0, 2, 3, 1).contiguous()), on(dev, w.permute(2, 3, 0, 1).contiguous()), on(dev, scale), on(dev, shift),
                     y_d, off, 1)
    got = host(y_d)
    err = float(np.max(np.abs(got[..., off:off + Cout] - want))) / float(np.max(np.abs(want)))
    print(f"tconv {H}x{W} {Cin}->{Cout}: max |delta| / peak = {err:.3e}")
    assert err < 1e-5
    assert np.all(got[..., :off] == 7.0) and np.all(got[..., off + Cout:] == 7.0)


def test_tconv_refuses_channels_not_in_fours(dev):
    with pytest.raises(AlsepError):
        rmvpe.tconv3x3s2(dev, dev.zeros((1, 2, 2, 4)), dev.zeros((3, 3, 4, 6)), dev.zeros((6,)), dev.zeros((6,)), dev.zeros((1, 4, 4, 6)))


# ---- average pool ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,C", [(2, 4, 3), (6, 128, 16)])
def test_avgpool(dev, H, W, C):
    g = torch.Generator().manual_seed(H + C)
    x = torch.randn(1, H, W, C, generator=g)
    want = F.avg_pool2d(x.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1).numpy()
    cat = torch.full((1, H, W, 2 * C + 1), -3.0)
    cat_d = on(dev, cat)
    got = host(rmvpe.avgpool2(dev, on(dev, x), cat_d, C))
    assert got.shape == want.shape
    assert float(np.max(np.abs(got - want))) < 1e-6
    c = host(cat_d)
    assert np.array_equal(c[..., C:2 * C], x.numpy())                         # the skip, copied in the same pass
    assert np.all(c[..., :C] == -3.0) and np.all(c[..., 2 * C:] == -3.0)
    assert float(np.max(np.abs(host(rmvpe.avgpool2(dev, on(dev, x))) - want))) < 1e-6


def test_avgpool_refuses_odd_sizes(dev):
    with pytest.raises(AlsepError):
        rmvpe.avgpool2(dev, dev.zeros((1, 3, 4, 2)))


# ---- log-mel front end -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [160, 5280, 16000])
def test_mel_frontend(dev, n):
    audio = o.test_signal(n, seed=n)
    want_lin = o.mel_linear(audio).T                                          # [T, 128]
    logm, lin = rmvpe.mel_frontend(dev, on(dev, audio), want_linear=True)
    got_lin, got_log = host(lin), host(logm)
    assert got_lin.shape == (n // 160 + 1, 128)
    peak = float(np.max(np.abs(want_lin)))
    err = float(np.max(np.abs(got_lin - want_lin))) / peak
    print(f"mel n={n}: max |delta| / peak = {err:.3e} (peak {peak:.3e})")
    assert err < 1e-5
    want_log = np.log(np.maximum(want_lin, np.float32(1e-5)))
    sel = want_lin > 1e-4
    assert sel.any()
    # d log = d lin / lin <= 1e-5 peak / lin on the compared entries, plus the float32 logarithm's own rounding
    bound = 1e-5 * peak / want_lin[sel] + 2e-5
    assert np.all(np.abs(got_log[sel] - want_log[sel]) <= bound)
    assert np.all(got_log >= np.float32(np.log(np.float32(1e-5))))            # the clamp


def test_mel_matches_the_reference(dev, golden_dir):
    z = np.load(f"{golden_dir}/rmvpe.npz")
    got = host(rmvpe.mel_frontend(dev, on(dev, z["audio"]))).T
    lin = np.exp(z["mel"].astype(np.float64))                                 # the reference returns the log only
    sel = lin > 1e-4
    assert np.all(np.abs(got[sel] - z["mel"][sel]) <= 1e-5 * lin.max() / lin[sel] + 2e-5)


def test_mel_refuses_an_empty_track(dev):
    with pytest.raises(AlsepError, match="0 samples"):
        rmvpe.mel_frontend(dev, dev.zeros((0,)))


# ---- decode ---------------------------------------------------------------------------------------------------------------------------------
def _constructed_salience():
    rng = np.random.default_rng(5)
    rows = []
    for peak in (0, 3, 356, 359, 100):
        r = (0.2 * rng.random(360)).astype(np.float32)
        r[peak] = 0.9
        if peak == 100:
            r[101] = 0.6
        rows.append(r)
    tie = (0.2 * rng.random(360)).astype(np.float32)
    tie[[50, 200]] = 0.75                                                     # an exact tie: bin 50 wins
    at_thred = np.zeros(360, dtype=np.float32)
    at_thred[120], at_thred[121] = np.float32(0.03), np.float32(0.02)         # the largest salience exactly at thred: unvoiced
    above = at_thred.copy()
    above[120] = np.nextafter(np.float32(0.03), np.float32(1))
    return np.stack(rows + [tie, at_thred, above, np.zeros(360, dtype=np.float32)])


def test_decode_constructed(dev):
    sal = _constructed_salience()
    want = o.decode(sal, 0.03)
    got = host(rmvpe.decode_salience(dev, on(dev, sal), 0.03))
    assert got.dtype == np.float64 and got.shape == want.shape
    assert np.array_equal(got == 0, want == 0)
    assert list(want == 0) == [False] * 6 + [True, False, True]
    nz = want != 0
    rel = np.abs(got[nz] - want[nz]) / want[nz]
    print("decode: max relative delta", float(rel.max()))
    assert float(rel.max()) < 1e-12
    # the tie resolves to the lower bin: its f0 lies near bin 50's, not bin 200's
    assert abs(1200 * np.log2(got[5] / 10) - (20 * 50 + 1997.3794084376191)) < 60


def test_decode_matches_the_reference(dev, golden_dir):
    z = np.load(f"{golden_dir}/rmvpe.npz")
    for tag in ("reduced", "full"):
        got = host(rmvpe.decode_salience(dev, on(dev, z[f"hidden_{tag}"]), 0.03))
        want = z[f"f0_{tag}"]
        assert np.array_equal(got == 0, want == 0)
        assert float(np.max(np.abs(got - want) / np.maximum(want, 1e-300))) < 1e-12


# ---- frame padding -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [33, 63, 64, 65])
def test_frame_padding(dev, T):
    pad = rmvpe.pad_frames_of(T)
    assert pad == o.padded_frames(T) and (T + pad) % 32 == 0
    x = torch.randn(T, 128, generator=torch.Generator().manual_seed(T))
    want = F.pad(x.t()[None], (0, pad), mode="reflect")[0].t().numpy() * np.float32(0.5) + np.float32(0.25)
    got = host(rmvpe.pad_frames(dev, on(dev, x), T + pad, 0.5, 0.25))
    assert got.shape == (T + pad, 128)
    assert float(np.max(np.abs(got - want))) < 1e-6
    assert np.array_equal(host(rmvpe.pad_frames(dev, on(dev, x), T + pad)), F.pad(x.t()[None], (0, pad), mode="reflect")[0].t().numpy())


def test_frame_padding_refused_where_reflection_is_impossible():
    with pytest.raises(AlsepError, match="16 frames need 16 reflected"):
        rmvpe.pad_frames_of(16)
    assert rmvpe.pad_frames_of(17) == 15


def test_pad_frames_kernel_refuses_too_much(dev):
    with pytest.raises(AlsepError, match="cannot be reflected"):
        rmvpe.pad_frames(dev, dev.zeros((16, 128)), 32)
