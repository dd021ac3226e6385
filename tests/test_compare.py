"""audiolab_amd.compare (csrc/compare.h, ``alsep_resample_fft_f64``) on the emulated kernels (-m "not gpu") and on the GPU (-m gpu), same
bodies, against tests/compare_oracle.py -- scipy.signal.resample and scipy.signal.stft themselves -- every element.

Tolerances.  Linear arrays (waveforms, differences, S1, |S1 - S2|): max|ours - want| <= 1e-12 max|want|.  The float64 chain rounds by about
1e-16 log2(n) O(10) < 1e-14 at these sizes, a hundredfold margin; a single-precision stage (6e-8) cannot pass, on purpose.  Decibel arrays:
|ours - want| <= 8.686e-12 M / (v + 1e-9) + 2e-5 per element, v the oracle's linear value and M = max S1: the linear bound carried through
20 log10 (d dB = 8.686 dv / (v + 1e-9)) plus the float32 rounding of a value of up to 180 (half an ulp is 7.6e-6).  No element is masked.

The reductions are selections, so they are compared bit for bit with numpy applied to our own full arrays."""
import struct

import numpy as np
import pytest
import torch

from tests import compare_oracle as co
from tests.conftest import host, on

_ORACLE = {}
_OURS = {}


def signal(n: int, seed: int) -> np.ndarray:
    """0.1 N(0, 1) noise plus two sines, float64"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 44100.0
    return 0.1 * rng.standard_normal(n) + 0.3 * np.sin(2 * np.pi * 440.0 * t) + 0.2 * np.sin(2 * np.pi * 3613.7 * t + 1.0)


# name -> ((samples, rate), (samples, rate))
CASES = {
    "mono 2048": ((2048, 44100), (2048, 44100)),                             # 3 frames, the minimum
    "mono 2049": ((2049, 44100), (2049, 44100)),                             # the padded tail adds a frame
    "mono 5000": ((5000, 44100), (5000, 44100)),
    "stereo, lengths differ": ((2 * 2600, 44100), (2 * 2400, 44100)),        # interleaved; cut to 4800
    "48 k down": ((9600, 48000), (9601, 48000)),                             # both -> 8820: even length going down, Bluestein both sides
    "40 k up": ((8000, 40000), (8001, 40000)),                               # 8820 (Nyquist halved) and 8821
    "88.2 k, powers of two": ((8192, 88200), (4096, 44100)),                 # 8192 -> 4096 on the plain Stockham path
}


def tracks(name):
    (na, ra), (nb, rb) = CASES[name]
    seed = sorted(CASES).index(name)
    return (signal(na, 2 * seed + 1), ra), (signal(nb, 2 * seed + 2), rb)


def oracle(name):
    """computed once per case, shared, read-only"""
    if name not in _ORACLE:
        _ORACLE[name] = co.compare(*tracks(name))
    return _ORACLE[name]


def ours(dev, name, frames_per_batch=0):
    from audiolab_amd import compare
    key = (dev.device.type, name, frames_per_batch)
    if key not in _OURS:
        a, b = tracks(name)
        _OURS[key] = compare.compare_arrays((on(dev, a[0]), a[1]), (on(dev, b[0]), b[1]), ctx=dev, frames_per_batch=frames_per_batch, want_linear=True)
    _OURS[key].ctx = dev                                                     # the emulation's context lives for one test; the tensors stay
    return _OURS[key]


def check_linear(got, want, label):
    got = host(got)
    assert got.dtype == np.float64 and got.shape == want.shape, label
    err, peak = float(np.max(np.abs(got - want))), float(np.max(np.abs(want)))
    print(f"{label}: max|ours - want| = {err:.3e} (bound {1e-12 * peak:.3e})")
    assert np.all(np.isfinite(got)) and err <= 1e-12 * peak, label


def check_db(got, want_db, want_lin, peak_s1, label):
    got = host(got)
    assert got.dtype == np.float32 and got.shape == want_db.shape, label
    bound = 8.686e-12 * peak_s1 / (want_lin + 1e-9) + 2e-5
    excess = np.abs(got.astype(np.float64) - want_db) - bound
    print(f"{label}: max|ours - want| = {np.max(np.abs(got - want_db)):.3e} dB, worst margin to the bound {np.max(excess):.3e}")
    assert np.all(np.isfinite(got)) and np.all(excess <= 0.0), label


def check_case(res, want, label):
    n = len(want["differences"])
    assert tuple(res.differences.shape) == (n,) and res.spec1_db.shape[1] == 1 + -(-n // 1024) == want["spec1"].shape[1]
    check_linear(res.waveforms[0], want["waveforms"][0], f"{label}: track 1")
    check_linear(res.waveforms[1], want["waveforms"][1], f"{label}: track 2")
    check_linear(res.differences, want["differences"], f"{label}: differences")
    check_linear(res.spec1, want["spec1"], f"{label}: S1")
    check_linear(res.spec_diff, want["spec_diff"], f"{label}: |S1 - S2|")
    peak = float(np.max(want["spec1"]))
    check_db(res.spec1_db, want["spec1_db"], want["spec1"], peak, f"{label}: spec1_db")
    check_db(res.diff_db, want["diff_db"], want["spec_diff"], peak, f"{label}: diff_db")
    assert np.allclose(res.t, want["t"], rtol=0, atol=1e-12) and np.allclose(res.f, want["f"], rtol=0, atol=1e-9)


@pytest.mark.parametrize("name", list(CASES))
def test_against_scipy_every_element(dev, name):
    check_case(ours(dev, name), oracle(name), f"{name} [{dev.device.type}]")


def test_two_frames_per_launch(dev):
    """F = 6 frames in three launches: against the oracle, and not a bit away from the single launch"""
    res = ours(dev, "mono 5000", frames_per_batch=2)
    check_case(res, oracle("mono 5000"), f"mono 5000, 2 frames per launch [{dev.device.type}]")
    whole = ours(dev, "mono 5000")
    for a, b in ((res.spec1_db, whole.spec1_db), (res.diff_db, whole.diff_db), (res.spec1, whole.spec1), (res.spec_diff, whole.spec_diff)):
        assert np.array_equal(host(a), host(b))


def test_the_same_track_twice(dev):
    from audiolab_amd import compare
    x = signal(3000, 40)
    res = compare.compare_arrays((on(dev, x), 44100), (on(dev, x.copy()), 44100), ctx=dev, want_linear=True)
    want = co.compare((x, 44100), (x, 44100))
    assert not np.any(host(res.differences)) and not np.any(want["differences"])
    assert not np.any(want["spec_diff"])
    check_db(res.diff_db, want["diff_db"], want["spec_diff"], float(np.max(want["spec1"])), f"same track twice: diff_db [{dev.device.type}]")
    assert np.all(want["diff_db"] == -180.0)
    check_db(res.spec1_db, want["spec1_db"], want["spec1"], float(np.max(want["spec1"])), f"same track twice: spec1_db [{dev.device.type}]")


def test_a_silent_track_is_left_as_it_is(dev):
    from audiolab_amd import compare
    x, z = signal(2500, 41), np.zeros(2500)
    for pair in (((z, 44100), (x, 44100)), ((x, 44100), (z, 44100))):
        res = compare.compare_arrays((on(dev, pair[0][0]), 44100), (on(dev, pair[1][0]), 44100), ctx=dev, want_linear=True)
        want = co.compare(*pair)
        silent = 0 if pair[0][0] is z else 1
        assert not np.any(host(res.waveforms[silent]))
        for arr in (res.waveforms[0], res.waveforms[1], res.differences, res.spec1_db, res.diff_db, res.spec1, res.spec_diff):
            assert np.all(np.isfinite(host(arr)))
        check_linear(res.waveforms[1 - silent], want["waveforms"][1 - silent], "the other track")
        check_linear(res.differences, want["differences"], "differences beside silence")
        peak = float(np.max(want["spec1"]))
        check_db(res.spec1_db, want["spec1_db"], want["spec1"], peak, "spec1_db beside silence")
        check_db(res.diff_db, want["diff_db"], want["spec_diff"], peak, "diff_db beside silence")


KERNELS = ("cmp_sumsq_partial_kernel", "cmp_wave_kernel", "cmp_spectra_kernel", "pack_rows_kernel")


def test_too_short_for_a_frame(dev):
    from audiolab_amd import _lib, compare
    before = [dev.launch_count(k) for k in KERNELS]
    x = signal(2047, 42)
    with pytest.raises(ValueError):
        compare.compare_arrays((on(dev, x), 44100), (on(dev, signal(5000, 43)), 44100), ctx=dev)
    with pytest.raises(ValueError):                                          # 2229 samples at 48 kHz are 2047 at 44.1 kHz
        compare.compare_arrays((on(dev, signal(2229, 44)), 48000), (on(dev, signal(5000, 43)), 44100), ctx=dev)
    assert [dev.launch_count(k) for k in KERNELS] == before                  # nothing was launched
    # the entry point itself: refused, no output buffer touched
    lib = dev.lib
    assert lib.alsep_compare_frames(2047) == -1 and lib.alsep_compare_frames(2048) == 3 and lib.alsep_compare_frames(2049) == 4
    d = on(dev, x)
    tab = on(dev, np.zeros(4096))
    db = [torch.full((1025, 3), 7.0, dtype=torch.float32, device=dev.device) for _ in range(2)]
    lin = [torch.full((1025, 3), 7.0, dtype=torch.float64, device=dev.device) for _ in range(2)]
    rc = lib.alsep_compare_spectra(dev.handle, _lib.ptr(d), _lib.ptr(d), 2047, _lib.ptr(tab), _lib.ptr(tab), 0, _lib.ptr(db[0]), _lib.ptr(db[1]),
                                   _lib.ptr(lin[0]), _lib.ptr(lin[1]))
    assert rc == -1
    for buf in db + lin:
        assert np.all(host(buf) == 7.0)
    assert [dev.launch_count(k) for k in KERNELS] == before


def test_too_long_for_the_transform(dev):
    """2^26 + 1 samples at 48 kHz: Bluestein needs 2^28 points.  Refused before the samples are looked at (the zeros are never touched)"""
    from audiolab_amd import compare
    from audiolab_amd._lib import AlsepError
    before = [dev.launch_count(k) for k in KERNELS]
    z = torch.from_numpy(np.zeros((1 << 26) + 1))
    with pytest.raises(AlsepError, match="2\\^27"):
        compare.compare_arrays((z, 48000), (z, 48000), ctx=dev)
    assert [dev.launch_count(k) for k in KERNELS] == before


def test_sum_of_squares_is_reproducible(dev):
    from audiolab_amd import _lib
    lib = dev.lib
    need = int(lib.alsep_compare_rms_workspace_bytes())
    ws = torch.empty((need,), dtype=torch.uint8, device=dev.device)
    for n in (1, 255, 5000, 300001):                                         # one block, a ragged one, several, more blocks than partials
        x = signal(n, 50 + n % 7)
        d = on(dev, x)
        out = torch.zeros((2,), dtype=torch.float64, device=dev.device)
        for i in range(2):
            assert lib.alsep_compare_rms(dev.handle, _lib.ptr(d), n, _lib.ptr(out) + 8 * i, _lib.ptr(ws), need) == 0
        got = host(out)
        assert got.view(np.uint64)[0] == got.view(np.uint64)[1]
        want = float(np.sum(x ** 2))
        print(f"n = {n}: sum of squares {got[0]!r}, numpy {want!r}")
        assert abs(got[0] - want) <= 1e-12 * want
    assert lib.alsep_compare_rms(dev.handle, _lib.ptr(d), 0, _lib.ptr(out), _lib.ptr(ws), need) == -1
    assert lib.alsep_compare_rms(dev.handle, _lib.ptr(d), 5, _lib.ptr(out), _lib.ptr(ws), need - 1) == -1


def _numpy_minmax(x, k):
    n = len(x)
    edges = [(j * n // k, (j + 1) * n // k) for j in range(k)]
    mn = np.array([x[a:b].min() for a, b in edges])
    mx = np.array([x[a:b].max() for a, b in edges])
    imn = np.array([a + int(np.argmin(x[a:b])) for a, b in edges])
    imx = np.array([a + int(np.argmax(x[a:b])) for a, b in edges])
    return mn, imn, mx, imx


@pytest.mark.parametrize("columns", [8, 50, 7, 613, 4800, 9000])            # 4800 = 8 * 600 = 50 * 96; 7 and 613 do not divide it; K = n; K > n
def test_minmax_is_numpy_on_our_own_array(dev, columns):
    res = ours(dev, "stereo, lengths differ")
    for curve in (res.waveforms[0], res.differences):
        x = host(curve)
        k = min(columns, len(x))
        got = [host(v) for v in res.minmax(curve, columns)]
        want = _numpy_minmax(x, k)
        assert got[0].shape == (k,) and got[1].dtype == np.int64
        for g, w in zip(got, want):
            assert np.array_equal(g, w)
        assert np.array_equal(x[got[1]], got[0]) and np.array_equal(x[got[3]], got[2])


def test_minmax_takes_the_first_index_on_ties(dev):
    res = ours(dev, "mono 2048")
    x = signal(1000, 60)
    x[100:400] = x.max() + 1.0                                               # a constant stretch over several buckets: the maximum
    x[600:900] = x.min() - 1.0                                               # and the minimum
    x[950:] = 0.25
    for k in (1, 10, 33, 1000):
        got = [host(v) for v in res.minmax(on(dev, x), k)]
        for g, w in zip(got, _numpy_minmax(x, k)):
            assert np.array_equal(g, w), k
    from audiolab_amd import _lib
    d = on(dev, x)
    o = [torch.zeros((4,), dtype=dt, device=dev.device) for dt in (torch.float64, torch.int64, torch.float64, torch.int64)]
    for n, k in ((1000, 0), (1000, 1001), (0, 1)):
        assert dev.lib.alsep_compare_minmax(dev.handle, _lib.ptr(d), n, k, *[_lib.ptr(v) for v in o]) == -1


@pytest.mark.parametrize("columns", [1, 2, 3, 4, 6, 100])                   # F = 6: dividing it, not dividing it, Kt = F, capped at F
def test_bucket_maxima_are_numpy_on_our_own_arrays(dev, columns):
    res = ours(dev, "mono 5000")
    frames = int(res.spec1_db.shape[1])
    assert frames == 6
    kt = min(columns, frames)
    t, s1, sd = res.spectra_reduced(columns)
    first = [j * frames // kt for j in range(kt)]
    assert np.array_equal(t, res.t[first])
    for got, full in ((s1, host(res.spec1_db)), (sd, host(res.diff_db))):
        want = np.stack([full[:, j * frames // kt:(j + 1) * frames // kt].max(axis=1) for j in range(kt)], axis=1)
        assert host(got).dtype == np.float32 and np.array_equal(host(got), want)
    if kt == frames:
        assert np.array_equal(host(s1), host(res.spec1_db))


def test_bucket_maxima_with_ties(dev):
    from audiolab_amd import _lib
    rng = np.random.default_rng(61)
    full = rng.integers(-3, 3, size=(1025, 37)).astype(np.float32)           # few distinct values: ties everywhere
    d = on(dev, full)
    for kt in (5, 37):
        out = torch.zeros((1025, kt), dtype=torch.float32, device=dev.device)
        assert dev.lib.alsep_compare_colmax(dev.handle, _lib.ptr(d), 37, kt, _lib.ptr(out)) == 0
        want = np.stack([full[:, j * 37 // kt:(j + 1) * 37 // kt].max(axis=1) for j in range(kt)], axis=1)
        assert np.array_equal(host(out), want)
    out = torch.zeros((1025, 38), dtype=torch.float32, device=dev.device)
    assert dev.lib.alsep_compare_colmax(dev.handle, _lib.ptr(d), 37, 38, _lib.ptr(out)) == -1
    assert dev.lib.alsep_compare_colmax(dev.handle, _lib.ptr(d), 37, 0, _lib.ptr(out)) == -1


def test_envelopes_are_real_samples_in_index_order(dev):
    res = ours(dev, "mono 5000")
    curves = res.envelopes(64)
    assert len(curves) == 3
    for (x, y), full in zip(curves, (res.waveforms[0], res.waveforms[1], res.differences)):
        full = host(full)
        assert x.shape == y.shape == (128,) and np.all(np.diff(x) >= 0)
        assert np.array_equal(full[x], y)
        mn, imn, mx, imx = _numpy_minmax(full, 64)
        assert np.array_equal(np.minimum(y[0::2], y[1::2]), mn) and np.array_equal(np.maximum(y[0::2], y[1::2]), mx)
        assert np.array_equal(np.minimum(x[0::2], x[1::2]), np.minimum(imn, imx))


def test_resample_f64_entry_point(dev):
    """float64 rows in pairs, as the float32 entry point takes them; against scipy.signal.resample"""
    from scipy.signal import resample
    from audiolab_amd import _lib
    lib = dev.lib
    rng = np.random.default_rng(62)
    for rows, n_in, n_out in ((1, 601, 450), (3, 512, 700), (2, 700, 700)):
        x = rng.standard_normal((rows, n_in))
        d, y = on(dev, x), torch.zeros((rows, n_out), dtype=torch.float64, device=dev.device)
        need = int(lib.alsep_resample_fft_f64_workspace_bytes(n_in, n_out))
        assert need == lib.alsep_resample_fft_workspace_bytes(n_in, n_out) > 0
        ws = torch.empty((need,), dtype=torch.uint8, device=dev.device)
        assert lib.alsep_resample_fft_f64(dev.handle, _lib.ptr(d), n_in, _lib.ptr(y), n_out, rows, n_in, n_out, _lib.ptr(ws), need) == 0
        check_linear(y, resample(x, n_out, axis=1), f"{rows} rows {n_in} -> {n_out}")
        assert lib.alsep_resample_fft_f64(dev.handle, _lib.ptr(d), n_in, _lib.ptr(y), n_out, rows, n_in, n_out, _lib.ptr(ws), need - 1) == -1
    assert lib.alsep_resample_fft_f64_workspace_bytes(0, 5) == -1


def _wav(path, tag, channels, rate, bits, payload):
    block = channels * bits // 8
    fmt = struct.pack("<HHIIHH", tag, channels, rate, rate * block, block, bits)
    body = b"fmt " + struct.pack("<I", len(fmt)) + fmt + b"data" + struct.pack("<I", len(payload)) + payload + (b"\x00" if len(payload) & 1 else b"")
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 4 + len(body)) + b"WAVE" + body)


def test_the_interleaved_reader(tmp_path):
    """v / 2^(bits - 1), exact in float64, in file order; float samples as they are"""
    from audiolab_amd import wavio
    rng = np.random.default_rng(63)
    p = str(tmp_path / "x.wav")
    v16 = rng.integers(-32768, 32768, size=(7, 2)).astype("<i2")
    _wav(p, 1, 2, 48000, 16, v16.tobytes())
    x, rate = wavio.read_wav_interleaved(p)
    assert rate == 48000 and x.dtype == np.float64 and np.array_equal(x, v16.reshape(-1) / 32768.0)
    v32 = rng.integers(-2 ** 31, 2 ** 31, size=9).astype("<i4")
    _wav(p, 1, 1, 44100, 32, v32.tobytes())
    assert np.array_equal(wavio.read_wav_interleaved(p)[0], v32 / 2147483648.0)
    v24 = np.array([-8388608, -1, 0, 1, 8388607, 123456, -654321, 77], dtype=np.int64)
    _wav(p, 1, 2, 44100, 24, b"".join(int(v & 0xFFFFFF).to_bytes(3, "little") for v in v24))
    assert np.array_equal(wavio.read_wav_interleaved(p)[0], v24 / 8388608.0)
    v8 = np.array([0, 1, 127, 128, 129, 255], dtype=np.uint8)
    _wav(p, 1, 2, 8000, 8, v8.tobytes())
    assert np.array_equal(wavio.read_wav_interleaved(p)[0], (v8.astype(np.float64) - 128.0) / 128.0)
    f32 = rng.standard_normal(10).astype("<f4") * 3.0                        # beyond full scale: kept
    _wav(p, 3, 2, 44100, 32, f32.tobytes())
    assert np.array_equal(wavio.read_wav_interleaved(p)[0], f32.astype(np.float64))
    f64 = rng.standard_normal(6)
    _wav(p, 3, 1, 44100, 64, f64.astype("<f8").tobytes())
    assert np.array_equal(wavio.read_wav_interleaved(p)[0], f64)
    _wav(p, 1, 1, 44100, 12, b"\x00" * 6)
    with pytest.raises(ValueError):
        wavio.read_wav_interleaved(p)


def test_paths_are_read_as_fractions_of_full_scale(dev, tmp_path):
    """a 16-bit stereo file at 48 kHz beside a float file at 44.1 kHz, by path: the same as the arrays"""
    from audiolab_amd import compare, wavio
    a = np.clip(0.5 * signal(2 * 2400, 64), -1, 1).reshape(-1, 2).T                                   # [2, 2400]
    b = 0.5 * signal(4500, 65)
    pa, pb = str(tmp_path / "a.wav"), str(tmp_path / "b.wav")
    wavio.write_wav(pa, a, 48000, subtype="PCM_16")
    wavio.write_wav(pb, b.astype(np.float32), 44100, subtype="FLOAT")
    res = compare.compare_arrays(pa, pb, ctx=dev, want_linear=True)
    a16 = np.clip(np.rint(a.T.reshape(-1) * 32768.0), -32768, 32767) / 32768.0
    want = co.compare((a16, 48000), (b.astype(np.float32).astype(np.float64), 44100))
    assert len(want["differences"]) == 4410
    check_case(res, want, f"by path [{dev.device.type}]")
