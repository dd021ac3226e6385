"""CPU only.  (1) tests/golden/merge.npz -- written by scripts/make_golden_merge.py with the stdlib C module ``audioop`` -- is reproduced
exactly by the numpy restatements of its four routines in tests/merge_cases.py, so the fixture can be audited where ``audioop`` is absent;
where the module is present, the restatements are also compared with it directly.  (2) audiolab_amd.wavio: the PCM_32 subtype, the integer
write path and ``read_wav_info``."""
import math
import os
import struct

import numpy as np
import pytest

from tests.merge_cases import NUMPY_OPS, VARIANTS, fixture_of, make_case, np_add, np_max, np_mul, np_rms, reference_mix


@pytest.mark.parametrize("name,bits", VARIANTS)
def test_numpy_restatement_reproduces_the_fixture(golden_dir, name, bits):
    from audiolab_amd import merge                                           # the module under test must exist: the fixture is its yardstick
    assert merge.HEADROOM_DB == 0.1
    g = fixture_of(golden_dir, name, bits)
    stems, widths, source, source_width, prevent = make_case(name, bits)
    r = reference_mix(stems, widths, bits, source, source_width, prevent, NUMPY_OPS)
    assert np.array_equal(r["acc"], g["acc"]) and np.array_equal(r["y2"], g["y2"])
    assert (r["peak"], r["peak1"], r["rms"]) == (g["peak"], g["peak1"], g["rms"])
    same = lambda a, b: a == b or (math.isnan(a) and math.isnan(b))          # raw float64, bit for bit (log10 / pow of this libm)
    assert same(r["f1"], g["f1"]) and same(r["f2"], g["f2"]) and same(r["target_dBFS"], g["target"]) and same(r["gain_dB"], g["gain"])
    assert min(r["margins"]) >= 1e-3                                          # the condition under which np_rms and audioop.rms agree


def test_cases_hit_what_they_are_for(golden_dir):
    hot = fixture_of(golden_dir, "hot", 16)
    assert hot["peak"] == 32768 and (hot["acc"] == -32768).any() and (hot["acc"] == 32767).any()
    assert fixture_of(golden_dir, "hot", 32)["peak"] == 1 << 31
    assert abs(fixture_of(golden_dir, "quiet_source", 32)["gain"] + 23.0) < 0.1
    capped, free = fixture_of(golden_dir, "loud_source", 16), fixture_of(golden_dir, "loud_source_free", 16)
    assert capped["gain"] < free["gain"] and capped["gain"] == -20 * math.log10(capped["peak1"] / 32768)
    at_the_rail = lambda g: int(np.sum(np.abs(g["y2"]) >= 32767))                # capped: the peak sample alone may touch it
    assert at_the_rail(free) > 10 * max(at_the_rail(capped), 1)
    assert fixture_of(golden_dir, "silent_source", 32)["f2"] == 0.0 and not fixture_of(golden_dir, "silent_source", 32)["y2"].any()
    assert fixture_of(golden_dir, "silent_mix", 16)["peak"] == 0
    nf = fixture_of(golden_dir, "nonfinite", 16)["acc"]
    assert nf[1, 9] == 32767 and nf[0, 9] == -32768 and nf[0, 5] == 4096     # +inf, -inf clip; NaN counts as 0 (+ 0.125)


def test_restatements_against_audioop_itself():
    audioop = pytest.importorskip("audioop")
    rng = np.random.default_rng(0)
    for bits, dt in ((16, "<i2"), (32, "<i4")):
        full = 1 << (bits - 1)
        a = rng.integers(-full, full, 4001).astype(dt)
        b = rng.integers(-full, full, 4001).astype(dt)
        a[:4], b[:4] = [-full, full - 1, -full, 0], [-full, full - 1, full - 1, -full]
        unpack = lambda raw: np.frombuffer(raw, dtype=dt).astype(np.int64)
        assert np.array_equal(unpack(audioop.add(a.tobytes(), b.tobytes(), bits // 8)), np_add(a, b, bits))
        for f in (0.0, 0.3, 0.9885530946569389, 1.0, 1.7, 2.5e-10, 40.0):
            assert np.array_equal(unpack(audioop.mul(a.tobytes(), bits // 8, f)), np_mul(a, f, bits))
        assert audioop.max(a.tobytes(), bits // 8) == np_max(a, bits) == full
        assert audioop.rms(a.tobytes(), bits // 8) == np_rms(a, bits)


# ---- wavio --------------------------------------------------------------------------------------------------------------------------
def _fmt(path):
    with open(path, "rb") as f:
        data = f.read(44)
    return struct.unpack("<HHIIHH", data[20:36])


def test_pcm32_round_trip_and_integer_writes(tmp_path):
    from audiolab_amd import wavio
    rng = np.random.default_rng(3)
    ints = rng.integers(-(1 << 31), 1 << 31, (2, 333)).astype(np.int32)
    ints[:, 0], ints[:, 1] = -(1 << 31), (1 << 31) - 1
    p = str(tmp_path / "i32.wav")
    wavio.write_wav(p, ints, 44100, subtype="PCM_32")
    tag, ch, sr, _, block, bits = _fmt(p)
    assert (tag, ch, sr, block, bits) == (1, 2, 44100, 8, 32)
    with open(p, "rb") as f:
        raw = np.frombuffer(f.read()[44:], dtype="<i4").reshape(-1, 2).T
    assert np.array_equal(raw, ints)                                         # the samples themselves, interleaved
    assert np.array_equal(wavio.read_wav(p)[0], (ints.astype(np.float32) / np.float32(2147483648.0)))
    # floats: round to nearest on the 32-bit grid, clipped
    x = np.array([[0.5, -1.0, 1.0, 3.0, -3.0, 2.0 ** -31, 2.0 ** -32, 3 * 2.0 ** -32, 0.25 + 2.0 ** -30]], dtype=np.float64)
    wavio.write_wav(p, x, 8000, subtype="PCM_32")
    with open(p, "rb") as f:
        raw = np.frombuffer(f.read()[44:], dtype="<i4")
    assert raw.tolist() == [1 << 30, -(1 << 31), (1 << 31) - 1, (1 << 31) - 1, -(1 << 31), 1, 0, 2, (1 << 29) + 2]
    # an int16 array under PCM_16 is written as it is
    i16 = np.array([[-32768, 32767, 0, 12345]], dtype=np.int16)
    wavio.write_wav(p, i16, 8000, subtype="PCM_16")
    assert np.array_equal(wavio.read_wav(p)[0], i16.astype(np.float32) / 32768.0)
    with pytest.raises(ValueError):
        wavio.write_wav(p, i16, 8000, subtype="PCM_24")


@pytest.mark.parametrize("subtype,want", [("FLOAT", (32, True)), ("PCM_16", (16, False)), ("PCM_32", (32, False))])
def test_read_wav_info(tmp_path, subtype, want):
    from audiolab_amd import wavio
    p = str(tmp_path / f"{subtype}.wav")
    wavio.write_wav(p, np.zeros((2, 7), np.float32), 22050, subtype=subtype)
    assert wavio.read_wav_info(p) == (2, 22050) + want
    wavio.write_wav(p, np.zeros(7, np.float32), 48000, subtype=subtype)
    assert wavio.read_wav_info(p) == (1, 48000) + want
    assert os.path.getsize(p) > 0
