"""audiolab_amd.tempo (csrc/tempo.h, the ``alsep_tempo_*`` entry points) on the emulated kernels (-m "not gpu") and on the GPU (-m gpu), same
bodies, pinned against tests/tempo_oracle.py (numpy / scipy; parity with librosa itself is unpinned: the library is not available).

Per stage, the kernel gets the ORACLE's input of that stage, so every bound is that stage's own rounding:
  mel power     max|ours - want| <= 1e-12 max(want): the float64 chain rounds near 1e-14 of the peak, a float32 stage cannot pass;
  flux          see test_flux;
  tempogram     1e-12 absolute: its values lie in [-1, 1];
  local score   1e-12 of its peak;
  DP            bit for bit (the kernel only adds and compares; ties go to the lowest index);
  finish        exact.
End to end, ``beat_track_array`` must reproduce the oracle's lag, period and beat frames.  The oracle's decisions on these inputs were checked
for near-ties when the seeds were fixed: the tempo pick wins by >= 4e-4 (>= 0.06 on the click tracks), the DP's best candidate by >= 5e-5,
the half-median and the 1 % threshold are missed by >= 1e-4 -- against rounding differences near 1e-13."""
import functools

import numpy as np
import pytest

from tests import tempo_oracle as o
from tests.conftest import host
from tests.conftest import on as _on


def on(ctx, a):
    """a copy of the (read-only, shared) reference array on the context's device"""
    return _on(ctx, np.array(a))


CLICKS = {  # name: (bpm, seconds, seed, start_bpm)
    "c120": (120.0, 12.0, 1, 120.0), "c90": (90.0, 12.0, 2, 120.0), "c150": (150.0, 6.0, 3, 120.0), "c120_3s": (120.0, 3.0, 4, 120.0),
    "slow45": (45.0, 12.0, 5, 45.0),
}
EXPECT = {"c120": (22, 517), "c90": (29, 517), "c150": (17, 259), "c120_3s": (22, 130), "slow45": (57, 517)}   # (k = period, F)


@functools.lru_cache(maxsize=None)
def signal(name):
    """-> (y, sr, start_bpm)"""
    if name in CLICKS:
        bpm, seconds, seed, start = CLICKS[name]
        y, sr = o.click_track(bpm, seconds, seed), o.SR
    elif name == "lead_silence":                                             # a silent first second: the back = -1 prefix
        y, sr, start = o.click_track(120.0, 6.0, 6, lead_silence=1.0), o.SR, 120.0
    elif name == "stereo_44k":                                               # the resample path; the channels differ by a gain
        m = o.click_track(120.0, 12.0, 1, sr=44100)
        y, sr, start = np.stack([m, 0.5 * m]), 44100, 120.0
    else:                                                                    # "n<samples>": noise; F = 1, 4, 4, 5
        y, sr, start = 0.1 * np.random.default_rng(7).standard_normal(int(name[1:])), o.SR, 120.0
    y.setflags(write=False)
    return y, sr, start


@functools.lru_cache(maxsize=None)
def ref(name):
    y, sr, start = signal(name)
    out = o.beat_track(y, sr, start_bpm=start)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def test_the_filterbank_table_is_the_oracles():
    from audiolab_amd import tempo
    bands, weights = tempo.mel_bands()
    dense = np.zeros((o.N_MELS, o.BINS))
    for i, (first, count, at) in enumerate(bands):
        dense[i, first:first + count] = weights[at:at + count]
    want = o.mel_filterbank()
    # both are differences of frequencies of up to 11025 Hz (ulp 1.8e-12) over widths of 23 Hz and more: 1e-13 of the value, written differently
    assert np.max(np.abs(dense - want)) <= 1e-13 * want.max()
    assert bands[:, 1].min() == 4 and bands[0, 0] == 1 and bands[:, 1].max() == 53          # the narrowest band, the widest one


@pytest.mark.parametrize("name", ["n100", "n1600", "n2047", "n2049", "c120_3s", "c150", "lead_silence"])
def test_mel_power(dev, name):
    from audiolab_amd import tempo
    r = ref(name)
    want = r["mel"]
    got = host(tempo.mel_power(dev, on(dev, r["y"])))
    assert got.shape == want.shape == (128, 1 + len(r["y"]) // 512)
    err = np.max(np.abs(got - want))
    print(f"mel {name}: F {want.shape[1]} max|delta| {err:.3e} of peak {want.max():.3e}")
    assert err <= 1e-12 * want.max()


@pytest.mark.parametrize("name", ["n100", "n1600", "n2049", "c120_3s", "c120", "lead_silence"])
def test_flux(dev, name):
    """The kernel gets the oracle's mel array.  A linear error of 1e-12 max(M) in a value v moves 10 log10(v) by (10 / ln 10) 1e-12 max(M) / v =
    4.343e-12 max(M) / v dB; values are floored at 1e-10, so the bound per decibel element is 4.343e-12 max(M) / max(v, 1e-10).  An element
    at the floor max(D) - 80 carries the error of the maximum, 4.343e-12 dB, which is no more than that.  The envelope is a difference of two
    such elements, then a selection (rectifier, median: 1-Lipschitz in every input): twice the largest bound among the elements above the floor,
    and at least twice 4.343e-12."""
    from audiolab_amd import tempo
    r = ref(name)
    mel, want_db, want_env = r["mel"], r["db"], r["env"]
    db, env = (host(v) for v in tempo.flux(dev, on(dev, mel)))
    bound = 4.343e-12 * mel.max() / np.maximum(mel, 1e-10)
    floored = want_db <= want_db.max() - 80.0
    bound = np.where(floored, 4.343e-12, bound)
    err_db, err_env = np.abs(db - want_db), np.max(np.abs(env - want_env))
    print(f"flux {name}: max dB error {err_db.max():.3e} (bound >= {bound.min():.3e}), envelope error {err_env:.3e} (bound {2 * bound.max():.3e})")
    assert np.all(err_db <= bound)
    assert err_env <= 2.0 * bound.max()
    assert np.all(env[:3] == 0.0)


@pytest.mark.parametrize("name", ["n1600", "c120_3s", "c120", "lead_silence"])
def test_tempogram_mean(dev, name):
    from audiolab_amd import tempo
    r = ref(name)
    got = host(tempo.tempogram_mean(dev, on(dev, r["env"])))
    err = np.max(np.abs(got - r["tg"]))
    print(f"tempogram {name}: F {len(r['env'])} max|delta| {err:.3e}")
    assert got.shape == (344,) and err <= 1e-12
    assert int(np.argmax(tempo.tempo_scores(got)[1])) == int(np.argmax(o.tempo_scores(r["tg"])[1]))


@pytest.mark.parametrize("name,period", [("c150", 17), ("c120", 22), ("c90", 29), ("c120", 64), ("n1600", 19), ("c120_3s", 343)])
def test_local_score(dev, name, period):
    from audiolab_amd import tempo
    env = ref(name)["env"]
    want = o.local_score(env, period)
    got = host(tempo.local_score(dev, on(dev, env), period))
    err = np.max(np.abs(got - want))
    print(f"local score {name} period {period}: max|delta| {err:.3e} of peak {np.max(np.abs(want)):.3e}")
    assert err <= 1e-12 * np.max(np.abs(want))


@pytest.mark.parametrize("name,period", [("c150", 17), ("c120", 22), ("c90", 29), ("c120", 64), ("slow45", 57), ("lead_silence", 22), ("n2049", 19),
                                         ("c120", 343)])
def test_beat_dp_bit_for_bit(dev, name, period):
    """the oracle's local score, bit for bit, and the host tables: cum and back match exactly; 64 and 343 make the window wider than a wave
    (97 and 515 offsets)"""
    from audiolab_amd import tempo
    ls = o.local_score(ref(name)["env"], period)
    want_cum, want_back = o.beat_dp(ls, period)
    cum, back = (host(v) for v in tempo.beat_dp(dev, on(dev, ls), period))
    assert back.dtype == np.int32 and np.array_equal(back, want_back)
    assert np.array_equal(cum, want_cum)
    if name == "lead_silence":
        assert np.all(want_back[:40] == -1) and want_back.max() > 0


def test_beat_dp_ties_go_to_the_lowest_index(dev):
    """no transition cost and small whole numbers for scores: every step has exact ties among its candidates"""
    from audiolab_amd import tempo
    ls = np.random.default_rng(11).integers(0, 3, 300).astype(np.float64)
    for period in (9, 40):
        want_cum, want_back = o.beat_dp(ls, period, tightness=0.0)
        cum, back = (host(v) for v in tempo.beat_dp(dev, on(dev, ls), period, tightness=0.0))
        assert np.array_equal(back, want_back) and np.array_equal(cum, want_cum)


@pytest.mark.parametrize("name", list(CLICKS) + ["lead_silence", "n1600", "n2049"])
def test_finish_is_exact(name):
    from audiolab_amd import tempo
    r = ref(name)
    for trim in (True, False):
        want = o.finish(r["cum"], r["back"], r["ls"], trim)
        got = tempo.finish(r["cum"], r["back"], r["ls"], trim)
        assert got.dtype == want.dtype and np.array_equal(got, want)
    assert len(o.finish(r["cum"], r["back"], r["ls"], False)) >= len(r["beats"]) >= 1


@pytest.mark.parametrize("name", list(CLICKS) + ["lead_silence", "stereo_44k", "n1600", "n2047", "n2049"])
def test_end_to_end_matches_the_oracle(dev, name):
    from audiolab_amd import tempo
    y, sr, start = signal(name)
    r = ref(name)
    res = tempo.beat_track_array(np.array(y), sr, dev, start_bpm=start, want_stages=True)
    print(f"{name}: k {res.k} bpm {res.bpm:.3f} period {res.period} beats {res.beat_frames.tolist()}")
    assert (res.k, res.period) == (r["k"], r["period"]) and res.bpm == r["bpm"]
    assert np.array_equal(res.beat_frames, r["beats"]) and np.array_equal(res.beat_times, r["beat_times"])
    assert np.array_equal(host(res.stages["back"]), r["back"])
    if name in EXPECT:
        assert (res.k, len(r["env"])) == EXPECT[name]


@pytest.mark.parametrize("name", list(CLICKS) + ["stereo_44k"])
def test_click_tracks_without_the_oracle(dev, name):
    """the reported tempo is one of the two grid tempi 60 * 22050 / (512 k) around the true one; every inter-beat interval is period +- 1"""
    from audiolab_amd import tempo
    y, sr, start = signal(name)
    true = CLICKS[name][0] if name in CLICKS else 120.0
    res = tempo.beat_track_array(np.array(y), sr, dev, start_bpm=start)
    grid = 60.0 * 22050 / (512.0 * np.arange(1, 344))
    above, below = grid[grid >= true].min(), grid[grid <= true].max()
    assert res.bpm in (above, below)
    gaps = np.diff(res.beat_frames)
    assert len(gaps) >= 4 and np.all(np.abs(gaps - res.period) <= 1)


def test_silence_and_the_shortest_tracks_have_no_tempo(dev):
    from audiolab_amd import tempo
    for y in (np.zeros(4096), np.zeros((2, 30000)), signal("n100")[0], np.ones(1)):
        res = tempo.beat_track_array(np.array(y), 22050, dev)
        assert res.bpm == 0.0 and len(res.beat_frames) == 0 and len(res.beat_times) == 0
    assert ref("n100")["bpm"] == 0.0


def test_refusals(dev):
    from audiolab_amd import tempo
    with pytest.raises(ValueError, match="60 minutes"):
        tempo.beat_track_array(np.zeros(3601 * 8), 8, dev)
    with pytest.raises(ValueError):
        tempo.beat_track_array(np.zeros((2, 2, 8)), 22050, dev)
    with pytest.raises(ValueError):
        tempo.beat_track_array(np.zeros(100), 22050, dev, tightness=0.0)
    assert dev.lib.alsep_tempo_frames(0) == -1 and dev.lib.alsep_tempo_frames(3600 * 22050 + 1) == -1
    assert dev.lib.alsep_tempo_frames(2047) == 4 and dev.lib.alsep_tempo_frames(3600 * 22050) == 155040


def test_detect_bpm(dev, tmp_path):
    """the reference's helper: the file is cut before resampling, an unreadable file gives (0, [])"""
    from audiolab_amd import tempo, wavio
    y, sr, _ = signal("stereo_44k")
    path = str(tmp_path / "song(Instrumental).wav")
    wavio.write_wav(path, y.astype(np.float32), sr, subtype="FLOAT")
    stored = y.astype(np.float32).astype(np.float64)
    bpm, times = tempo.detect_bpm(path, 1.0, 4.0, ctx=dev)
    want = tempo.beat_track_array(stored[:, 44100:4 * 44100], sr, dev)
    assert bpm == want.bpm > 0 and times == [float(t) for t in want.beat_times] and all(isinstance(t, float) for t in times)
    assert bpm == o.beat_track(stored[:, 44100:4 * 44100], sr)["bpm"]
    junk = str(tmp_path / "junk.wav")
    with open(junk, "wb") as f:
        f.write(b"not a wave file")
    assert tempo.detect_bpm(junk, ctx=dev) == (0, [])
    assert tempo.detect_bpm(str(tmp_path / "missing.wav"), ctx=dev) == (0, [])
