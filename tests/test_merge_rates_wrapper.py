"""The Merge wrapper and ``merge_files`` with stems of differing sample rates (``mixed_rates="ratecv"``) on the emulated kernels
(-m "not gpu") and on the GPU (-m gpu), with tiny WAV files at 8000, 11025 and 16000 Hz: the rate in the written header, the written samples
against ``mixdown_array(..., rates=...)`` (itself pinned to ``audioop`` by tests/test_merge_rates.py), the bookkeeping and callbacks, the
re-reverb branch with a vocal stem at another rate, a device-signal tuple at another rate, and the default, which still raises."""
import json
import os

import numpy as np
import pytest

from tests.conftest import host, on

RATES = {"(Vocals)": 11025, "(BG_Vocals)": 8000, "(Instrumental)": 16000}


def _sig(seed, n, channels=2, gain=0.2):
    rng = np.random.default_rng(seed)
    return np.clip(gain * rng.standard_normal((channels, n)), -1.0, 1.0).astype(np.float32)


@pytest.fixture()
def project(tmp_path, monkeypatch, dev):
    """a project after Separate and Clone: source/song.wav (PCM_16, 16000 Hz) and three float32 stems at three rates as last_outputs"""
    from audiolab_amd import wavio
    from audiolab_amd.handlers import config
    from audiolab_amd.util.data_classes import ProjectFiles
    from audiolab_amd.wrappers.merge import Merge
    monkeypatch.setattr(config, "output_path", str(tmp_path / "outputs"))
    monkeypatch.setattr(Merge, "ctx", dev)
    src = tmp_path / "song.wav"
    wavio.write_wav(str(src), _sig(1, 900, gain=0.1), 16000, subtype="PCM_16")
    p = ProjectFiles(str(src))
    stem_dir = os.path.join(p.project_dir, "stems")
    os.makedirs(stem_dir)
    stems = []
    for k, (label, n) in enumerate([("(Vocals)", 801), ("(BG_Vocals)", 700), ("(Instrumental)", 1000)]):
        path = os.path.join(stem_dir, f"song{label}.wav")
        wavio.write_wav(path, _sig(10 + k, n), RATES[label])
        stems.append(path)
    p.add_output("stems", stems)
    return p


def _expected(dev, stems, widths, rates, src_path):
    from audiolab_amd import merge, wavio
    src = wavio.read_wav(src_path)[0]
    out, rec = merge.mixdown_array([on(dev, s) for s in stems], (on(dev, src), wavio.read_wav_info(src_path)[2]), src_bits=widths, ctx=dev,
                                   rates=rates)
    return host(out), rec


def _samples(path):
    with open(path, "rb") as f:
        data = f.read()
    bits = int.from_bytes(data[34:36], "little")
    ch = int.from_bytes(data[22:24], "little")
    return np.frombuffer(data[44:], dtype="<i2" if bits == 16 else "<i4").reshape(-1, ch).T, bits


def test_the_switch_is_a_class_attribute_not_a_kwarg():
    from audiolab_amd.wrappers.merge import Merge
    assert Merge.mixed_rates == "error"
    assert list(Merge.allowed_kwargs) == ["pitch_shift", "prevent_clipping", "selected_voice", "pitch_extraction_method"]


def test_merges_stems_of_three_rates(dev, project, monkeypatch):
    from audiolab_amd import merge, wavio
    from audiolab_amd.wrappers.merge import Merge
    monkeypatch.setattr(Merge, "mixed_rates", "ratecv")
    stems = list(project.last_outputs)
    seen = []
    out = Merge().process_audio([project], callback=lambda frac, desc, total: seen.append((frac, desc, total)), mixed_rates="error", bogus=3)
    merged = os.path.join(project.project_dir, "merged", "song(Merged).wav")
    assert out == [project] and project.last_outputs == [merged] and project.output_dict["merged"] == [merged]
    assert seen == [(i / 3, f"Processing stem: {os.path.basename(s)}", 3) for i, s in enumerate(stems)]
    assert wavio.read_wav_info(merged) == (2, 16000, 32, False)                  # the largest rate in the header
    got, bits = _samples(merged)
    rates = [11025, 8000, 16000]
    want, rec = _expected(dev, [wavio.read_wav(s)[0] for s in stems], [32, 32, 32], rates, project.src_file)
    assert rec.rate == 16000 and rec.peak > 0
    assert got.shape == (2, merge.ratecv_length(801, 11025, 16000)) and np.array_equal(got, want)


def test_the_default_still_raises_and_names_the_switch(dev, project):
    from audiolab_amd import merge
    from audiolab_amd.wrappers.merge import Merge
    seen = []
    with pytest.raises(ValueError, match="sample rates") as e:
        Merge().process_audio([project], callback=lambda frac, desc: seen.append((frac, desc)))
    assert "mixed_rates" in str(e.value)
    assert seen[-1] == (1.0, "Error merging audio files.") and "merged" not in project.output_dict
    assert not os.listdir(os.path.join(project.project_dir, "merged"))
    with pytest.raises(ValueError, match="mixed_rates"):
        merge.merge_files(list(project.last_outputs), project.src_file, os.path.join(project.project_dir, "x.wav"), ctx=dev, mixed_rates="resample")


def test_stored_room_goes_back_on_vocals_of_another_rate(dev, project, monkeypatch):
    from audiolab_amd import reverb, wavio
    from audiolab_amd.wrappers.merge import Merge
    monkeypatch.setattr(Merge, "mixed_rates", "ratecv")
    ir = np.zeros(40)
    ir[0], ir[7], ir[39] = 1.0, 0.4, -0.2
    with open(os.path.join(project.project_dir, "stems", "impulse_response.ir"), "w") as f:
        json.dump({"sample_rate": 11025, "pre_delay": 0.001, "impulse_response": ir.tolist()}, f)
    stems = list(project.last_outputs)
    Merge().process_audio([project])
    rr = os.path.join(project.project_dir, "stems", "song(Vocals)(Re-Reverb).wav")
    assert wavio.read_wav_info(rr) == (2, 11025, 16, False)                      # the reverb runs and is written at the stem's own rate
    merged = project.last_outputs[0]
    assert wavio.read_wav_info(merged) == (2, 16000, 32, False)
    audio = [wavio.read_wav(s)[0] for s in stems]
    wet = reverb.apply_reverb_array(on(dev, audio[0]), ir, int(0.001 * 11025), ctx=dev)
    assert np.array_equal(host(wet).shape, audio[0].shape)
    # the device signal enters the mix with source width 16 at its own rate; the mix is resampled when the 16 kHz stem arrives
    want, _ = _expected(dev, [wavio.read_wav(rr)[0], audio[1], audio[2]], [16, 32, 32], [11025, 8000, 16000], project.src_file)
    got, bits = _samples(merged)
    assert bits == 32 and np.array_equal(got, want)


def test_merge_files_takes_a_device_signal_of_another_rate(dev, tmp_path):
    from audiolab_amd import merge, wavio
    a, b = _sig(60, 257), _sig(61, 300, channels=1)
    src, pa, out = str(tmp_path / "src.wav"), str(tmp_path / "a.wav"), str(tmp_path / "out.wav")
    wavio.write_wav(src, _sig(62, 400, gain=0.05), 8000)
    wavio.write_wav(pa, a, 8000)
    with pytest.raises(ValueError, match="sample rates"):
        merge.merge_files([pa, (on(dev, b), 11025, 16)], src, out, ctx=dev)
    assert not os.path.exists(out)
    rec = merge.merge_files([pa, (on(dev, b), 11025, 16)], src, out, ctx=dev, mixed_rates="ratecv")
    want, rec_w = _expected(dev, [a, b], [32, 16], [8000, 11025], src)
    got, bits = _samples(out)
    assert bits == 32 and rec == rec_w and rec.rate == 11025 and wavio.read_wav_info(out)[1] == 11025
    assert got.shape == (2, merge.ratecv_length(257, 8000, 11025)) and np.array_equal(got, want)
    # the other way round: the device signal is the one below the rate, the file keeps its length
    rec = merge.merge_files([pa, (on(dev, b), 4000, 16)], src, out, ctx=dev, mixed_rates="ratecv")
    got, _ = _samples(out)
    want, _ = _expected(dev, [a, b], [32, 16], [8000, 4000], src)
    assert rec.rate == 8000 and wavio.read_wav_info(out)[1] == 8000 and got.shape == (2, 257) and np.array_equal(got, want)
    # equal rates with the switch on: exactly the record and the file of the default
    rec_e = merge.merge_files([pa, (on(dev, b), 8000, 16)], src, out, ctx=dev, mixed_rates="ratecv")
    rec_d = merge.merge_files([pa, (on(dev, b), 8000, 16)], src, str(tmp_path / "out2.wav"), ctx=dev)
    assert rec_e == rec_d and open(out, "rb").read() == open(str(tmp_path / "out2.wav"), "rb").read()
