"""``Compare.process_audio`` (audiolab_amd/wrappers/compare.py; reference wrappers/compare.py:42-166) on the emulated kernels (-m "not gpu")
and on the GPU (-m gpu), with tiny WAV files: the output's name, that a PNG is written in both render modes, the callback sequence,
``add_output``, the quirks around the number of inputs, a pair of differing rates, and the ``render`` switch."""
import hashlib
import os

import numpy as np
import pytest

PNG = b"\x89PNG\r\n\x1a\n"


def _sig(seed, n, channels=1, gain=0.2):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 44100.0
    x = gain * rng.standard_normal((channels, n)) + 0.3 * np.sin(2 * np.pi * 440.0 * t)
    return np.clip(x, -1.0, 1.0).astype(np.float32)


@pytest.fixture()
def project(tmp_path, monkeypatch, dev):
    """source/song.wav (16-bit stereo, 44.1 kHz) and one selected file, stems/song(Vocals).wav (float32 mono), as last_outputs"""
    from audiolab_amd import wavio
    from audiolab_amd.handlers import config
    from audiolab_amd.util.data_classes import ProjectFiles
    from audiolab_amd.wrappers.compare import Compare
    monkeypatch.setattr(config, "output_path", str(tmp_path / "outputs"))
    monkeypatch.setattr(Compare, "ctx", dev)
    src = tmp_path / "song.wav"
    wavio.write_wav(str(src), _sig(1, 1500, channels=2), 44100, subtype="PCM_16")
    p = ProjectFiles(str(src))
    stem_dir = os.path.join(p.project_dir, "stems")
    os.makedirs(stem_dir)
    other = os.path.join(stem_dir, "song(Vocals).wav")
    wavio.write_wav(other, _sig(2, 2700), 44100, subtype="FLOAT")
    p.add_output("stems", [other])
    return p


def _md5(path):
    with open(path, "rb") as f:
        return hashlib.md5(f.read()).hexdigest()


def _expected_path(project, other):
    name = f"song_VS_{os.path.splitext(os.path.basename(other))[0]}_{_md5(project.src_file)[:6]}_{_md5(other)[:6]}_comparison.png"
    return os.path.join(project.project_dir, "comparisons", name)


@pytest.mark.parametrize("render", ["full", "reduced"])
def test_a_png_with_the_reference_name_and_callbacks(dev, project, monkeypatch, render):
    from audiolab_amd.wrappers import Compare
    monkeypatch.setattr(Compare, "render", render)
    monkeypatch.setattr(Compare, "plot_columns", 300)                        # fewer buckets than samples, so that "reduced" reduces
    monkeypatch.setattr(Compare, "spec_columns", 2)
    other = project.last_outputs[0]
    want = _expected_path(project, other)
    seen = []
    out = Compare().process_audio([project], callback=lambda step, desc, total: seen.append((step, desc, total)))
    assert out == [project] and project.last_outputs == [want] and project.output_dict["comparison"] == [want]
    with open(want, "rb") as f:
        data = f.read()
    assert data[:8] == PNG and len(data) > 1000
    assert seen == [(0, "Starting audio comparison with spectrogram difference", 5),
                    (1, "Loaded/resampled song.wav", 5),
                    (2, "Loaded/resampled song(Vocals).wav", 5),
                    (3, "Calculated differences", 5),
                    (4, f"Saved visualization to {want}", 5)]


def test_class_attributes():
    from audiolab_amd.wrappers.compare import Compare
    assert Compare.title == "Compare" and Compare.priority == 1000000 and Compare.allowed_kwargs == {}
    assert Compare.description == "Compare two audio files using time-domain waveforms and spectrogram differences."
    assert Compare.render == "full" and Compare.ctx is None and Compare.plot_columns == 4096 and Compare.spec_columns == 2048
    assert Compare().title == "Compare"


def test_the_figure_shows_what_compare_arrays_computes(dev, project, monkeypatch):
    """the arrays handed to the plot are those of compare_arrays on [src_file, the selected file], interleaved as they are"""
    from audiolab_amd import compare, wavio
    from audiolab_amd.wrappers.compare import Compare
    from tests.conftest import host
    seen = {}
    monkeypatch.setattr(Compare, "_plot", lambda self, result, path: seen.update(result=result, path=path))
    Compare().process_audio([project])
    a = wavio.read_wav_interleaved(project.src_file)
    b = wavio.read_wav_interleaved(project.output_dict["stems"][0])
    assert len(a[0]) == 3000 and len(b[0]) == 2700
    want = compare.compare_arrays(a, b, ctx=dev)
    got = seen["result"]
    assert tuple(got.differences.shape) == (2700,) and np.array_equal(host(got.differences), host(want.differences))
    assert np.array_equal(host(got.diff_db), host(want.diff_db)) and np.array_equal(host(got.spec1_db), host(want.spec1_db))
    assert seen["path"] == project.last_outputs[0]


def test_two_inputs_end_the_whole_call(dev, project):
    from audiolab_amd import wavio
    from audiolab_amd.wrappers.compare import Compare
    second = os.path.join(project.project_dir, "stems", "song(Instrumental).wav")
    wavio.write_wav(second, _sig(3, 2500), 44100)
    first = project.last_outputs[0]
    project.add_output("stems", [first, second])
    seen = []
    out = Compare().process_audio([project], callback=lambda step, desc, total: seen.append((step, desc, total)))
    assert out == [] and seen == [(0, "Expected exactly 2 unique audio files, got 2.", 1)]
    assert "comparison" not in project.output_dict and not os.path.exists(os.path.join(project.project_dir, "comparisons"))
    assert Compare().process_audio([project]) == []                          # without a callback too


def test_no_audio_input_is_an_index_error(dev, project):
    from audiolab_amd.wrappers.compare import Compare
    note = os.path.join(project.project_dir, "stems", "notes.txt")
    with open(note, "w") as f:
        f.write("not audio")
    project.add_output("stems", [note])
    with pytest.raises(IndexError):
        Compare().process_audio([project])


def test_a_48_khz_file_against_the_44_1_khz_source(dev, project, monkeypatch):
    from audiolab_amd import compare, wavio
    from audiolab_amd.wrappers.compare import Compare
    from tests.conftest import host
    other = os.path.join(project.project_dir, "stems", "song(Vocals)(Cloned).wav")
    wavio.write_wav(other, _sig(4, 2880), 48000, subtype="PCM_16")          # 2880 -> 2646 samples at 44.1 kHz
    project.add_output("cloned", [other])
    results = []
    plot = Compare._plot
    monkeypatch.setattr(Compare, "_plot", lambda self, result, path: (results.append(result), plot(self, result, path)))
    out = Compare().process_audio([project])
    want = _expected_path(project, other)
    assert out == [project] and project.last_outputs == [want]
    with open(want, "rb") as f:
        assert f.read(8) == PNG
    assert tuple(results[0].differences.shape) == (2646,) and results[0].spec1_db.shape[1] == 4
    ref = compare.compare_arrays(project.src_file, other, ctx=dev)
    assert np.array_equal(host(results[0].waveforms[1]), host(ref.waveforms[1]))


def test_a_bad_render_value(dev, project, monkeypatch):
    from audiolab_amd.wrappers.compare import Compare
    monkeypatch.setattr(Compare, "render", "fast")
    with pytest.raises(ValueError, match="render"):
        Compare().process_audio([project])
    assert "comparison" not in project.output_dict
