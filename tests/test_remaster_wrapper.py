"""``Remaster.process_audio`` (audiolab_amd/wrappers/remaster.py; reference wrappers/remaster.py:43-86) on the emulated kernels (-m "not gpu")
and on the GPU (-m gpu), with tiny WAV files: the output's name, ``add_output``, the callback sequence (its first call unguarded, as in the
reference), ``use_source_track_as_reference`` overriding ``reference_track``, the missing-reference ValueError, and that the file written is
24-bit PCM holding the samples of ``remaster_file``."""
import os

import numpy as np
import pytest

CONFIG = dict(n_fft=256, P=3000)


def _sig(seed, n, channels=1, gain=0.2):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 44100.0
    x = gain * rng.standard_normal((channels, n)) + 0.3 * np.sin(2 * np.pi * 440.0 * t)
    return np.clip(x, -1.0, 1.0).astype(np.float32)


@pytest.fixture()
def project(tmp_path, monkeypatch, dev):
    """source/song.wav (16-bit stereo) and two selected files, stems/song(Vocals).wav (float32 mono) and stems/song(Other).wav, as last_outputs;
    reference.wav beside them"""
    from audiolab_amd import master, wavio
    from audiolab_amd.handlers import config
    from audiolab_amd.util.data_classes import ProjectFiles
    from audiolab_amd.wrappers.remaster import Remaster
    monkeypatch.setattr(config, "output_path", str(tmp_path / "outputs"))
    monkeypatch.setattr(Remaster, "ctx", dev)
    monkeypatch.setattr(Remaster, "config", master.MasterConfig(**CONFIG))
    src = tmp_path / "song.wav"
    wavio.write_wav(str(src), _sig(1, 1500, channels=2), 44100, subtype="PCM_16")
    wavio.write_wav(str(tmp_path / "reference.wav"), _sig(5, 2000, channels=2, gain=0.05), 44100, subtype="PCM_16")
    p = ProjectFiles(str(src))
    stem_dir = os.path.join(p.project_dir, "stems")
    os.makedirs(stem_dir)
    stems = [os.path.join(stem_dir, "song(Vocals).wav"), os.path.join(stem_dir, "song(Other).wav")]
    wavio.write_wav(stems[0], _sig(2, 2700), 44100, subtype="FLOAT")
    wavio.write_wav(stems[1], _sig(3, 900, channels=2), 44100, subtype="FLOAT")
    p.add_output("stems", stems)
    return p


def test_class_attributes():
    from audiolab_amd.wrappers import Remaster
    assert Remaster.title == "Remaster" and Remaster.priority == 7 and Remaster().title == "Remaster"
    assert Remaster.description == "Remaster audio files using a reference track. Uses Matchering."
    assert list(Remaster.allowed_kwargs) == ["use_source_track_as_reference", "reference_track"]
    use, ref = Remaster.allowed_kwargs["use_source_track_as_reference"], Remaster.allowed_kwargs["reference_track"]
    assert use.type is bool and use.field.default is True and use.gradio_type == "Checkbox"
    assert use.description == "Use the source audio as the reference track. (Overrides the reference track input)"
    assert ref.type is str and ref.field.default is None and ref.gradio_type == "File"
    assert ref.description == "The reference track to use for the remastering process."
    assert Remaster.ctx is None and Remaster.config is None


def test_names_outputs_and_callbacks(dev, project, tmp_path):
    from audiolab_amd import master, wavio
    from audiolab_amd.wrappers import Remaster
    stems = list(project.last_outputs)
    want = [os.path.join(project.project_dir, "remastered", n) for n in ("song(Vocals)(Remastered).wav", "song(Other)(Remastered).wav")]
    seen = []
    out = Remaster().process_audio([project], callback=lambda *a: seen.append(a), use_source_track_as_reference=True,
                                   reference_track=str(tmp_path / "reference.wav"))
    assert out == [project] and project.last_outputs == want and project.output_dict["remaster"] == want
    assert seen == [(0, "Remastering 1 audio files", 1), (0, f"Remastering {stems[0]}", 1), (1, f"Remastering {stems[1]}", 1)]
    # the source track was the reference, although a reference_track was given; 24-bit PCM with the samples of remaster_file
    for stem, path in zip(stems, want):
        assert wavio.read_wav_info(path) == (2, 44100, 24, False)
        other = str(tmp_path / "direct.wav")
        res = master.remaster_file(stem, project.src_file, other, master.MasterConfig(**CONFIG), ctx=dev)
        with open(path, "rb") as f, open(other, "rb") as g:
            assert f.read() == g.read()
        back, _ = wavio.read_wav_interleaved(path)
        assert np.array_equal(back.reshape(-1, 2).T * 8388608.0, np.rint(res.result.cpu().numpy() * 8388607.0))


def test_a_reference_track(dev, project, tmp_path):
    from audiolab_amd import master
    from audiolab_amd.wrappers import Remaster
    project.add_output("stems", [project.output_dict["stems"][0]])
    ref = str(tmp_path / "reference.wav")
    out = Remaster().process_audio([project], callback=lambda *a: None, use_source_track_as_reference=False, reference_track=ref)
    path = os.path.join(project.project_dir, "remastered", "song(Vocals)(Remastered).wav")
    assert out == [project] and project.last_outputs == [path]
    other = str(tmp_path / "direct.wav")
    master.remaster_file(project.output_dict["stems"][0], ref, other, master.MasterConfig(**CONFIG), ctx=dev)
    with open(path, "rb") as f, open(other, "rb") as g:
        assert f.read() == g.read()
    master.remaster_file(project.output_dict["stems"][0], project.src_file, other, master.MasterConfig(**CONFIG), ctx=dev)
    with open(path, "rb") as f, open(other, "rb") as g:
        assert f.read() != g.read()


def test_no_reference_is_a_value_error(dev, project):
    from audiolab_amd.wrappers import Remaster
    seen = []
    for kw in ({}, dict(use_source_track_as_reference=False), dict(use_source_track_as_reference=False, reference_track="")):
        with pytest.raises(ValueError, match="Reference track not provided"):
            Remaster().process_audio([project], callback=lambda *a: seen.append(a), **kw)
    assert seen == [] and "remaster" not in project.output_dict


def test_the_first_callback_is_not_guarded(dev, project):
    from audiolab_amd.wrappers import Remaster
    with pytest.raises(TypeError):
        Remaster().process_audio([project], use_source_track_as_reference=True)
    assert "remaster" not in project.output_dict


def test_an_error_is_reported_and_raised(dev, project):
    from audiolab_amd import wavio
    from audiolab_amd.wrappers import Remaster
    short = os.path.join(project.project_dir, "stems", "short.wav")
    wavio.write_wav(short, _sig(4, 100), 44100)
    project.add_output("stems", [short])
    seen = []
    with pytest.raises(ValueError, match="at least 256"):
        Remaster().process_audio([project], callback=lambda *a: seen.append(a), use_source_track_as_reference=True)
    assert seen == [(0, "Remastering 1 audio files", 1), (0, f"Remastering {short}", 1), (1, "Error remastering audio")]
    assert "remaster" not in project.output_dict
