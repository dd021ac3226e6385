"""The Merge wrapper (audiolab_amd/wrappers/merge.py; reference wrappers/merge.py:48-191) and ``merge_files`` on the emulated kernels
(-m "not gpu") and on the GPU (-m gpu), with tiny WAV files: file names, the re-reverb branch and its ``src_name`` quirk, output subtype,
bookkeeping, progress callbacks, the error path, and the written samples against ``mixdown_array``."""
import json
import os

import numpy as np
import pytest

from tests.conftest import host, on

SR = 8000


def _sig(seed, n, channels=2, gain=0.2):
    rng = np.random.default_rng(seed)
    return np.clip(gain * rng.standard_normal((channels, n)), -1.0, 1.0).astype(np.float32)


@pytest.fixture()
def project(tmp_path, monkeypatch, dev):
    """a project after Separate: source/song.wav (PCM_16) and three float32 stems as last_outputs"""
    from audiolab_amd import wavio
    from audiolab_amd.handlers import config
    from audiolab_amd.util.data_classes import ProjectFiles
    from audiolab_amd.wrappers.merge import Merge
    monkeypatch.setattr(config, "output_path", str(tmp_path / "outputs"))
    monkeypatch.setattr(Merge, "ctx", dev)
    src = tmp_path / "song.wav"
    wavio.write_wav(str(src), _sig(1, 900, gain=0.1), SR, subtype="PCM_16")
    p = ProjectFiles(str(src))
    stem_dir = os.path.join(p.project_dir, "stems")
    os.makedirs(stem_dir)
    stems = []
    for k, (label, n) in enumerate([("(Vocals)", 801), ("(BG_Vocals)", 700), ("(Instrumental)", 1000)]):
        path = os.path.join(stem_dir, f"song{label}.wav")
        wavio.write_wav(path, _sig(10 + k, n), SR)
        stems.append(path)
    p.add_output("stems", stems)
    return p


def _store_ir(project):
    ir = np.zeros(40)
    ir[0], ir[7], ir[39] = 1.0, 0.4, -0.2
    path = os.path.join(project.project_dir, "stems", "impulse_response.ir")
    with open(path, "w") as f:
        json.dump({"sample_rate": SR, "pre_delay": 0.001, "impulse_response": ir.tolist()}, f)
    return ir, int(0.001 * SR)


def _expected(dev, stems, widths, src_path):
    from audiolab_amd import merge, wavio
    src = wavio.read_wav(src_path)[0]
    out, rec = merge.mixdown_array([on(dev, s) for s in stems], (on(dev, src), wavio.read_wav_info(src_path)[2]), src_bits=widths, ctx=dev)
    return host(out), rec


def _samples(path):
    with open(path, "rb") as f:
        data = f.read()
    bits = int.from_bytes(data[34:36], "little")
    ch = int.from_bytes(data[22:24], "little")
    return np.frombuffer(data[44:], dtype="<i2" if bits == 16 else "<i4").reshape(-1, ch).T, bits


def test_surface_matches_the_reference():
    from audiolab_amd.wrappers.merge import Merge
    m = Merge()
    assert (m.title, Merge.priority, Merge.default) == ("Merge", 6, True) and Merge() is m
    assert list(Merge.allowed_kwargs) == ["pitch_shift", "prevent_clipping", "selected_voice", "pitch_extraction_method"]
    d = {k: v.field.default for k, v in Merge.allowed_kwargs.items()}
    assert d == {"pitch_shift": 0, "prevent_clipping": True, "selected_voice": "Vocals", "pitch_extraction_method": "rmvpe+"}
    ps = Merge.allowed_kwargs["pitch_shift"]
    assert (ps.field.ge, ps.field.le, ps.render, ps.gradio_type, ps.type) == (-24, 24, False, "Slider", int)
    assert Merge.allowed_kwargs["prevent_clipping"].render and not Merge.allowed_kwargs["selected_voice"].render


def test_merges_the_stems_in_order(dev, project):
    from audiolab_amd import wavio
    from audiolab_amd.wrappers.merge import Merge
    stems = list(project.last_outputs)
    seen = []
    out = Merge().process_audio([project], callback=lambda frac, desc, total: seen.append((frac, desc, total)), bogus_option=3)
    merged = os.path.join(project.project_dir, "merged", "song(Merged).wav")    # selected_voice not passed: None, no name_str (:91,137)
    assert out == [project] and project.last_outputs == [merged] and project.output_dict["merged"] == [merged]
    assert seen == [(i / 3, f"Processing stem: {os.path.basename(s)}", 3) for i, s in enumerate(stems)]
    got, bits = _samples(merged)
    assert bits == 32 and wavio.read_wav_info(merged) == (2, SR, 32, False)     # float32 stems: a 32-bit mix
    want, rec = _expected(dev, [wavio.read_wav(s)[0] for s in stems], [32, 32, 32], project.src_file)
    assert got.shape == (2, 801) and np.array_equal(got, want) and rec.peak > 0
    assert not os.path.exists(os.path.join(project.project_dir, "stems", "song(Vocals)(Re-Reverb).wav"))   # no IR stored


def test_selected_voice_names_the_file_and_an_old_one_is_replaced(dev, project):
    from audiolab_amd.wrappers.merge import Merge
    folder = os.path.join(project.project_dir, "merged")
    os.makedirs(folder)
    target = os.path.join(folder, "song(Ann_rmvpe+)(Merged).wav")
    with open(target, "wb") as f:
        f.write(b"stale")
    stems = list(project.last_outputs)
    two = []
    Merge().process_audio([project], callback=lambda frac, desc: two.append(frac), selected_voice="Ann")        # a 2-argument callback
    assert two == [0.0, 1 / 3, 2 / 3] and project.last_outputs == [target]
    assert _samples(target)[0].shape == (2, 801)
    project.add_output("stems", stems)
    Merge().process_audio([project], selected_voice="Ann", pitch_extraction_method="crepe", prevent_clipping=False)
    assert project.last_outputs == [os.path.join(folder, "song(Ann_crepe)(Merged).wav")]
    project.add_output("stems", stems)
    Merge().process_audio([project], selected_voice="")
    assert project.last_outputs == [os.path.join(folder, "song(Merged).wav")]


def test_stored_room_goes_back_on_the_main_vocals_only(dev, project):
    from audiolab_amd import reverb, wavio
    from audiolab_amd.wrappers.merge import Merge
    ir, pre = _store_ir(project)
    stems = list(project.last_outputs)
    Merge().process_audio([project], selected_voice="Ann")
    stem_dir = os.path.join(project.project_dir, "stems")
    rr = os.path.join(stem_dir, "song(Vocals)(Re-Reverb).wav")
    assert wavio.read_wav_info(rr) == (2, SR, 16, False)                        # written as sf.write does for .wav: PCM_16
    assert sorted(f for f in os.listdir(stem_dir) if "Re-Reverb" in f) == ["song(Vocals)(Re-Reverb).wav"]   # the BG vocals keep theirs off
    # the quirk of :115: src_name is the vocal stem's name minus "(Vocals)" from then on -- the same string here
    merged = os.path.join(project.project_dir, "merged", "song(Ann_rmvpe+)(Merged).wav")
    assert project.last_outputs == [merged]
    audio = [wavio.read_wav(s)[0] for s in stems]
    wet = reverb.apply_reverb_array(on(dev, audio[0]), ir, pre, ctx=dev)
    assert np.array_equal(wavio.read_wav(rr)[0], np.clip(np.rint(host(wet).astype(np.float64) * 32768), -32768, 32767).astype(np.float32) / 32768)
    # the device signal enters the mix with source width 16: the values the reference reads back from the file
    want, _ = _expected(dev, [wavio.read_wav(rr)[0], audio[1], audio[2]], [16, 32, 32], project.src_file)
    got, bits = _samples(merged)
    assert bits == 32 and np.array_equal(got, want)


def test_src_name_quirk_takes_the_vocal_stems_name(dev, project):
    from audiolab_amd import wavio
    from audiolab_amd.wrappers.merge import Merge
    _store_ir(project)
    cloned = os.path.join(project.project_dir, "stems", "take2(Vocals)(Cloned).wav")
    wavio.write_wav(cloned, _sig(30, 500), SR, subtype="PCM_16")
    inst = [p for p in project.last_outputs if "Instrumental" in p][0]
    project.add_output("cloned", [inst, cloned])
    Merge().process_audio([project])
    assert project.last_outputs == [os.path.join(project.project_dir, "merged", "take2(Cloned)(Merged).wav")]
    assert os.path.exists(os.path.join(project.project_dir, "stems", "take2(Vocals)(Cloned)(Re-Reverb).wav"))


def test_all_16_bit_stems_give_a_16_bit_file(dev, project):
    from audiolab_amd import wavio
    from audiolab_amd.wrappers.merge import Merge
    paths = []
    for k in range(2):
        path = os.path.join(project.project_dir, "stems", f"pcm{k}.wav")
        wavio.write_wav(path, _sig(40 + k, 301 + k), SR, subtype="PCM_16")
        paths.append(path)
    project.add_output("stems", paths)
    Merge().process_audio([project])
    merged = project.last_outputs[0]
    got, bits = _samples(merged)
    assert bits == 16 and wavio.read_wav_info(merged) == (2, SR, 16, False)
    want, rec = _expected(dev, [wavio.read_wav(p)[0] for p in paths], [16, 16], project.src_file)
    assert rec.bits == 16 and np.array_equal(got, want)


def test_error_path_calls_back_and_raises_again(dev, project):
    from audiolab_amd import wavio
    from audiolab_amd.wrappers.merge import Merge
    seen = []
    cb = lambda frac, desc, total: seen.append((frac, desc, total))
    with pytest.raises(NotImplementedError):                                     # rubberband is not built; nothing is written
        Merge().process_audio([project], callback=cb, pitch_shift=2)
    assert seen == [(1.0, "Error merging audio files.", 1)] and "merged" not in project.output_dict
    assert not os.listdir(os.path.join(project.project_dir, "merged"))
    other = os.path.join(project.project_dir, "stems", "other_rate.wav")
    wavio.write_wav(other, _sig(50, 100), SR * 2)
    project.add_output("stems", project.last_outputs + [other])
    del seen[:]
    with pytest.raises(ValueError, match="sample rates"):
        Merge().process_audio([project], callback=lambda frac, desc: seen.append((frac, desc)))
    assert seen[-1] == (1.0, "Error merging audio files.") and len(seen) == 5


def test_merge_files_takes_device_signals(dev, tmp_path):
    from audiolab_amd import merge, wavio
    a, b = _sig(60, 257), _sig(61, 300, channels=1)
    src, pa, out = str(tmp_path / "src.wav"), str(tmp_path / "a.wav"), str(tmp_path / "out.wav")
    wavio.write_wav(src, _sig(62, 400, gain=0.05), SR)
    wavio.write_wav(pa, a, SR)
    rec = merge.merge_files([pa, (on(dev, b), SR, 16)], src, out, ctx=dev)
    want, rec_w = _expected(dev, [a, b], [32, 16], src)
    got, bits = _samples(out)
    assert bits == 32 and rec == rec_w and np.array_equal(got, want)
    rec16 = merge.merge_files([pa, (on(dev, b), SR, 16)], src, out, bits=16, prevent_clipping=False, ctx=dev)   # forced onto the 16-bit grid
    assert rec16.bits == 16 and _samples(out)[1] == 16
