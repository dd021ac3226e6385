"""``Merge.process_audio(..., pitch_shift=s)`` with ``Merge.pitch_shifter = "vocoder"`` (audiolab_amd/wrappers/merge.py; reference
wrappers/merge.py:125-127 -> util/audio_track.py:603-694) on the emulated kernels (-m "not gpu") and on the GPU (-m gpu), with tiny WAV
files: which stems are shifted, with which width they enter the mix, what reaches the disk, and the two switches."""
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
    """a project after Separate and Clone: source/song.wav (PCM_16), two float32 stems and a 16-bit cloned voice as last_outputs"""
    from audiolab_amd import wavio
    from audiolab_amd.handlers import config
    from audiolab_amd.util.data_classes import ProjectFiles
    from audiolab_amd.wrappers.merge import Merge
    monkeypatch.setattr(config, "output_path", str(tmp_path / "outputs"))
    monkeypatch.setattr(Merge, "ctx", dev)
    monkeypatch.setattr(Merge, "pitch_shifter", "vocoder")
    src = tmp_path / "song.wav"
    wavio.write_wav(str(src), _sig(1, 900, gain=0.1), SR, subtype="PCM_16")
    p = ProjectFiles(str(src))
    stem_dir = os.path.join(p.project_dir, "stems")
    os.makedirs(stem_dir)
    stems = []
    for k, (label, n, subtype) in enumerate([("(Vocals)", 801, "FLOAT"), ("(Instrumental)", 1000, "FLOAT"), ("(Vocals)(Cloned)", 640, "PCM_16")]):
        path = os.path.join(stem_dir, f"song{label}.wav")
        wavio.write_wav(path, _sig(10 + k, n), SR, subtype=subtype)
        stems.append(path)
    p.add_output("stems", stems)
    return p


def _expected(dev, stems, widths, src_path):
    from audiolab_amd import merge, wavio
    src = wavio.read_wav(src_path)[0]
    out, rec = merge.mixdown_array([on(dev, s) if isinstance(s, np.ndarray) else s for s in stems],
                                   (on(dev, src), wavio.read_wav_info(src_path)[2]), src_bits=widths, ctx=dev)
    return host(out), rec


def _samples(path):
    with open(path, "rb") as f:
        data = f.read()
    bits = int.from_bytes(data[34:36], "little")
    ch = int.from_bytes(data[22:24], "little")
    return np.frombuffer(data[44:], dtype="<i2" if bits == 16 else "<i4").reshape(-1, ch).T, bits


def _files(project):
    return sorted(os.path.join(d, f)[len(project.project_dir) + 1:] for d, _, fs in os.walk(project.project_dir) for f in fs)


def test_every_stem_but_the_cloned_voice_is_shifted(dev, project):
    from audiolab_amd import pitch, wavio
    from audiolab_amd.wrappers.merge import Merge
    stems = list(project.last_outputs)
    before = _files(project)
    seen = []
    out = Merge().process_audio([project], callback=lambda frac, desc, total: seen.append((frac, desc, total)), pitch_shift=3)
    merged = os.path.join(project.project_dir, "merged", "song(Merged).wav")
    assert out == [project] and project.last_outputs == [merged]
    assert seen == [(i / 3, f"Processing stem: {os.path.basename(s)}", 3) for i, s in enumerate(stems)]
    assert _files(project) == sorted(before + [os.path.join("merged", "song(Merged).wav")])          # no other file is written
    audio = [wavio.read_wav(s)[0] for s in stems]
    shifted = [pitch.shift_pitch_array(on(dev, a), 3, ctx=dev) for a in audio[:2]]
    assert tuple(shifted[0].shape) == (2, 801) and not np.array_equal(host(shifted[0]), audio[0])
    # shifted stems enter with width 16, the cloned voice unshifted with its file's own
    want, rec = _expected(dev, shifted + [audio[2]], [16, 16, 16], project.src_file)
    got, bits = _samples(merged)
    assert bits == 16 and rec.bits == 16 and got.shape == (2, 801) and np.array_equal(got, want)


def test_width_16_whatever_the_files_width(dev, project):
    """float32 stems alone: unshifted they make a 32-bit mix, shifted a 16-bit one (the reference's ffmpeg call writes pcm_s16le)"""
    from audiolab_amd import pitch, wavio
    from audiolab_amd.wrappers.merge import Merge
    stems = list(project.last_outputs)[:2]
    project.add_output("stems", stems)
    Merge().process_audio([project], pitch_shift=-2)
    got, bits = _samples(project.last_outputs[0])
    audio = [wavio.read_wav(s)[0] for s in stems]
    want, _ = _expected(dev, [pitch.shift_pitch_array(on(dev, a), -2, ctx=dev) for a in audio], [16, 16], project.src_file)
    assert bits == 16 and np.array_equal(got, want)
    project.add_output("stems", stems)
    Merge().process_audio([project])
    assert _samples(project.last_outputs[0])[1] == 32


def test_the_room_goes_back_first_and_its_file_stays_unshifted(dev, project):
    from audiolab_amd import pitch, reverb, wavio
    from audiolab_amd.wrappers.merge import Merge
    ir = np.zeros(40)
    ir[0], ir[7], ir[39] = 1.0, 0.4, -0.2
    with open(os.path.join(project.project_dir, "stems", "impulse_response.ir"), "w") as f:
        json.dump({"sample_rate": SR, "pre_delay": 0.001, "impulse_response": ir.tolist()}, f)
    stems = list(project.last_outputs)[:2]
    project.add_output("stems", stems)
    Merge().process_audio([project], pitch_shift=5)
    rr = os.path.join(project.project_dir, "stems", "song(Vocals)(Re-Reverb).wav")
    audio = [wavio.read_wav(s)[0] for s in stems]
    wet = reverb.apply_reverb_array(on(dev, audio[0]), ir, int(0.001 * SR), ctx=dev)
    assert wavio.read_wav_info(rr) == (2, SR, 16, False)
    wet16 = np.clip(np.rint(host(wet).astype(np.float64) * 32768), -32768, 32767).astype(np.float32) / 32768
    assert np.array_equal(wavio.read_wav(rr)[0], wet16)                                               # the unshifted reverb output
    shifted = [pitch.shift_pitch_array(on(dev, a), 5, ctx=dev) for a in (wet16, audio[1])]
    want, _ = _expected(dev, shifted, [16, 16], project.src_file)
    got, bits = _samples(project.last_outputs[0])
    assert bits == 16 and np.array_equal(got, want)
    assert sorted(f for f in os.listdir(os.path.dirname(rr)) if f.endswith(".wav")) == sorted(
        [os.path.basename(s) for s in stems] + ["song(Vocals)(Cloned).wav", "song(Vocals)(Re-Reverb).wav"])


def test_zero_shift_takes_the_plain_path(dev, project):
    from audiolab_amd.wrappers.merge import Merge
    stems = list(project.last_outputs)
    Merge().process_audio([project], pitch_shift=0)
    with open(project.last_outputs[0], "rb") as f:
        with_kwarg = f.read()
    project.add_output("stems", stems)
    Merge().process_audio([project])
    with open(project.last_outputs[0], "rb") as f:
        assert f.read() == with_kwarg


def test_the_switch_is_off_by_default():
    from audiolab_amd.wrappers.merge import Merge
    assert Merge.pitch_shifter == "error"


def test_the_default_still_refuses(dev, project, monkeypatch):
    from audiolab_amd.wrappers.merge import Merge
    monkeypatch.setattr(Merge, "pitch_shifter", "error")
    seen = []
    with pytest.raises(NotImplementedError):
        Merge().process_audio([project], callback=lambda frac, desc, total: seen.append((frac, desc, total)), pitch_shift=2)
    assert seen == [(1.0, "Error merging audio files.", 1)] and "merged" not in project.output_dict
    # cloned stems alone need no shifter
    cloned = [p for p in project.output_dict["stems"] if "(Cloned)" in p]
    project.add_output("stems", cloned)
    Merge().process_audio([project], pitch_shift=2)
    assert _samples(project.last_outputs[0])[0].shape == (2, 640)


def test_an_unknown_shifter_is_refused(dev, project, monkeypatch):
    from audiolab_amd.wrappers.merge import Merge
    monkeypatch.setattr(Merge, "pitch_shifter", "rubberband")
    for kwargs in ({"pitch_shift": 2}, {}):
        with pytest.raises(ValueError, match="pitch_shifter"):
            Merge().process_audio([project], **kwargs)
