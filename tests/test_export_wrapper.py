"""``Export.process_audio`` (audiolab_amd/wrappers/export.py; reference wrappers/export.py:151-363) on the emulated kernels (-m "not gpu") and on
the GPU (-m gpu), with a temporary project of ``(Instrumental)`` and ``(Vocals)`` WAVs of a few seconds: the Reaper project (the zip's layout,
the RPP text parsed as balanced chunks, the tempo ``detect_bpm`` finds, one track per stem in order, the item length of the first stem, the
copied media), the recorded outputs, and the paths around it: no stems, a stem that is not a WAV, no tempo source, the Ableton default, an
unreadable instrumental."""
import os
import shlex
import zipfile

import numpy as np
import pytest

from tests import tempo_oracle as o


@pytest.fixture()
def project(tmp_path, monkeypatch, dev):
    """source/song.wav and stems/song(Vocals).wav (2.5 s, mono float32), stems/song(Instrumental).wav (3 s of 120 bpm clicks, stereo 16-bit),
    recorded as the "stems" output in that order"""
    from audiolab_amd import wavio
    from audiolab_amd.handlers import config
    from audiolab_amd.util.data_classes import ProjectFiles
    from audiolab_amd.wrappers.export import Export
    monkeypatch.setattr(config, "output_path", str(tmp_path / "outputs"))
    monkeypatch.setattr(Export, "ctx", dev)
    clicks = o.click_track(120.0, 3.0, 4)
    src = tmp_path / "song.wav"
    wavio.write_wav(str(src), clicks.astype(np.float32), 22050, subtype="PCM_16")
    p = ProjectFiles(str(src))
    stem_dir = os.path.join(p.project_dir, "stems")
    os.makedirs(stem_dir)
    stems = [os.path.join(stem_dir, "song(Vocals).wav"), os.path.join(stem_dir, "song(Instrumental).wav")]
    wavio.write_wav(stems[0], (0.1 * np.random.default_rng(3).standard_normal(int(2.5 * 22050))).astype(np.float32), 22050, subtype="FLOAT")
    wavio.write_wav(stems[1], np.stack([clicks, 0.5 * clicks]).astype(np.float32), 22050, subtype="PCM_16")
    p.add_output("stems", stems)
    return p


def parse_rpp(text):
    """-> the root chunk as (header tokens, [children]); a child is a chunk or a list of tokens.  Raises on unbalanced chunks."""
    root, stack = None, []
    for line in text.splitlines():
        line = line.strip()
        if not line:
            continue
        if line.startswith("<"):
            node = (shlex.split(line[1:]), [])
            if stack:
                stack[-1][1].append(node)
            else:
                assert root is None, "two top-level chunks"
                root = node
            stack.append(node)
        elif line == ">":
            stack.pop()                                                      # IndexError: a closing line too many
        else:
            stack[-1][1].append(shlex.split(line))
    assert root is not None and not stack, "a chunk is left open"
    return root


def chunks(node, name):
    return [c for c in node[1] if isinstance(c, tuple) and c[0][0] == name]


def values(node, key):
    return [c[1:] for c in node[1] if isinstance(c, list) and c[0] == key]


def test_class_attributes():
    from audiolab_amd.wrappers import Export
    assert Export.title == "Export to Ableton Live" and Export.priority == 5
    assert Export.description == "Export stems to an Ableton Live project file (.als)"
    assert list(Export.allowed_kwargs) == ["project_format", "export_all_stems", "export_videos", "pitch_shift"]
    fmt, every, videos, shift = (Export.allowed_kwargs[k] for k in Export.allowed_kwargs)
    assert fmt.type is str and fmt.field.default == "Ableton" and fmt.choices == ["Ableton", "Reaper"] and fmt.gradio_type == "Dropdown"
    assert every.type is bool and every.field.default is True and videos.type is bool and videos.field.default is True
    assert shift.type is int and shift.field.default == 0 and (shift.field.ge, shift.field.le) == (-12, 12) and shift.render is False
    assert Export.ctx is None


def test_reaper_project(dev, project):
    from audiolab_amd import tempo
    from audiolab_amd.wrappers import Export
    stems = list(project.last_outputs)
    name = os.path.basename(project.project_dir)
    seen = []
    out = Export().process_audio([project], callback=lambda *a: seen.append(a), project_format="Reaper", not_a_kwarg=1)
    folder = os.path.join(project.project_dir, "export", "reaper", name)
    zip_path = folder + ".zip"
    assert out == [project] and seen == []
    assert project.output_dict["export"] == [zip_path] and project.last_outputs == stems + [zip_path]
    # the zip: the project folder on top, the .rpp and the media inside
    with zipfile.ZipFile(zip_path) as z:
        names = sorted(z.namelist())
        text = z.read(f"{name}/{name}.rpp").decode("utf-8")
        media = {n: z.read(n) for n in names if "/Media/" in n}
    assert names == sorted([f"{name}/{name}.rpp", f"{name}/Media/song(Vocals).wav", f"{name}/Media/song(Instrumental).wav"])
    for stem in stems:
        with open(stem, "rb") as f:
            data = f.read()
        assert media[f"{name}/Media/{os.path.basename(stem)}"] == data
        with open(os.path.join(folder, "Media", os.path.basename(stem)), "rb") as f:
            assert f.read() == data
    with open(os.path.join(folder, f"{name}.rpp"), encoding="utf-8") as f:
        assert f.read() == text
    # the RPP text
    root = parse_rpp(text)
    assert root[0][0] == "REAPER_PROJECT"
    bpm, beats = tempo.detect_bpm(stems[1], ctx=dev)
    assert bpm == 60.0 * 22050 / (512 * 22) and len(beats) >= 4              # 117.45: the 120 bpm clicks
    assert [float(v[0]) for v in values(root, "TEMPO")] == [bpm]
    tracks = chunks(root, "TRACK")
    assert [values(t, "NAME") for t in tracks] == [[["1-song(Vocals)"]], [["2-song(Instrumental)"]]]
    for track, stem in zip(tracks, stems):
        (item,) = chunks(track, "ITEM")
        assert values(item, "POSITION") == [["0.0"]]
        assert [float(v[0]) for v in values(item, "LENGTH")] == [int(2.5 * 22050) / 22050]      # the FIRST stem's length, in every item
        (source,) = chunks(item, "SOURCE")
        assert source[0] == ["SOURCE", "WAVE"] and values(source, "FILE") == [[f"Media/{os.path.basename(stem)}"]]


def test_last_outputs_only(dev, project):
    """``export_all_stems=False``: the stems are ``last_outputs`` alone"""
    from audiolab_amd.wrappers import Export
    vocals, instrumental = project.last_outputs
    project.add_output("cloned", [instrumental])
    Export().process_audio([project], project_format="Reaper", export_all_stems=False)
    name = os.path.basename(project.project_dir)
    with zipfile.ZipFile(project.output_dict["export"][0]) as z:
        root = parse_rpp(z.read(f"{name}/{name}.rpp").decode("utf-8"))
    assert [values(t, "NAME") for t in chunks(root, "TRACK")] == [[["1-song(Instrumental)"]]]
    assert project.last_outputs == [instrumental, project.output_dict["export"][0]]


def test_no_stems(dev, project):
    from audiolab_amd.wrappers import Export
    for stem in project.last_outputs:
        os.remove(stem)
    seen = []
    assert Export().process_audio([project], callback=lambda *a: seen.append(a), project_format="Reaper") == [project]
    assert seen == [(1.0, "No valid audio stems found for export")] and "export" not in project.output_dict
    assert Export().process_audio([project], project_format="Reaper") == [project]          # and without a callback


def test_a_stem_that_is_not_a_wav_is_ignored_and_the_tempo_defaults(dev, project):
    from audiolab_amd.wrappers import Export
    vocals, instrumental = project.last_outputs
    other = os.path.join(project.project_dir, "stems", "song(Instrumental).flac")
    os.rename(instrumental, other)
    with open(os.path.join(project.project_dir, "stems", "separation.json"), "w") as f:
        f.write("{}")
    project.add_output("stems", [vocals, other])
    Export().process_audio([project], project_format="Reaper")
    name = os.path.basename(project.project_dir)
    with zipfile.ZipFile(project.output_dict["export"][0]) as z:
        assert sorted(z.namelist()) == [f"{name}/Media/song(Vocals).wav", f"{name}/{name}.rpp"]
        root = parse_rpp(z.read(f"{name}/{name}.rpp").decode("utf-8"))
    assert values(root, "TEMPO") == [["120", "4", "4"]] and len(chunks(root, "TRACK")) == 1   # neither (Instrumental) nor (Drums): 120


def test_an_unreadable_instrumental_gives_120(dev, project):
    from audiolab_amd.wrappers import Export
    with open(project.last_outputs[1], "wb") as f:
        f.write(b"RIFF....not a wave file")
    Export().process_audio([project], project_format="Reaper")
    name = os.path.basename(project.project_dir)
    with zipfile.ZipFile(project.output_dict["export"][0]) as z:
        root = parse_rpp(z.read(f"{name}/{name}.rpp").decode("utf-8"))
    assert values(root, "TEMPO") == [["120", "4", "4"]] and len(chunks(root, "TRACK")) == 2


def test_a_drums_stem_is_a_tempo_source(dev, project):
    from audiolab_amd.wrappers import Export
    vocals, instrumental = project.last_outputs
    drums = os.path.join(project.project_dir, "stems", "song(Drums).wav")
    os.rename(instrumental, drums)
    project.add_output("stems", [vocals, drums])
    Export().process_audio([project], project_format="Reaper")
    name = os.path.basename(project.project_dir)
    with zipfile.ZipFile(project.output_dict["export"][0]) as z:
        root = parse_rpp(z.read(f"{name}/{name}.rpp").decode("utf-8"))
    assert [float(v[0]) for v in values(root, "TEMPO")] == [60.0 * 22050 / (512 * 22)]


def test_the_ableton_default_does_not_fail(dev, project):
    from audiolab_amd.wrappers import Export
    stems = list(project.last_outputs)
    seen = []
    assert Export().process_audio([project], callback=lambda *a: seen.append(a)) == [project]
    assert len(seen) == 1 and seen[0][0] == 0.9 and seen[0][1].startswith("Error creating Ableton project: ")
    assert "export" not in project.output_dict and project.last_outputs == stems
    assert Export().process_audio([project]) == [project]                                   # and without a callback
