"""A Reaper project for a list of stems (reference handlers/reaper.py:9-62): ``<project_dir>/export/reaper/<name>/`` with the stems copied to
``Media/`` and ``<name>.rpp`` beside them -- one track per stem, named ``<index + 1>-<stem name>``, holding one item at position 0 whose
length is that of the FIRST stem, on a source that points at ``Media/<file>``; the tempo when one is given.

The reference builds the file with the reathon library; an RPP file is plain text -- nested ``<NAME ...`` / ``>`` chunks of ``KEY value``
lines -- and is written directly here.  Departure: the first stem's length comes from audiolab_amd.wavio, which also reads the float32 WAVs
Separate writes (the reference asks the ``wave`` module, which refuses them)."""
import os
import shutil
from typing import List, Optional

from audiolab_amd import wavio
from audiolab_amd.util.data_classes import ProjectFiles


def _quoted(text: str) -> str:
    """an RPP string: the quote character must not occur inside"""
    for q in ('"', "'", "`"):
        if q not in text:
            return f"{q}{text}{q}"
    return '"' + text.replace('"', "'") + '"'


def rpp_text(names: List[str], files: List[str], length: float, bpm=None) -> str:
    lines = ['<REAPER_PROJECT 0.1 "audiolab_amd"']
    if bpm is not None:
        lines.append(f"  TEMPO {bpm!r} 4 4")
    for name, file in zip(names, files):
        lines += ["  <TRACK", f"    NAME {_quoted(name)}", "    <ITEM", "      POSITION 0.0", f"      LENGTH {length!r}", "      <SOURCE WAVE",
                  f"        FILE {_quoted(file)}", "      >", "    >", "  >"]
    lines.append(">")
    return "\n".join(lines) + "\n"


def create_reaper_project(project: ProjectFiles, stems: List[str], bpm: Optional[float] = None) -> str:
    """-> the project folder"""
    name = os.path.basename(project.project_dir)
    folder = os.path.join(project.project_dir, "export", "reaper", name)
    media = os.path.join(folder, "Media")
    os.makedirs(media, exist_ok=True)
    samples, rate = wavio.read_wav_interleaved(stems[0])
    length = (len(samples) // wavio.read_wav_info(stems[0])[0]) / rate
    names, files = [], []
    for idx, stem in enumerate(stems):
        base = os.path.basename(stem)
        shutil.copy2(stem, os.path.join(media, base))
        names.append(f"{idx + 1}-{os.path.splitext(base)[0]}")
        files.append("Media/" + base)
    with open(os.path.join(folder, f"{name}.rpp"), "w", encoding="utf-8") as f:
        f.write(rpp_text(names, files, length, bpm))
    return folder
