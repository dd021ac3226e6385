"""``Export`` -- drop-in for the reference's Process->Export plugin (wrappers/export.py): same class attributes and the same four
``allowed_kwargs`` (:151-183), and the same ``process_audio(inputs, callback=None, **kwargs)`` behaviour (:185-363): unknown kwargs dropped; the
stems are ``last_outputs`` or, with ``export_all_stems`` (the default), ``all_outputs()`` plus the files of ``stems/`` that are not ``.json``;
only existing ``.wav`` files are used; without any, ``callback(1.0, "No valid audio stems found for export")`` and the inputs come back; the
tempo is 120 unless the FIRST stem whose path contains ``(Instrumental)`` or ``(Drums)`` yields a bpm above 0; the project is written, zipped
with its folder as the top-level entry, recorded with ``add_output("export", zip)`` and appended to what ``last_outputs`` was; a failure to
write the project is logged, reported as ``callback(0.9, ...)`` and does not stop the call; any other exception is reported as
``callback(1, "Error exporting to project")`` and raised again.

The tempo comes from audiolab_amd.tempo.detect_bpm, which runs on the GPU (csrc/tempo.h) where the reference calls librosa.

A class attribute that is not a kwarg of the reference: ``ctx``, an audiolab_amd._lib.Context to run on (None: the default context of the
current device).

Departures from the reference:
  * ``project_format="Ableton"``, the default, needs the reference's template set and is not built: project creation raises
    NotImplementedError, which takes the path above (logged, ``callback(0.9, ...)``, no zip, no ``"export"`` output);
  * the Reaper project is written as RPP text directly (audiolab_amd/handlers/reaper.py), not through reathon;
  * recombining audio with video sources (:240-301) is out of scope, as in Merge: video sources are logged and skipped;
  * ``pitch_shift`` is accepted and, like the reference's Reaper path, not used."""
import logging
import os
import zipfile
from typing import Any, Dict, List

from audiolab_amd import tempo
from audiolab_amd.handlers.reaper import create_reaper_project
from audiolab_amd.util.data_classes import ProjectFiles
from audiolab_amd.wrappers.base_wrapper import BaseWrapper, TypedInput

logger = logging.getLogger(__name__)


def create_ableton_project(project: ProjectFiles, stems: List[str], bpm, pitch_shift=0):
    raise NotImplementedError("Export: an Ableton Live set needs the reference's template set, which this build does not have "
                              "(project_format='Reaper' is built)")


def zip_folder(folder_path: str) -> str:
    """``<folder>.zip`` beside the folder, with the folder itself as the archive's top-level entry"""
    top = os.path.basename(folder_path)
    out_zip = os.path.join(os.path.dirname(folder_path), f"{top}.zip")
    with zipfile.ZipFile(out_zip, "w", zipfile.ZIP_DEFLATED) as z:
        for root, _, files in os.walk(folder_path):
            for name in sorted(files):
                path = os.path.join(root, name)
                z.write(path, os.path.join(top, os.path.relpath(path, start=folder_path)))
    return out_zip


class Export(BaseWrapper):
    title = "Export to Ableton Live"
    description = "Export stems to an Ableton Live project file (.als)"
    priority = 5
    allowed_kwargs = {
        "project_format": TypedInput(
            default="Ableton",
            description="Project format to export.",
            choices=["Ableton", "Reaper"],
            gradio_type="Dropdown",
            type=str,
        ),
        "export_all_stems": TypedInput(
            default=True,
            description="Export all stems, including non-cloned vocals, etc.",
            type=bool,
            gradio_type="Checkbox",
        ),
        "export_videos": TypedInput(
            default=True,
            description="Reconstruct videos with processed audio.",
            type=bool,
            gradio_type="Checkbox",
        ),
        "pitch_shift": TypedInput(
            default=0,
            description="Pitch shift in semitones.",
            type=int,
            gradio_type="Slider",
            ge=-12,
            le=12,
            render=False
        ),
    }

    # an audiolab_amd._lib.Context to run on (None: the default context of the current device); not a kwarg of the reference
    ctx = None

    def process_audio(self, inputs: List[ProjectFiles], callback=None, **kwargs: Dict[str, Any]) -> List[ProjectFiles]:
        filtered_kwargs = {key: value for key, value in kwargs.items() if key in self.allowed_kwargs}
        project_format = filtered_kwargs.get("project_format", "Ableton")
        export_all_stems = filtered_kwargs.get("export_all_stems", True)
        export_videos = filtered_kwargs.get("export_videos", True)
        pitch_shift = filtered_kwargs.get("pitch_shift", 0)
        try:
            for project in inputs:
                stems = project.last_outputs
                if export_videos and getattr(project, "video_sources", None):
                    logger.warning(f"Export: {len(project.video_sources)} video sources are skipped (video recombination is not built)")
                if export_all_stems:
                    stems = project.all_outputs()
                    stems_dir = os.path.join(project.project_dir, "stems")
                    if os.path.exists(stems_dir):
                        for name in os.listdir(stems_dir):
                            path = os.path.join(stems_dir, name)
                            if os.path.isfile(path) and not name.endswith(".json") and path not in stems:
                                stems.append(path)
                    else:
                        logger.warning(f"Stems directory not found: {stems_dir}")

                existing = []
                for stem in stems:
                    if not os.path.exists(stem):
                        logger.error(f"Stem file not found: {stem}")
                    elif not stem.endswith(".wav"):
                        logger.warning(f"Ignoring non-WAV file: {stem}")
                    else:
                        existing.append(stem)
                if not existing:
                    logger.warning("No valid audio stems found for export")
                    if callback:
                        callback(1.0, "No valid audio stems found for export")
                    return inputs
                stems = existing

                bpm = 120
                for stem in stems:
                    if "(Instrumental)" in stem or "(Drums)" in stem:
                        found, _ = tempo.detect_bpm(stem, ctx=self.ctx)
                        if found > 0:
                            logger.info(f"Detected BPM: {found}")
                            bpm = found
                        break

                out_zip = None
                try:
                    if project_format == "Ableton":
                        out_zip = zip_folder(create_ableton_project(project, stems, bpm, pitch_shift))
                    elif project_format == "Reaper":
                        out_zip = zip_folder(create_reaper_project(project, stems, bpm))
                    if out_zip:
                        logger.info(f"Saved {project_format} project to: {out_zip}")
                except Exception as e:
                    logger.error(f"Error creating {project_format} project: {e}")
                    if callback:
                        callback(0.9, f"Error creating {project_format} project: {str(e)}")

                last_outputs = project.last_outputs
                if out_zip:
                    project.add_output("export", out_zip)
                    last_outputs.append(out_zip)
                project.last_outputs = last_outputs
        except Exception as e:
            logger.error(f"Error exporting to project: {e}")
            if callback is not None:
                callback(1, "Error exporting to project")
            raise e
        return inputs
