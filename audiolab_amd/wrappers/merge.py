"""``Merge`` -- drop-in for the reference's Process->Merge plugin (wrappers/merge.py), the last step of the default chain
Separate -> ... -> Merge: same class attributes (:49-52), the same four ``allowed_kwargs`` (:54-84) and the same
``process_audio(pj_inputs, callback=None, **kwargs)`` behaviour (:86-191): unknown kwargs dropped; the stems are
``filter_inputs(project, "audio")`` in that order; a ``(Vocals)`` stem that is not a ``(BG_Vocals`` one gets the stored room back when
``stems/impulse_response.ir`` exists -- the ``...(Re-Reverb).wav`` file is written to ``stems/`` as 16-bit PCM as the reference's
``apply_reverb`` does, and ``src_name`` becomes that stem's name minus ``(Vocals)`` from then on (:115, a quirk that is kept); the output is
``<project_dir>/merged/<src_name><name_str>(Merged).wav`` with ``name_str`` of :137-141 (``selected_voice`` is None when not passed), an
existing file is removed first; ``callback(i / len, "Processing stem: ...", len)`` per stem; on an error it logs, calls
``callback(1.0, "Error merging audio files.", 1)`` and re-raises; ``project.add_output("merged", path)``.

The mixdown itself -- pydub's overlay / normalize / dBFS match / apply_gain in the reference -- runs on the GPU on the integer grid
(audiolab_amd/merge.py); the convolution reverb runs on the GPU too and its result enters the mix from device memory with source width 16.

Departures from the reference:
  * lengths are sample-exact; pydub slices by milliseconds;
  * a non-zero ``pitch_shift`` with a stem that is not a ``(Cloned)`` one raises NotImplementedError before any work while the class
    attribute ``pitch_shifter`` is ``"error"``, the default: the reference shells out to ffmpeg's rubberband filter (util/audio_track.py),
    which is not built.  With ``Merge.pitch_shifter = "vocoder"`` every such stem is shifted on the GPU by the project's own phase-locked
    vocoder (audiolab_amd/pitch.py; parity unpinned: no transient handling, channels shifted independently, not rubberband's quality),
    after the re-reverb step where that applies, and enters the mix from device memory with source width 16 -- the reference's ffmpeg call
    writes pcm_s16le (util/audio_track.py:642, 678); the ``...(Re-Reverb).wav`` file stays the unshifted reverb output, no other file is
    written, ``(Cloned)`` stems pass through untouched (Clone shifted the voice already);
  * a ``src_file`` that is not a WAV goes through ``ensure_wav`` (one ffmpeg transcode) before its loudness is read;
  * stems of differing sample rates -- the default chain's case: Separate writes 44.1 kHz, a cloned voice comes at the model's 40 or
    48 kHz -- raise ValueError while the class attribute ``mixed_rates`` is ``"error"``, the default; with ``Merge.mixed_rates = "ratecv"``
    they are resampled on the GPU with the integer arithmetic of ``audioop.ratecv``, which pydub's overlay runs in the reference, and the
    merged file is written at the largest rate (pydub's control flow around it is restated from its source, unpinned);
  * float samples reach the integer grid by ``clip(rint(x 2^(b-1)))``; the reference's conversion goes through ffmpeg;
  * recombining the merged audio with a video source (:162-185) is out of scope.
"""
import logging
import os
from typing import Any, Dict, List

from audiolab_amd import merge, pitch, reverb, wavio
from audiolab_amd.separator.stem_separator import _call_progress, ensure_wav
from audiolab_amd.util.data_classes import ProjectFiles
from audiolab_amd.wrappers.base_wrapper import BaseWrapper, TypedInput

logger = logging.getLogger(__name__)


class Merge(BaseWrapper):
    title = "Merge"
    description = "Merge multiple audio files into a single track."
    priority = 6
    default = True

    allowed_kwargs = {
        "pitch_shift": TypedInput(
            default=0,
            description="Pitch shift in semitones (+12 for an octave up, -12 for an octave down).",
            type=int,
            gradio_type="Slider",
            ge=-24,
            le=24,
            render=False
        ),
        "prevent_clipping": TypedInput(
            default=True,
            description="Prevent clipping in the output audio by normalizing the final mix.",
            type=bool,
            gradio_type="Checkbox"
        ),
        "selected_voice": TypedInput(
            default="Vocals",
            description="Select the voice to be processed.",
            type=str,
            gradio_type="Text",
            render=False
        ),
        "pitch_extraction_method": TypedInput(
            default="rmvpe+",
            description="Select the pitch extraction method.",
            type=str,
            gradio_type="Text",
            render=False
        ),
    }

    # an audiolab_amd._lib.Context to run on (None: the default context of the current device)
    ctx = None
    # stems of differing sample rates: "error" (ValueError) or "ratecv" (resampled as pydub's overlay does); not a kwarg of the reference
    mixed_rates = "error"
    # a non-zero pitch_shift with stems that are not (Cloned): "error" (NotImplementedError) or "vocoder" (audiolab_amd/pitch.py); not a kwarg
    # of the reference
    pitch_shifter = "error"

    def process_audio(self, pj_inputs: List[ProjectFiles], callback=None, **kwargs: Dict[str, Any]) -> List[ProjectFiles]:
        pj_outputs = []
        filtered_kwargs = {key: value for key, value in kwargs.items() if key in self.allowed_kwargs}      # :89
        pitch_shift = filtered_kwargs.get("pitch_shift", 0)
        selected_voice = filtered_kwargs.get("selected_voice", None)
        pitch_extraction_method = filtered_kwargs.get("pitch_extraction_method", "rmvpe+")
        try:
            for project in pj_inputs:
                logger.info(f"Processing project: {os.path.basename(project.project_dir)}")
                src_name, _ = os.path.splitext(os.path.basename(project.src_file))
                output_folder = os.path.join(project.project_dir, "merged")
                os.makedirs(output_folder, exist_ok=True)
                inputs, _ = self.filter_inputs(project, "audio")
                if self.pitch_shifter not in ("error", "vocoder"):
                    raise ValueError(f"Merge.pitch_shifter is {self.pitch_shifter!r}; 'error' or 'vocoder'")
                if pitch_shift != 0 and self.pitch_shifter == "error" and any("(Cloned)" not in p for p in inputs):   # :125-127
                    raise NotImplementedError("Merge: pitch_shift needs ffmpeg's rubberband filter, which this build does not have "
                                              "(Merge.pitch_shifter = 'vocoder' shifts with the project's own phase vocoder)")
                ir_file = os.path.join(project.project_dir, "stems", "impulse_response.ir")

                new_inputs = []
                for i, stem_path in enumerate(inputs):
                    _call_progress(callback, i / len(inputs), f"Processing stem: {os.path.basename(stem_path)}", len(inputs))
                    logger.info(f"Processing stem: {os.path.basename(stem_path)}")
                    if "(Vocals)" in stem_path and "(BG_Vocals" not in stem_path and os.path.exists(ir_file):  # :110-119
                        logger.info(f"Applying reverb to {os.path.basename(stem_path)}")
                        stem_name, ext = os.path.splitext(os.path.basename(stem_path))
                        src_name = stem_name.replace("(Vocals)", "")
                        reverb_stem_path = os.path.join(project.project_dir, "stems", f"{stem_name}(Re-Reverb){ext}")
                        stem = self._re_reverb(stem_path, ir_file, reverb_stem_path)
                        shift_from = reverb_stem_path                # the reference shifts what it reads back from that file
                    else:
                        stem = shift_from = stem_path
                    if pitch_shift != 0 and "(Cloned)" not in stem_path:                                     # :125-127
                        logger.info(f"Shifting pitch of {os.path.basename(stem_path)} by {pitch_shift} semitones")
                        stem = self._shift(shift_from, pitch_shift)
                    new_inputs.append(stem)

                name_str = ""                                                                                # :137-141
                if selected_voice is not None and selected_voice != "":
                    name_str = f"({selected_voice}_{pitch_extraction_method})"
                if name_str in src_name:
                    name_str = ""
                output_file = os.path.join(output_folder, f"{src_name}{name_str}(Merged).wav")
                if os.path.exists(output_file):
                    os.remove(output_file)

                record = merge.merge_files(new_inputs, ensure_wav(project.src_file), output_file,
                                           prevent_clipping=filtered_kwargs.get("prevent_clipping", True), ctx=self.ctx,
                                           mixed_rates=self.mixed_rates)
                logger.info(f"Merged {len(new_inputs)} stems: {record.as_dict()}")
                project.add_output("merged", output_file)
                pj_outputs.append(project)
        except Exception as e:
            logger.exception("Error merging audio files.")
            _call_progress(callback, 1.0, "Error merging audio files.", 1)
            raise e
        return pj_outputs

    def _re_reverb(self, stem_path: str, ir_file: str, out_path: str):
        """handlers/reverb.py:179-209 on the device: writes ``out_path`` as 16-bit PCM and hands the device signal itself to the mix, with
        source width 16 -- the values the reference reads back from that file"""
        audio, sr = wavio.read_wav(stem_path)
        params = reverb.load_params_from_file(ir_file)
        wet = reverb.apply_reverb_array(audio, params["impulse_response"], int(params["pre_delay"] * sr), reverb.WET_GAIN, ctx=self.ctx)
        wavio.write_wav(out_path, wet.cpu().numpy(), sr, subtype="PCM_16")
        return wet, sr, 16

    def _shift(self, stem_path: str, pitch_shift):
        """util/audio_track.py:603-694 on the device: the shifted stem as a device signal with source width 16, the pcm_s16le the
        reference's ffmpeg call hands back (:642, :678)"""
        audio, sr = wavio.read_wav(stem_path)
        return pitch.shift_pitch_array(audio, pitch_shift, ctx=self.ctx), sr, 16
