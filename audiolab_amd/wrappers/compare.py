"""``Compare`` -- drop-in for the reference's Process->Compare plugin (wrappers/compare.py): same class attributes (:38-40), no
``allowed_kwargs``, and the same ``process_audio(inputs, callback=None, **kwargs)`` behaviour (:42-166).  Per project the inputs are
``filter_inputs(project, "audio")``; with two or more of them it reports ``callback(0, "Expected exactly 2 unique audio files, got N.", 1)``
and returns ``[]`` from the whole call (:55-59, a quirk that is kept), with none ``inputs[0]`` raises IndexError (:61); the pair compared is
``[project.src_file, inputs[0]]``; the figure goes to ``<project_dir>/comparisons/<base1>_VS_<base2>_<md5[:6]>_<md5[:6]>_comparison.png``
(:25-34); the callback sees ``0 "Starting ..."``, ``1`` and ``2`` per loaded file, ``3 "Calculated differences"`` and ``4 "Saved visualization to
..."``, each with a total of 5 -- the fifth step is never reported (:68-162, kept); ``project.add_output("comparison", path)``.

The arrays -- resampling to 44.1 kHz, RMS normalisation, difference, both spectrograms in decibels -- are computed on the GPU in float64
(audiolab_amd/compare.py, pinned against scipy); the figure is the reference's: ``figsize=(15, 10)``, four panels with its titles, labels,
colours, colormaps, ``shading='auto'`` and ``tight_layout``, drawn with matplotlib's Agg canvas.

Two class attributes that are not kwargs of the reference:
  * ``ctx``: an audiolab_amd._lib.Context to run on (None: the default context of the current device);
  * ``render``: ``"full"`` (the default) plots the full arrays, so the figure is the reference's -- and takes the reference's time, most of it
    matplotlib's (two lines of one point per sample, two meshes of 1025 quads per frame).  ``"reduced"`` plots what the GPU has reduced to
    figure resolution: per curve ``plot_columns`` buckets, each drawn by its two extremum samples in index order at their own x (a min / max
    polyline), and spectrograms of ``spec_columns`` frame buckets holding each bin's maximum, at the time of the bucket's first frame.
    Both column counts are capped by the number of samples / frames.  Any other value raises ValueError.

Departures from the reference: see audiolab_amd/compare.py (float WAV samples as they are, float32 decibel arrays); a file that is not a
WAV goes through ``ensure_wav`` (one ffmpeg transcode to 16-bit stereo at 44.1 kHz) where the reference decodes it with pydub; the REST
endpoint and the self-test of the reference's class (:168-318) are out of scope.
"""
import hashlib
import os
from typing import Any, Dict, List

from audiolab_amd import compare
from audiolab_amd.separator.stem_separator import ensure_wav
from audiolab_amd.util.data_classes import ProjectFiles
from audiolab_amd.wrappers.base_wrapper import BaseWrapper


def compute_file_hash(filepath: str, chunk_size: int = 65536) -> str:
    hasher = hashlib.md5()
    with open(filepath, "rb") as f:
        for data in iter(lambda: f.read(chunk_size), b""):
            hasher.update(data)
    return hasher.hexdigest()


def generate_output_filename(file1: str, file2: str, output_folder: str) -> str:
    """:25-34"""
    tags = [compute_file_hash(f)[:6] for f in (file1, file2)]
    bases = [os.path.splitext(os.path.basename(f))[0] for f in (file1, file2)]
    return os.path.join(output_folder, f"{bases[0]}_VS_{bases[1]}_{tags[0]}_{tags[1]}_comparison.png")


class Compare(BaseWrapper):
    title = "Compare"
    description = "Compare two audio files using time-domain waveforms and spectrogram differences."
    priority = 1000000

    # an audiolab_amd._lib.Context to run on (None: the default context of the current device)
    ctx = None
    # "full": the reference's figure from the full arrays; "reduced": from the GPU's min / max and bucket-max reductions; not a kwarg of the reference
    render = "full"
    plot_columns = 4096
    spec_columns = 2048

    def process_audio(self, inputs: List[ProjectFiles], callback=None, **kwargs: Dict[str, Any]) -> List[ProjectFiles]:
        if self.render not in ("full", "reduced"):
            raise ValueError(f"Compare.render is {self.render!r}; 'full' or 'reduced'")
        pj_outputs = []
        for project in inputs:
            files, _ = self.filter_inputs(project, "audio")
            if len(files) >= 2:                                                                      # :55-59
                if callback is not None:
                    callback(0, f"Expected exactly 2 unique audio files, got {len(files)}.", 1)
                return []
            unique_files = [project.src_file, files[0]]
            output_folder = os.path.join(project.project_dir, "comparisons")
            os.makedirs(output_folder, exist_ok=True)
            output_file = generate_output_filename(unique_files[0], unique_files[1], output_folder)

            total_steps = 5
            current_step = 0
            if callback is not None:
                callback(0, "Starting audio comparison with spectrogram difference", total_steps)
            tracks = []
            for file in unique_files:                                        # read here; both are resampled on the device in compare_arrays
                tracks.append(compare.load_track(ensure_wav(file)))
                current_step += 1
                if callback is not None:
                    callback(current_step, f"Loaded/resampled {os.path.basename(file)}", total_steps)
            result = compare.compare_arrays(tracks[0], tracks[1], ctx=self.ctx)
            current_step += 1
            if callback is not None:
                callback(current_step, "Calculated differences", total_steps)

            self._plot(result, output_file)
            current_step += 1
            if callback is not None:
                callback(current_step, f"Saved visualization to {output_file}", total_steps)
            project.add_output("comparison", output_file)
            pj_outputs.append(project)
        return pj_outputs

    def _plot(self, result: "compare.CompareResult", output_file: str) -> None:
        """:126-158 on an Agg canvas of its own (no pyplot state, nothing left open)"""
        from matplotlib.backends.backend_agg import FigureCanvasAgg
        from matplotlib.figure import Figure
        import numpy as np

        if self.render == "full":
            n = int(result.differences.shape[0])
            xs = np.arange(n)
            curves = [(xs, v.cpu().numpy()) for v in (result.waveforms[0], result.waveforms[1], result.differences)]
            t, spec1_db, diff_db = result.t, result.spec1_db, result.diff_db
        else:
            curves = result.envelopes(self.plot_columns)
            t, spec1_db, diff_db = result.spectra_reduced(self.spec_columns)
        fig = Figure(figsize=(15, 10))
        FigureCanvasAgg(fig)

        ax = fig.add_subplot(4, 1, 1)
        ax.plot(curves[0][0], curves[0][1], label="Track 1 (RMS=1)", alpha=0.6)
        ax.plot(curves[1][0], curves[1][1], label="Track 2 (RMS=1)", alpha=0.6, linestyle="dashed")
        ax.set_title("Waveforms (RMS-Normalized)")
        ax.legend()

        ax = fig.add_subplot(4, 1, 2)
        ax.plot(curves[2][0], curves[2][1], color="red", label="|Track1 - Track2|")
        ax.set_title("Time-Domain Differences")
        ax.legend()

        ax = fig.add_subplot(4, 1, 3)
        ax.set_title("Spectrogram Track 1 (Magnitude)")
        ax.pcolormesh(t, result.f, spec1_db.cpu().numpy(), cmap="viridis", shading="auto")
        ax.set_ylabel("Frequency [Hz]")
        ax.set_xlabel("Time [sec]")

        ax = fig.add_subplot(4, 1, 4)
        ax.set_title("Spectrogram Difference (|Spec1 - Spec2|)")
        ax.pcolormesh(t, result.f, diff_db.cpu().numpy(), cmap="magma", shading="auto")
        ax.set_ylabel("Frequency [Hz]")
        ax.set_xlabel("Time [sec]")

        fig.tight_layout()
        fig.savefig(output_file)
