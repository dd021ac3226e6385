"""Writes tests/golden/rmvpe.npz: what the reference's own RMVPE code computes for a short seeded signal, to pin tests/rmvpe_oracle.py.

    python scripts/make_golden_rmvpe.py --reference /path/to/the/reference/tree

The reference module (modules/rvc/infer/lib/rmvpe.py) is imported at run time.  Its librosa imports are stubbed, because librosa is not
available: ``librosa.util`` with a ``pad_center`` (``tiny`` and ``normalize`` are only used by the inverse transform), ``librosa.filters.mel``
with the project's ``mel_filterbank_htk`` -- so the filterbank itself stays parity unpinned, everything downstream of it is the
reference's arithmetic.  The object is made with ``object.__new__(RMVPE)`` and given the network with the project's seeded synthetic
weights (``load_state_dict`` is strict, which also pins the state dict's names and shapes), once for the reduced network
``E2E(1, 1, (2, 2), 2, 1, 1, 4)`` and once for the full ``E2E(4, 1, (2, 2))``.
"""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from audiolab_amd import rmvpe as product  # noqa: E402
import rmvpe_oracle as oracle  # noqa: E402


def load_reference(tree: str):
    def pad_center(data, size, axis=-1, **kw):
        n = data.shape[axis]
        lpad = (size - n) // 2
        widths = [(0, 0)] * data.ndim
        widths[axis] = (lpad, size - n - lpad)
        return np.pad(data, widths, **kw)

    def mel(sr, n_fft, n_mels, fmin, fmax, htk):
        assert htk
        return product.mel_filterbank_htk(int(sr), int(n_fft), int(n_mels), float(fmin), float(fmax))

    librosa = types.ModuleType("librosa")
    librosa.util = types.ModuleType("librosa.util")
    librosa.util.pad_center, librosa.util.tiny, librosa.util.normalize = pad_center, None, None
    librosa.filters = types.ModuleType("librosa.filters")
    librosa.filters.mel = mel
    sys.modules.update({"librosa": librosa, "librosa.util": librosa.util, "librosa.filters": librosa.filters})
    spec = importlib.util.spec_from_file_location("reference_rmvpe", os.path.join(tree, "modules", "rvc", "infer", "lib", "rmvpe.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def make_object(ref, args, cfg, seed):
    obj = object.__new__(ref.RMVPE)
    obj.resample_kernel, obj.is_half, obj.onnx, obj.device = {}, False, False, "cpu"
    obj.mel_extractor = ref.MelSpectrogram(False, 128, 16000, 1024, 160, None, 30, 8000)
    model = ref.E2E(*args)
    model.load_state_dict(product.synthetic_state_dict(cfg, seed))
    obj.model = model.eval()
    obj.cents_mapping = np.pad(20 * np.arange(360) + 1997.3794084376191, (4, 4))
    return obj


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "rmvpe.npz"))
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    ref = load_reference(a.reference)
    audio = oracle.test_signal(5280, 0)
    out = {"audio": audio, "seed": np.int64(a.seed)}
    for tag, args, cfg in (("reduced", (1, 1, (2, 2), 2, 1, 1, 4), oracle.REDUCED), ("full", (4, 1, (2, 2)), oracle.FULL)):
        obj = make_object(ref, args, cfg, a.seed)
        with torch.no_grad():
            mel = obj.mel_extractor(torch.from_numpy(audio).float().unsqueeze(0), center=True)
            hidden = obj.mel2hidden(mel).squeeze(0).numpy()
        out["mel"] = mel[0].numpy()
        out[f"hidden_{tag}"] = hidden
        out[f"f0_{tag}"] = obj.decode(hidden.copy(), thred=0.03)
        out[f"f0_pitch_{tag}"] = obj.infer_from_audio_with_pitch(audio, thred=0.03)
        obj.model = None                                                     # the reference's __del__ moves a live model
    np.savez_compressed(a.out, **out)
    print({k: (v.shape, str(v.dtype)) for k, v in out.items()}, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
