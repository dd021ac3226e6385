"""audiolab_amd.rmvpe end to end against tests/rmvpe_oracle.py (itself pinned to the reference by tests/test_rmvpe_oracle.py): the reduced
network ``E2E(1, 1, (2, 2), 2, 1, 1, 4)`` on the CPU emulation and on the GPU, the full ``E2E(4, 1, (2, 2))`` on the GPU only, both at 5 280
samples (34 frames, padded to 64), and the public surface of ``RMVPE``.

Bounds: the salience (in (0, 1)) within 1e-4 of the oracle, the project's float32 gate; f0 within 1e-4 relative on every frame where the
oracle's largest salience leads its second largest by more than 1e-3 (below that lead two float32 evaluations may pick different bins);
at most 10 % of the frames may be left out by that rule."""
import numpy as np
import pytest
import torch

from audiolab_amd import rmvpe
from audiolab_amd._lib import AlsepError
from tests import rmvpe_oracle as o
from tests.conftest import host, on

SEED = 3


def _check(model: rmvpe.RMVPE, cfg, full: bool):
    audio = o.test_signal(5280, 0)
    want_hidden = o.network(o.weights(full, SEED), cfg, o.log_mel(audio))
    want_f0 = o.decode(want_hidden, 0.03)
    hidden = host(model.mel2hidden(model.mel_extractor(torch.from_numpy(audio)[None])))[0]
    assert hidden.shape == (34, 360)
    err = float(np.max(np.abs(hidden - want_hidden)))
    f0 = model.infer_from_audio(audio, thred=0.03)
    assert f0.dtype == np.float64 and f0.shape == (5280 // 160 + 1,)
    clear = o.margins(want_hidden) > 1e-3
    rel = np.abs(f0[clear] - want_f0[clear]) / np.maximum(want_f0[clear], 1e-300)
    print(f"full={full}: max |hidden delta| = {err:.3e}, max relative f0 delta = {float(rel.max()):.3e} over {int(clear.sum())} of 34 frames")
    assert err < 1e-4
    assert np.mean(~clear) <= 0.10
    assert np.array_equal(f0[clear] == 0, want_f0[clear] == 0)
    assert float(rel.max()) < 1e-4
    assert np.array_equal(model.decode(hidden, 0.03), f0)                     # the stages compose to infer_from_audio


def test_reduced_network(dev):
    _check(rmvpe.RMVPE(None, ctx=dev, allow_synthetic=True, config=o.REDUCED, seed=SEED), o.REDUCED, False)


@pytest.mark.gpu
def test_full_network(gpu_ctx):
    _check(rmvpe.RMVPE(None, ctx=gpu_ctx, allow_synthetic=True, seed=SEED), o.FULL, True)


@pytest.fixture()
def reduced(dev):
    return rmvpe.RMVPE(None, ctx=dev, allow_synthetic=True, config=o.REDUCED, seed=SEED)


def test_with_pitch_zeroes_outside_the_range(reduced):
    audio = o.test_signal(5280, 0)
    f0 = reduced.infer_from_audio(audio)
    assert np.count_nonzero(f0) > 0
    lo, hi = np.percentile(f0[f0 > 0], [30, 70])
    ranged = reduced.infer_from_audio_with_pitch(audio, thred=0.03, f0_min=lo, f0_max=hi)
    outside = (f0 < lo) | (f0 > hi)
    assert outside.any() and (~outside).any()
    assert np.all(ranged[outside] == 0) and np.array_equal(ranged[~outside], f0[~outside])
    assert np.array_equal(reduced.infer_from_audio(on(reduced.ctx, audio)), f0)                 # a device tensor is taken as well


def test_refusals(dev, tmp_path):
    with pytest.raises(AlsepError, match="not built"):
        rmvpe.RMVPE(None, is_half=True, ctx=dev, allow_synthetic=True, config=o.REDUCED)
    with pytest.raises(AlsepError, match="not built"):
        rmvpe.RMVPE(None, onnx=True, ctx=dev, allow_synthetic=True, config=o.REDUCED)
    with pytest.raises(FileNotFoundError):
        rmvpe.RMVPE(str(tmp_path / "rmvpe.pt"), ctx=dev, config=o.REDUCED)
    with pytest.raises(AlsepError, match="not built"):
        rmvpe.RMVPEConfig(kernel_size=(1, 2)).check()
    with pytest.raises(AlsepError, match="not built"):
        rmvpe.RMVPEConfig(n_gru=0).check()
    model = rmvpe.RMVPE(None, ctx=dev, allow_synthetic=True, config=o.REDUCED)
    with pytest.raises(AlsepError, match="not built"):
        model.mel_extractor(np.zeros(4000, dtype=np.float32), keyshift=2)
    with pytest.raises(AlsepError, match="16 frames need 16 reflected"):
        model.infer_from_audio(np.zeros(15 * 160, dtype=np.float32))
    with pytest.raises(AlsepError, match=str(rmvpe.MAX_FRAMES)):
        model.model.forward(torch.zeros((1, 1)).to(dev.device).expand(rmvpe.MAX_FRAMES + 1, 128))   # a view: no memory behind it


def test_wrong_shape_names_the_tensor(dev, tmp_path):
    sd = dict(o.weights(False, SEED))
    name = "unet.decoder.layers.0.conv1.0.weight"
    sd[name] = sd[name][:, :-1]
    path = tmp_path / "bad.pt"
    torch.save(sd, str(path))
    with pytest.raises(AlsepError, match=name.replace(".", r"\.")):
        rmvpe.RMVPE(str(path), ctx=dev, config=o.REDUCED)
    sd = dict(o.weights(False, SEED))
    del sd["fc.1.bias"]
    torch.save(sd, str(path))
    with pytest.raises(AlsepError, match=r"fc\.1\.bias"):
        rmvpe.RMVPE(str(path), ctx=dev, config=o.REDUCED)


def test_real_format_file_loads_to_the_same_hidden(reduced, tmp_path):
    path = tmp_path / "rmvpe.pt"
    torch.save(o.weights(False, SEED), str(path))
    loaded = rmvpe.RMVPE(str(path), is_half=False, ctx=reduced.ctx, config=o.REDUCED)
    mel = reduced.mel_extractor(o.test_signal(5280, 0))
    assert tuple(mel.shape) == (1, 128, 34)
    assert torch.equal(loaded.mel2hidden(mel), reduced.mel2hidden(mel))
