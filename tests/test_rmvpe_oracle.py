"""CPU only: tests/rmvpe_oracle.py pinned to what the reference's own RMVPE code computed (tests/golden/rmvpe.npz, written by
scripts/make_golden_rmvpe.py), the mel filterbank pinned to its closed form (parity unpinned: librosa is not available), and the seeded
synthetic weights checked for a network that is not degenerate: the end-to-end tests compare f0 only where the salience has a clear peak,
so the draw itself has to leave most frames with one."""
import numpy as np
import pytest
import torch

from audiolab_amd import rmvpe
from tests import rmvpe_oracle as o

SEED = 3                                                                     # the seed of the golden file and of the end-to-end tests


@pytest.fixture(scope="module")
def golden(golden_dir):
    z = np.load(f"{golden_dir}/rmvpe.npz")
    assert int(z["seed"]) == SEED
    return z


def test_signal_is_the_goldens(golden):
    assert np.array_equal(o.test_signal(5280, 0), golden["audio"])


def test_mel_matches_the_reference(golden):
    lin, want = o.mel_linear(golden["audio"]), np.exp(golden["mel"].astype(np.float64))
    assert lin.shape == (128, 34)
    assert float(np.max(np.abs(lin - want))) < 1e-5 * float(want.max())       # where neither is clamped the exponential undoes the log
    got = o.log_mel(golden["audio"])
    sel = want > 1e-4
    assert np.all(np.abs(got[sel] - golden["mel"][sel]) <= 1e-5 * want.max() / want[sel] + 2e-5)


@pytest.mark.parametrize("tag", ["reduced", "full"])
def test_hidden_and_f0_match_the_reference(golden, tag):
    cfg = o.FULL if tag == "full" else o.REDUCED
    hidden = o.network(o.weights(tag == "full", SEED), cfg, golden["mel"])
    want = golden[f"hidden_{tag}"]
    assert hidden.shape == want.shape == (34, 360)
    assert float(np.max(np.abs(hidden - want))) < 1e-5 * float(np.max(np.abs(want)))
    f0, f0_want = o.decode(want, 0.03), golden[f"f0_{tag}"]
    assert np.array_equal(f0 == 0, f0_want == 0)
    assert float(np.max(np.abs(f0 - f0_want) / np.maximum(f0_want, 1e-300))) < 1e-9
    ranged = f0.copy()
    ranged[(ranged < 50) | (ranged > 1100)] = 0
    assert np.allclose(ranged, golden[f"f0_pitch_{tag}"], rtol=1e-9, atol=0)


@pytest.mark.parametrize("full", [False, True])
def test_synthetic_network_is_not_degenerate(golden, full):
    cfg = o.FULL if full else o.REDUCED
    trace = []
    sal = o.network(o.weights(full, SEED), cfg, golden["mel"], trace)
    spread = sal.max(axis=1) - sal.min(axis=1)
    assert float(spread.min()) > 0.05
    rms = [float(torch.sqrt(torch.mean(a * a))) for _, a in trace]
    assert len(rms) == (2 * cfg.en_de_layers + cfg.inter_layers) * cfg.n_blocks + cfg.en_de_layers
    assert 1e-2 <= min(rms) and max(rms) <= 1e2
    under = float(np.mean(o.margins(sal) <= 1e-3))
    print(f"full={full}: activation RMS {min(rms):.3g} .. {max(rms):.3g}, {100 * under:.1f}% of frames under the margin")
    assert under <= 0.10


def test_filterbank_closed_form():
    fb = rmvpe.mel_filterbank_htk().astype(np.float64)
    assert fb.shape == (128, 513) and rmvpe.mel_filterbank_htk().dtype == np.float32
    f = rmvpe.mel_points_htk()
    mel = 2595.0 * np.log10(1.0 + f / 700.0)
    assert abs(f[0] - 30.0) < 1e-9 and abs(f[-1] - 8000.0) < 1e-6
    assert np.allclose(np.diff(mel), (mel[-1] - mel[0]) / 129, rtol=1e-12)    # the corners are equally spaced on the HTK scale
    freqs = np.arange(513) * (16000.0 / 1024)
    for m in range(128):
        inside = (freqs > f[m]) & (freqs < f[m + 2])
        assert np.all(fb[m][~inside] == 0)                                    # zero at and beyond the corners
        height = 2.0 / (f[m + 2] - f[m])
        tri = np.where(freqs <= f[m + 1], (freqs - f[m]) / (f[m + 1] - f[m]), (f[m + 2] - freqs) / (f[m + 2] - f[m + 1]))
        assert np.allclose(fb[m][inside], (height * tri)[inside], rtol=1e-6, atol=0)
        assert fb[m].max() <= height * (1 + 1e-6)                             # the peak 2 / (f[m+2] - f[m]), scaled by the triangle at the bin
        if inside.any():
            k = int(np.argmax(fb[m]))
            assert abs(fb[m][k] - height * tri[k]) <= 1e-6 * height


def test_state_dict_layout():
    shapes = rmvpe.param_shapes()
    assert len([k for k in shapes if k.endswith("conv.0.weight")]) == 56      # residual blocks of E2E(4, 1, (2, 2))
    assert shapes["unet.intermediate.layers.0.conv.0.conv.0.weight"] == (512, 256, 3, 3)
    assert shapes["unet.decoder.layers.0.conv1.0.weight"] == (512, 256, 3, 3)
    assert shapes["unet.decoder.layers.4.conv2.0.shortcut.weight"] == (16, 32, 1, 1)
    assert shapes["fc.0.gru.weight_ih_l0_reverse"] == (768, 384) and shapes["fc.1.weight"] == (360, 512)
    a, b = rmvpe.synthetic_state_dict(o.REDUCED, 5), rmvpe.synthetic_state_dict(o.REDUCED, 5)
    assert all(torch.equal(a[k], b[k]) for k in a)
