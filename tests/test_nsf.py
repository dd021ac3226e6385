"""The NSF-HiFiGAN vocoder end to end against what the reference's GeneratorNSF computed (tests/golden/nsf.npz): the reduced network stage by
stage at 1e-5 of each stage's peak and its output within 1e-4 absolute, the full v2 40k network's output within 1e-4 absolute -- the
project's float32 PCM bound (the output is tanh-bounded in (-1, 1)).  Every body runs on the CPU emulation and, under ``-m gpu``, on the
MI355X.  The full network runs the fixture's T = 8 on both: 7 GFLOP, about a quarter of a minute on the CPU emulation (every MFMA is a
rendezvous of 64 fibres there), well under the minute that would have called for a shorter entry."""
import dataclasses

import numpy as np
import pytest
import torch

from audiolab_amd import nsf
from audiolab_amd._lib import AlsepError
from tests import nsf_oracle as o
from tests.conftest import host


@pytest.fixture(scope="module")
def golden(golden_dir):
    z = np.load(f"{golden_dir}/nsf.npz")
    assert int(z["seed"]) == o.SEED
    return z


def _inputs(z, tag):
    return z[f"{tag}_x"], z[f"{tag}_f0"], z[f"{tag}_g"], z[f"{tag}_noise"]


def test_reduced_stage_by_stage(dev, golden):
    voc = nsf.NSFVocoder(nsf.synthetic_state_dict(o.REDUCED, o.SEED), o.REDUCED, dev)
    x, f0, g, noise = _inputs(golden, "reduced")
    har = voc.source(f0, noise)
    err = float(np.max(np.abs(host(har) - golden["reduced_har"])))
    print(f"har: max |delta| = {err:.3e}")
    assert err < 1e-5
    h = voc.pre(x, g)
    for i, name in enumerate(["pre", "stage0", "stage1"]):
        if i:
            h = voc.stage(i - 1, h, har)
        want = golden[f"reduced_{name}"].T
        assert tuple(h.shape) == want.shape
        err = float(np.max(np.abs(host(h) - want))) / float(np.max(np.abs(want)))
        print(f"{name}: max |delta| / peak = {err:.3e}")
        assert err < 1e-5
    out = voc.forward(x, f0, g, noise=noise)
    assert tuple(out.shape) == (1, 1, 120) and out.device.type == dev.device.type
    err = float(np.max(np.abs(host(out).reshape(-1) - golden["reduced_out"])))
    print(f"out: max |delta| = {err:.3e}")
    assert err < 1e-4
    assert np.array_equal(host(voc.post(h)), host(out).reshape(-1))


def test_full_network(dev, golden):
    tag = "full"
    voc = nsf.NSFVocoder(nsf.synthetic_state_dict(o.FULL, o.SEED), o.FULL, dev)
    x, f0, g, noise = _inputs(golden, tag)
    out = host(voc.forward(x, f0, g, noise=noise)).reshape(-1)
    want = golden[f"{tag}_out"]
    assert out.shape == want.shape == (x.shape[2] * 400,)
    err = float(np.max(np.abs(out - want)))
    print(f"{tag}: out max |delta| = {err:.3e}")
    assert err < 1e-4


@pytest.fixture()
def small(dev):
    cfg = dataclasses.replace(o.REDUCED, gin_channels=0)
    return cfg, nsf.NSFVocoder(nsf.synthetic_state_dict(cfg, 5), cfg, dev)


def test_no_speaker_conditioning(small):
    cfg, voc = small
    x, f0, g, noise = o.test_inputs(cfg, 9, 2)
    assert g is None
    out = voc.forward(x, f0, None, noise=noise)
    sd = nsf.synthetic_state_dict(cfg, 5)
    want = o.forward(sd, cfg, x, f0, None, noise)[1]
    assert float(np.max(np.abs(host(out).reshape(-1) - want))) < 1e-4
    with pytest.raises(AlsepError, match="gin_channels = 0"):
        voc.forward(x, f0, np.zeros((1, 8, 1), dtype=np.float32), noise=noise)
    with pytest.raises(AlsepError, match="n_res"):
        voc.forward(x, f0, None, torch.tensor(9), noise=noise)
    with pytest.raises(AlsepError, match="batch 1"):
        voc.forward(np.concatenate([x, x]), f0, None, noise=noise)


def test_the_source_reaches_the_output(small):
    cfg, voc = small
    x, f0, _, noise = o.test_inputs(cfg, 9, 2)
    a = host(voc.forward(x, f0, noise=noise))
    f1 = f0.copy()
    assert f1[0, 1] > 0
    f1[0, 1] *= np.float32(1.5)
    b = host(voc.forward(x, f1, noise=noise))
    assert float(np.max(np.abs(a - b))) > 1e-3


def test_same_noise_twice_is_bit_identical(small):
    cfg, voc = small
    x, f0, _, noise = o.test_inputs(cfg, 9, 3)
    assert np.array_equal(host(voc.forward(x, f0, noise=noise)), host(voc.forward(x, f0, noise=noise)))


def test_seeded_generator_draws_the_same_noise(small):
    cfg, voc = small
    x, f0, _, noise = o.test_inputs(cfg, 9, 4)
    a = host(voc.manual_seed(11).forward(x, f0))
    b = host(voc.manual_seed(11).forward(x, f0))
    c = host(voc.manual_seed(12).forward(x, f0))
    assert np.array_equal(a, b)
    assert not np.array_equal(a, c)
    assert not np.array_equal(a, host(voc.forward(x, f0, noise=noise)))
