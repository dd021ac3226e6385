"""HDemucs (audiolab_amd/hdemucs.py) against the torch restatement (tests/hdemucs_oracle.py, float64).

A small configuration on the CPU emulation and the GPU (``dev``): nfft 256, depth 4, channels 16, norm_starts 2, BLSTM and LocalState from
layer 2 -- layer 2 is the last frequency layer (kernel = freqs, an empty time-branch partner), layer 3 is 1-D on the merged branch.  On the
GPU also the full-size default network (hdemucs_mmi's structure) on 10 s and a 60 s track through DemucsRunner."""
import numpy as np
import pytest
import torch

from tests.conftest import host, on
from tests import hdemucs_oracle as ho


def _small(mode: int):
    from audiolab_amd.hdemucs import HDemucsConfig
    return HDemucsConfig(nfft=256, depth=4, channels=16, norm_starts=2, dconv_lstm=2, dconv_attn=2, dconv_mode=mode, samplerate=4000,
                         segment_samples=3000)


def _mix(L: int, seed: int = 1, B: int = 0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*((B,) if B else ()), 2, L, generator=g) * 0.3


@pytest.mark.parametrize("mode", [1, 3])
@pytest.mark.parametrize("L", [4000, 20000, 100])
def test_small_matches_oracle(dev, mode, L):
    """one segment (4000 samples: T 63 at the BLSTM layers), a long input (20000: T 313 and 157 -- framing at layer 2) and a short one
    (100 samples: shorter than the STFT's reflection padding)"""
    from audiolab_amd.hdemucs import HDemucs, synthetic_state_dict
    cfg = _small(mode)
    sd = synthetic_state_dict(cfg, seed=mode)
    net = HDemucs(cfg, sd, ctx=dev)
    mix = _mix(L)
    got = host(net.forward(on(dev, mix)))
    want = ho.forward(cfg, sd, mix[None].double())[0].numpy()
    assert got.shape == (cfg.S, 2, L)
    err = float(np.max(np.abs(got - want)))
    assert err < 1e-4, f"dconv_mode {mode}, L {L}: max |delta| = {err:.3e} (peak {np.max(np.abs(want)):.3f})"


@pytest.mark.parametrize("B", [1, 3])
def test_small_batch_bit_identical(dev, B):
    from audiolab_amd.hdemucs import HDemucs, synthetic_state_dict
    cfg = _small(3)
    net = HDemucs(cfg, synthetic_state_dict(cfg, seed=2), ctx=dev)
    mixes = _mix(13000, seed=4, B=B)
    batch = host(net.forward(on(dev, mixes)))
    assert batch.shape == (B, cfg.S, 2, 13000)
    for b in range(B):
        alone = host(net.forward(on(dev, mixes[b].contiguous())))
        assert np.array_equal(batch[b], alone), f"sample {b} of a batch of {B} differs from that sample run alone"


def test_small_runner_matches_apply_model(dev):
    """DemucsRunner (shifts 2, overlap 0.25, unpadded chunks in batches) against the oracle's apply_model restatement"""
    from audiolab_amd.hdemucs import HDemucs, synthetic_state_dict
    from audiolab_amd.htdemucs import DemucsRunner
    cfg = _small(1)
    sd = synthetic_state_dict(cfg, seed=0)
    mix = _mix(9000, seed=2)
    r = DemucsRunner(HDemucs(cfg, sd, ctx=dev), shifts=2, overlap=0.25, batch=3)
    out = r.separate(on(dev, mix))
    got = np.stack([host(out[s]) for s in cfg.sources])
    want = ho.separate(cfg, sd, mix.double(), shifts=2, overlap=0.25).numpy()
    err = float(np.max(np.abs(got - want)))
    assert err < 1e-4, f"runner: max |delta| = {err:.3e}"
    assert r.batches_run < len(r.units(9000)[0]), "units of equal length run batched"


def test_shape_check_names_the_hyper_parameter():
    import dataclasses
    from audiolab_amd._lib import AlsepError
    from audiolab_amd.hdemucs import HDemucs, synthetic_state_dict
    cfg = _small(1)
    sd = synthetic_state_dict(cfg)
    with pytest.raises(AlsepError, match="dconv_comp"):
        HDemucs(dataclasses.replace(cfg, dconv_comp=2), sd, ctx=_CpuStub())
    with pytest.raises(AlsepError, match="norm_groups"):
        HDemucs(dataclasses.replace(cfg, norm_groups=3), sd, ctx=_CpuStub())


class _CpuStub:
    """a context stand-in for construction errors raised before any device work"""
    device = torch.device("cpu")


def test_expected_shapes_use_demucs_names():
    from audiolab_amd.hdemucs import HDemucsConfig, expected_shapes
    exp = expected_shapes(HDemucsConfig())
    assert exp["encoder.4.dconv.layers.0.3.lstm.weight_ih_l0"][0] == (768, 192)
    assert exp["encoder.5.dconv.layers.1.3.lstm.weight_hh_l1_reverse"][0] == (1536, 384)
    assert exp["encoder.4.dconv.layers.0.3.linear.weight"][0] == (192, 384)
    assert exp["encoder.4.dconv.layers.0.4.query_decay.weight"][0] == (16, 192, 1)
    assert exp["encoder.4.dconv.layers.0.8.scale"][0] == (768,)
    assert exp["encoder.4.conv.weight"][0] == (768, 384, 8, 1)
    assert exp["tencoder.4.conv.weight"][0] == (768, 384, 8)
    assert "tencoder.4.rewrite.weight" not in exp and "tencoder.5.conv.weight" not in exp
    assert exp["encoder.5.conv.weight"][0] == (1536, 768, 4)
    assert exp["tdecoder.0.conv_tr.weight"][0] == (768, 384, 8) and exp["tdecoder.0.norm2.weight"][0] == (384,)
    assert exp["decoder.0.conv_tr.weight"][0] == (1536, 768, 4)
    assert exp["decoder.5.conv_tr.weight"][0] == (48, 16, 8, 1)
    assert exp["encoder.4.norm1.weight"][0] == (768,) and "encoder.3.norm1.weight" not in exp
    assert "decoder.0.dconv.layers.0.0.weight" not in exp                         # dconv_mode 1: encoder only


# ---- the full-size default network (hdemucs_mmi's structure), GPU only ------------------------------------------------------------------
_FULL = {}


def _full():
    if not _FULL:
        from audiolab_amd.hdemucs import HDemucsConfig, synthetic_state_dict
        cfg = HDemucsConfig()
        _FULL["cfg"], _FULL["sd"] = cfg, synthetic_state_dict(cfg, seed=11)
    return _FULL["cfg"], _FULL["sd"]


@pytest.mark.gpu
def test_full_size_10s_matches_oracle(gpu_ctx):
    """10 s: T 431 at layer 4 and 216 at layer 5, framing at both BLSTMs"""
    from audiolab_amd.hdemucs import HDemucs
    cfg, sd = _full()
    net = HDemucs(cfg, sd, ctx=gpu_ctx)
    mix = _mix(441000, seed=5)
    got = host(net.forward(on(gpu_ctx, mix)))
    with torch.no_grad():
        torch.set_num_threads(min(16, torch.get_num_threads()))
        want = ho.forward(cfg, sd, mix[None].double())[0].numpy()
    err = float(np.max(np.abs(got - want)))
    assert err < 1e-4, f"full-size HDemucs, 10 s: max |delta| = {err:.3e} (peak {np.max(np.abs(want)):.3f})"


@pytest.mark.gpu
def test_full_size_runner_60s_matches_apply_model(gpu_ctx):
    from audiolab_amd.hdemucs import HDemucs
    from audiolab_amd.htdemucs import DemucsRunner
    cfg, sd = _full()
    mix = _mix(60 * 44100, seed=6)
    r = DemucsRunner(HDemucs(cfg, sd, ctx=gpu_ctx), shifts=2, overlap=0.25)
    out = r.separate(on(gpu_ctx, mix))
    got = np.stack([host(out[s]) for s in cfg.sources])
    torch.set_num_threads(min(16, torch.get_num_threads()))
    want = ho.separate(cfg, sd, mix.double(), shifts=2, overlap=0.25).numpy()
    err = float(np.max(np.abs(got - want)))
    assert err < 1e-4, f"full-size HDemucs through DemucsRunner, 60 s: max |delta| = {err:.3e} (peak {np.max(np.abs(want)):.3f})"
