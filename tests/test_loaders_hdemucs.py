"""hdemucs_mmi.yaml through the engine: the roster entry with synthetic weights, a demucs package of class ``demucs.hdemucs.HDemucs``
(written here the way demucs.states.save_with_checksum writes one, read by the restricted unpickler), the structural options this build
refuses by name, and ``demucs_precision="f16"`` falling back to float32."""
import dataclasses
import fractions
import logging
import sys
import types

import numpy as np
import pytest
import torch

from tests.conftest import host, on


def _small():
    from audiolab_amd.hdemucs import HDemucsConfig
    return HDemucsConfig(nfft=256, depth=4, channels=16, norm_starts=2, dconv_lstm=2, dconv_attn=2, dconv_mode=3, samplerate=4000,
                         segment_samples=3000)


def _kwargs(cfg, **extra):
    kw = dict(sources=list(cfg.sources), audio_channels=2, channels=cfg.channels, growth=cfg.growth, nfft=cfg.nfft, depth=cfg.depth,
              norm_starts=cfg.norm_starts, dconv_lstm=cfg.dconv_lstm, dconv_attn=cfg.dconv_attn, dconv_mode=cfg.dconv_mode,
              samplerate=cfg.samplerate, segment=fractions.Fraction(cfg.segment_samples, cfg.samplerate), cac=True, hybrid=True,
              rescale=0.1, dconv_init=1e-4, emb_smooth=True)
    kw.update(extra)
    return kw


def _write_th(path, kwargs, sd):
    """a pickled demucs package whose klass is demucs.hdemucs.HDemucs, made with stand-in modules that exist only while it is written"""
    mods = {name: types.ModuleType(name) for name in ("demucs", "demucs.hdemucs")}
    HD = type("HDemucs", (), {"__module__": "demucs.hdemucs"})
    mods["demucs.hdemucs"].HDemucs = HD
    saved = {k: sys.modules.get(k) for k in mods}
    sys.modules.update(mods)
    try:
        torch.save({"klass": HD, "args": (), "kwargs": kwargs, "state": {k: v.half() for k, v in sd.items()}}, path)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


def _package_dir(tmp_path, kwargs, sd):
    _write_th(str(tmp_path / "75fc33f5-1a2b3c4d.th"), kwargs, sd)
    (tmp_path / "hdemucs_mmi.yaml").write_text("models: ['75fc33f5']\n")
    return str(tmp_path)


def test_roster_has_hdemucs_mmi():
    from audiolab_amd.engine import MODEL_ROSTER
    from audiolab_amd.hdemucs import HDemucsConfig
    kind, cfg, opts = MODEL_ROSTER["hdemucs_mmi.yaml"]
    assert kind == "demucs" and isinstance(cfg, HDemucsConfig) and cfg.sources == ("drums", "bass", "other", "vocals")
    assert (cfg.depth, cfg.channels, cfg.nfft, cfg.dconv_comp, cfg.dconv_lstm, cfg.dconv_attn, cfg.segment_samples) == (6, 48, 4096, 4, 4, 4,
                                                                                                                      40 * 44100)
    assert opts == {"shifts": 2, "overlap": 0.25}


def test_synthetic_roster_model_loads(emul, tmp_path):
    from audiolab_amd.engine import Separator
    from audiolab_amd.hdemucs import HDemucs
    sep = Separator(model_file_dir=str(tmp_path), output_dir=str(tmp_path), allow_synthetic=True)
    sep.load_model("hdemucs_mmi.yaml")
    inst = sep.model_instance
    assert isinstance(inst.demucs.net, HDemucs) and inst.weights == "synthetic"


@pytest.mark.gpu
def test_synthetic_roster_model_separates_four_stems(tmp_path):
    from audiolab_amd.engine import Separator
    sep = Separator(model_file_dir=str(tmp_path), output_dir=str(tmp_path), allow_synthetic=True)
    sep.load_model("hdemucs_mmi.yaml")
    mix = torch.randn(2, 3 * 44100, generator=torch.Generator().manual_seed(3)) * 0.2
    out = sep.model_instance.demucs.separate(mix.cuda())
    assert list(out) == ["drums", "bass", "other", "vocals"]
    for v in out.values():
        assert tuple(v.shape) == (2, 3 * 44100) and bool(torch.isfinite(v).all())


def test_package_loads_through_restricted_unpickler(emul, tmp_path):
    from audiolab_amd.engine import Separator
    from audiolab_amd.hdemucs import HDemucs, synthetic_state_dict
    from tests import hdemucs_oracle as ho
    cfg = _small()
    sd = synthetic_state_dict(cfg, seed=3)
    d = _package_dir(tmp_path, _kwargs(cfg), sd)
    assert "demucs" not in sys.modules
    sep = Separator(model_file_dir=d, output_dir=str(tmp_path))
    sep.load_model("hdemucs_mmi.yaml")
    inst = sep.model_instance
    net = inst.demucs.net
    assert isinstance(net, HDemucs) and inst.weights == "real"
    assert net.cfg == cfg
    mix = torch.randn(2, 5000, generator=torch.Generator().manual_seed(1)) * 0.3
    got = host(net.forward(on(emul, mix)))
    want = ho.forward(cfg, {k: v.half().float() for k, v in sd.items()}, mix[None].double())[0].numpy()
    assert float(np.max(np.abs(got - want))) < 1e-4


@pytest.mark.parametrize("opt,value", [("multi_freqs", [4]), ("hybrid", False), ("hybrid_old", True), ("cac", False), ("wiener_iters", 1),
                                       ("channels_time", 32), ("nfreqs", 2), ("not_an_option", 1)])
def test_refused_options_raise_with_their_name(opt, value):
    from audiolab_amd._lib import AlsepError
    from audiolab_amd.th_reader import hdemucs_config_from_kwargs
    with pytest.raises(AlsepError, match=opt):
        hdemucs_config_from_kwargs(_kwargs(_small(), **{opt: value}))


def test_defaults_are_demucs_hdemucs_defaults():
    from audiolab_amd.hdemucs import HDemucsConfig
    from audiolab_amd.th_reader import hdemucs_config_from_kwargs
    cfg = hdemucs_config_from_kwargs({"sources": ["drums", "bass", "other", "vocals"]})
    assert cfg == HDemucsConfig()
    assert hdemucs_config_from_kwargs({"sources": ["a", "b"], "segment": 44, "rescale": 0.2}) == dataclasses.replace(
        HDemucsConfig(), sources=("a", "b"), segment_samples=44 * 44100)


def test_f16_precision_warns_and_runs_float32(emul, tmp_path, caplog):
    from audiolab_amd.engine import Separator
    from audiolab_amd.hdemucs import synthetic_state_dict
    cfg = _small()
    d = _package_dir(tmp_path, _kwargs(cfg), synthetic_state_dict(cfg, seed=4))
    sep = Separator(model_file_dir=d, output_dir=str(tmp_path), demucs_precision="f16")
    with caplog.at_level(logging.WARNING):
        sep.load_model("hdemucs_mmi.yaml")
    assert any("float32" in r.getMessage() and r.levelno == logging.WARNING for r in caplog.records)
    r = sep.model_instance.demucs
    assert r.precision == "f32"
    out = r.separate(torch.randn(2, 4000, generator=torch.Generator().manual_seed(2)) * 0.3)
    assert len(out) == 4 and all(bool(torch.isfinite(v).all()) for v in out.values())
