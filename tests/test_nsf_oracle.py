"""CPU only: tests/nsf_oracle.py pinned to what the reference's own GeneratorNSF computed (tests/golden/nsf.npz, written by
scripts/make_golden_nsf.py), the weight-norm fold against torch._weight_norm, the state-dict and configuration checks, and the checkpoint
loader.

What scripts/make_golden_nsf.py printed when the fixture was written (seed 0; the reference in float32 against itself in float64):

    reduced: T = 20,  120 samples; max |f32 - f64| of out = 7.019e-07, of har = 3.855e-08; rms har 0.067, pre 0.976, stage 0 1.171,
             stage 1 1.130, in front of tanh 0.675, out 0.480; max |out - out with a silent source| = 5.854e-01
    full:    T = 8,  3200 samples; max |f32 - f64| of out = 2.139e-06, of har = 2.324e-07; rms har 0.064, pre 0.925, stage 0 1.039,
             stage 1 1.114, stage 2 1.202, stage 3 1.378, in front of tanh 0.559, out 0.445; silent source 9.044e-01

All below the 1e-5 the draw has to keep; every stage O(1); the source reaches the output."""
import numpy as np
import pytest
import torch

from audiolab_amd import nsf
from audiolab_amd._lib import AlsepError
from tests import nsf_oracle as o


@pytest.fixture(scope="module")
def golden(golden_dir):
    z = np.load(f"{golden_dir}/nsf.npz")
    assert int(z["seed"]) == o.SEED
    return z


@pytest.fixture(scope="module")
def oracle_runs(golden):
    """the oracle on the fixture's inputs, once for all tests of this module"""
    runs = {}
    for tag, cfg in (("reduced", o.REDUCED), ("full", o.FULL)):
        sd = nsf.synthetic_state_dict(cfg, o.SEED)
        runs[tag] = o.forward(sd, cfg, golden[f"{tag}_x"], golden[f"{tag}_f0"], golden[f"{tag}_g"], golden[f"{tag}_noise"])
    return runs


@pytest.mark.parametrize("tag,T", [("reduced", 20), ("full", 8)])
def test_inputs_are_the_goldens(golden, tag, T):
    cfg = o.REDUCED if tag == "reduced" else o.FULL
    x, f0, g, noise = o.test_inputs(cfg, T, o.SEED)
    for name, v in (("x", x), ("f0", f0), ("g", g), ("noise", noise)):
        assert np.array_equal(v, golden[f"{tag}_{name}"])
    f = f0.reshape(-1)
    assert f[-1] > 0 and np.any(f == 0) and f[0] > 0                          # voiced, an unvoiced stretch inside, a voiced frame last


@pytest.mark.parametrize("tag", ["reduced", "full"])
def test_har_matches_the_reference(golden, oracle_runs, tag):
    har = oracle_runs[tag][0]
    err = float(np.max(np.abs(har - golden[f"{tag}_har"])))
    print(f"{tag}: har max |delta| = {err:.3e}")
    assert err < 1e-5


def test_stages_match_the_reference(golden, oracle_runs):
    keep = oracle_runs["reduced"][2]
    names = ["pre", "stage0", "stage1"]
    assert len(keep) == len(names)
    for name, got in zip(names, keep):
        want = golden[f"reduced_{name}"]
        assert got.shape == want.shape
        err = float(np.max(np.abs(got - want))) / float(np.max(np.abs(want)))
        print(f"reduced {name}: max |delta| / peak = {err:.3e}")
        assert err < 1e-5


@pytest.mark.parametrize("tag", ["reduced", "full"])
def test_out_matches_the_reference(golden, oracle_runs, tag):
    out = oracle_runs[tag][1]
    err = float(np.max(np.abs(out - golden[f"{tag}_out"])))
    print(f"{tag}: out max |delta| = {err:.3e}")
    assert err < 1e-5


def test_the_draw_is_not_degenerate(oracle_runs):
    har, out, keep = oracle_runs["full"]
    for s in keep:
        assert 0.3 < o.rms(s) < 3.0
    assert 0.2 < o.rms(np.arctanh(np.clip(out, -1 + 1e-12, 1 - 1e-12))) < 1.0
    assert 0.03 < o.rms(har) < 0.2


@pytest.mark.parametrize("kind", ["conv", "tconv"])
def test_weight_norm_fold_matches_torch(kind):
    g = torch.Generator().manual_seed(4)
    v = torch.randn((24, 16, 7) if kind == "conv" else (32, 16, 10), generator=g)
    gg = torch.rand((v.shape[0], 1, 1), generator=g) + 0.5
    want = torch._weight_norm(v.double(), gg.double(), 0)
    got = nsf.fold_weight_norm(gg, v)
    assert got.dtype == torch.float32
    assert torch.equal(got, want.float())                                    # float64, rounded once
    assert float((got - torch._weight_norm(v, gg, 0)).abs().max()) < 1e-6
    # the module's own parametrisation, the norm over every axis but the first: Cout for a Conv1d, Cin for a ConvTranspose1d
    m = torch.nn.utils.weight_norm(torch.nn.Conv1d(16, 24, 7) if kind == "conv" else torch.nn.ConvTranspose1d(32, 16, 10))
    assert tuple(m.weight_g.shape) == (v.shape[0], 1, 1)
    assert float((nsf.fold_weight_norm(m.weight_g.detach(), m.weight_v.detach()) - m.weight.detach()).abs().max()) < 1e-6


def test_state_dict_names_the_first_bad_tensor():
    cfg = o.REDUCED
    sd = nsf.synthetic_state_dict(cfg, 1)
    nsf.check_state_dict(sd, cfg)
    assert tuple(sd["ups.0.weight_g"].shape) == (32, 1, 1) and tuple(sd["resblocks.0.convs1.0.weight_g"].shape) == (16, 1, 1)
    bad = dict(sd)
    bad["ups.1.weight_v"] = torch.zeros(16, 8, 5)
    with pytest.raises(AlsepError, match=r"ups\.1\.weight_v has shape \(16, 8, 5\)"):
        nsf.check_state_dict(bad, cfg)
    bad = {k: v for k, v in sd.items() if k != "noise_convs.0.bias"}
    with pytest.raises(AlsepError, match=r"no tensor noise_convs\.0\.bias"):
        nsf.check_state_dict(bad, cfg)
    bad = dict(sd)
    bad["enc_p.emb_phone.weight"] = torch.zeros(2)
    with pytest.raises(AlsepError, match=r"does not know: enc_p\.emb_phone\.weight"):
        nsf.check_state_dict(bad, cfg)
    plain = {k: v for k, v in sd.items() if not k.startswith("ups.0.weight_")}       # what remove_weight_norm leaves
    plain["ups.0.weight"] = nsf.fold_weight_norm(sd["ups.0.weight_g"], sd["ups.0.weight_v"])
    nsf.check_state_dict(plain, cfg)
    assert torch.equal(nsf.layer_weight(plain, "ups.0"), nsf.layer_weight(sd, "ups.0"))


@pytest.mark.parametrize("change,word", [
    (dict(resblock="2"), "resblock = '2'"),
    (dict(upsample_initial_channel=48), "48 over 2 stages leaves 12 channels"),
    (dict(initial_channel=100), "initial_channel = 100"),
    (dict(upsample_kernel_sizes=(6, 4)), "kernel 6 at rate 3"),
    (dict(upsample_kernel_sizes=(27, 4)), "kernel 27 at rate 3"),
    (dict(upsample_kernel_sizes=(7, 1)), "kernel 1 at rate 2"),
    (dict(upsample_rates=(2, 3), upsample_kernel_sizes=(4, 7)), "source stride 3"),
    (dict(resblock_kernel_sizes=(3, 4)), "kernel size 4"),
    (dict(resblock_kernel_sizes=(3, 13)), "kernel size 13"),
    (dict(resblock_dilation_sizes=((1, 2, 3), (1, 2, 6))), "dilation 6"),
    (dict(resblock_dilation_sizes=((1, 2, 3), (1, 2))), "dilations (1, 2)"),
])
def test_config_refuses_what_is_not_built(change, word):
    import dataclasses
    import re
    cfg = dataclasses.replace(o.REDUCED, **change)
    with pytest.raises(AlsepError, match=re.escape(word)):
        cfg.check()
    o.REDUCED.check()
    o.FULL.check()


def test_config_from_a_checkpoint_list():
    lst = [1025, 32, 192, 192, 768, 2, 6, 3, 0, "1", [3, 7, 11], [[1, 3, 5], [1, 3, 5], [1, 3, 5]], [10, 10, 2, 2], 512, [16, 16, 4, 4], 109, 256, "40k"]
    assert nsf.NSFConfig.from_rvc(lst) == nsf.V2_40K
    lst[17] = 40000
    assert nsf.NSFConfig.from_rvc(lst) == nsf.V2_40K
    with pytest.raises(AlsepError, match="17 entries"):
        nsf.NSFConfig.from_rvc(lst[:17])
    # v1 at 32 kHz: five stages, kernel 16 at rate 4 (four taps an output phase), 16 channels at the end
    lst[12], lst[14], lst[17] = [10, 4, 2, 2, 2], [16, 16, 4, 4, 4], "32k"
    cfg = nsf.NSFConfig.from_rvc(lst)
    cfg.check()
    assert cfg.upp == 320 and cfg.sr == 32000 and cfg.stage_channels(4) == 16
    assert nsf.param_shapes(cfg)["ups.1.weight_v"] == (256, 128, 16) and nsf.param_shapes(cfg)["noise_convs.1.weight"] == (128, 1, 16)


def _checkpoint(cfg, f0=1):
    sd = nsf.synthetic_state_dict(cfg, 2)
    weight = {f"dec.{k}": v for k, v in sd.items()}
    weight["emb_g.weight"] = torch.randn(3, cfg.gin_channels, generator=torch.Generator().manual_seed(0))
    weight["enc_p.emb_pitch.weight"] = torch.zeros(4, 4)                      # the rest of the synthesizer is ignored
    config = [1025, 32, cfg.initial_channel, 192, 768, 2, 6, 3, 0, cfg.resblock, list(cfg.resblock_kernel_sizes),
              [list(d) for d in cfg.resblock_dilation_sizes], list(cfg.upsample_rates), cfg.upsample_initial_channel,
              list(cfg.upsample_kernel_sizes), 3, cfg.gin_channels, "40k"]
    return {"config": config, "weight": weight, "f0": f0, "version": "v2", "info": "synthetic"}, sd


def test_checkpoint_round_trip(tmp_path, emul):
    cpt, sd = _checkpoint(o.REDUCED)
    path = tmp_path / "voice.pth"
    torch.save(cpt, path)
    voc, emb_g = nsf.load_rvc_vocoder(path, emul)
    assert voc.cfg == o.REDUCED and tuple(emb_g.shape) == (3, 8)
    assert torch.equal(emb_g, cpt["weight"]["emb_g.weight"])
    want = nsf.layer_weight(sd, "ups.1").permute(2, 0, 1).contiguous()
    assert torch.equal(voc.stages[1].w.cpu(), want)
    x, f0, _, noise = o.test_inputs(o.REDUCED, 5, 1)
    out = voc.forward(x, f0, emb_g[1][None, :, None], noise=noise)
    assert tuple(out.shape) == (1, 1, 5 * 6) and bool(torch.isfinite(out).all())


def test_checkpoint_refusals(tmp_path, emul):
    with pytest.raises(FileNotFoundError):
        nsf.load_rvc_vocoder(tmp_path / "missing.pth", emul)
    cpt, _ = _checkpoint(o.REDUCED, f0=0)
    torch.save(cpt, tmp_path / "nono.pth")
    with pytest.raises(AlsepError, match="f0 = 0"):
        nsf.load_rvc_vocoder(tmp_path / "nono.pth", emul)
