"""Bags of Demucs models (htdemucs_ft, htdemucs): the bag reader (th_reader.resolve_demucs_bag), the bag runner (DemucsRunner over several
member networks and a per-source weight matrix), its finishing kernel (alsep_demucs_bag_finish in csrc/nn.hip) and the engine's roster
entries -- against a bag oracle composed here from oracle/htdemucs_oracle.py's pieces (demucs 4 apply.py semantics, restated: PARITY
UNPINNED): every member runs demucs' apply_model with its own slice of one seeded shift sequence, the outputs are weighed per source,
summed and divided by the per-source weight totals, inside the separator's whole-track normalisation."""
import ctypes as C
import dataclasses
import hashlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import htdemucs_oracle as ho
from tests.conftest import host, on
from tests.test_htdemucs import small_cfg
from tests.test_loaders import _write_th

SRC4 = ("drums", "bass", "other", "vocals")
IDENTITY4 = [[1.0 if i == j else 0.0 for j in range(4)] for i in range(4)]


def bag_oracle(ocfgs, sds, weights, mix, shifts, overlap=0.25, seed=0):
    """[S, 2, L]: apply_model(BagOfModels) inside DemucsSeparator's normalisation; member m, pass p at offset
    shift_offsets(M * shifts, max_shift, seed)[m * shifts + p]"""
    M, L = len(sds), mix.shape[-1]
    ref = mix.mean(0)
    mean, std = ref.mean(), ref.std()
    x = ((mix - mean) / std)[None]
    max_shift = int(0.5 * ocfgs[0].samplerate) if shifts else 0
    offs = ho.shift_offsets(M * shifts, max_shift, seed) if shifts else []
    est, tot = 0.0, 0.0
    for m, (ocfg, sd) in enumerate(zip(ocfgs, sds)):
        fwd = (lambda c, ocfg=ocfg, sd=sd: ho.forward(ocfg, sd, c))
        if not shifts:
            out = ho._run_split(ocfg, x, 0, L, overlap, fwd)
        else:
            padded = F.pad(x, (max_shift, max_shift))
            out = 0.0
            for p in range(shifts):
                off = offs[m * shifts + p]
                out = out + ho._run_split(ocfg, padded, off, L + max_shift - off, overlap, fwd)[..., max_shift - off:]
            out = out / shifts
        w = torch.tensor(weights[m], dtype=torch.float32)[None, :, None, None]
        est = est + w * out
        tot = tot + w
    return ((est / tot)[0] * std + mean).numpy()


def members(dev, ocfg, seeds):
    from audiolab_amd.htdemucs import HTDemucs, HTDemucsConfig
    sds = [ho.synthetic_state_dict(ocfg, s) for s in seeds]
    return [HTDemucs(HTDemucsConfig(**dataclasses.asdict(ocfg)), sd, ctx=dev) for sd in sds], sds


# ---- 1. host: the bag reader and the engine's member check -----------------------------------------------------------------------
def _touch_th(tmp_path, sigs):
    for sig in sigs:
        (tmp_path / f"{sig}-0123abcd.th").write_bytes(b"")


def test_resolve_demucs_bag(tmp_path):
    from audiolab_amd import th_reader
    from audiolab_amd._lib import AlsepError
    assert th_reader.resolve_demucs_bag(str(tmp_path), "htdemucs_ft.yaml") is None
    _touch_th(tmp_path, ["f7e0c4bc", "d12395a8", "92cfc3b6", "04573f0d"])
    (tmp_path / "htdemucs_ft.yaml").write_text("models: ['f7e0c4bc', 'd12395a8', '92cfc3b6', '04573f0d']\n"
                                               "weights: [[1., 0., 0., 0.], [0., 1., 0., 0.], [0., 0., 1., 0.], [0., 0., 0., 1.]]\n"
                                               "segment: 44\n")
    paths, w, seg = th_reader.resolve_demucs_bag(str(tmp_path), "htdemucs_ft.yaml")
    assert [p.split("/")[-1] for p in paths] == ["f7e0c4bc-0123abcd.th", "d12395a8-0123abcd.th", "92cfc3b6-0123abcd.th", "04573f0d-0123abcd.th"]
    assert w == IDENTITY4 and seg == 44.0
    # no weights: all ones (demucs' default) -- as a matrix when the caller knows the sources, None (= all ones) otherwise
    (tmp_path / "two.yaml").write_text("models: ['f7e0c4bc', 'd12395a8']\n")
    assert th_reader.resolve_demucs_bag(str(tmp_path), "two.yaml", n_sources=3)[1] == [[1.0] * 3] * 2
    paths, w, seg = th_reader.resolve_demucs_bag(str(tmp_path), "two.yaml")
    assert len(paths) == 2 and w is None and seg is None
    assert th_reader.bag_weights(None, 2, 4, "x") == [[1.0] * 4] * 2
    # a member file missing: the error names its signature
    (tmp_path / "gap.yaml").write_text("models: ['f7e0c4bc', 'beefcafe']\n")
    with pytest.raises(AlsepError, match="beefcafe"):
        th_reader.resolve_demucs_bag(str(tmp_path), "gap.yaml")
    # the weight matrix: wrong shape, a source whose weights sum to 0, a negative or non-finite weight
    for bad in ("[[1, 1], [1, 1], [1, 1]]", "[[1, 1, 1], [1, 1]]", "[[1, 0, 1], [1, 0, 1]]", "[[1, -1, 1], [1, 2, 1]]", "[[1, .nan, 1], [1, 1, 1]]",
                "[[1, .inf, 1], [1, 1, 1]]", "[1, 1]"):
        (tmp_path / "bad.yaml").write_text(f"models: ['f7e0c4bc', 'd12395a8']\nweights: {bad}\n")
        with pytest.raises(AlsepError):
            th_reader.resolve_demucs_bag(str(tmp_path), "bad.yaml")
    (tmp_path / "bad.yaml").write_text("models: ['f7e0c4bc', 'd12395a8']\nweights: [[1, 1, 1], [1, 1, 1]]\n")
    with pytest.raises(AlsepError):
        th_reader.resolve_demucs_bag(str(tmp_path), "bad.yaml", n_sources=4)           # 3 weights per model, the members have 4 sources
    # resolve_demucs_yaml keeps refusing a bag of several models
    with pytest.raises(AlsepError):
        th_reader.resolve_demucs_yaml(str(tmp_path), "htdemucs_ft.yaml")


def test_engine_refuses_members_that_disagree(emul, tmp_path):
    from audiolab_amd import htdemucs as H
    from audiolab_amd._lib import AlsepError
    from audiolab_amd.engine import Separator
    base = dict(channels=16, depth=2, nfft=256, bottom_channels=32, t_layers=2, t_heads=4, dconv_comp=4, segment_samples=2560, samplerate=4000)
    c4 = H.HTDemucsConfig(sources=SRC4, **base)
    c3 = H.HTDemucsConfig(sources=SRC4[:3], **base)
    _write_th(str(tmp_path / "aaaa0001-00.th"), c4, H.synthetic_state_dict(c4, 1))
    _write_th(str(tmp_path / "aaaa0002-00.th"), c3, H.synthetic_state_dict(c3, 2))
    (tmp_path / "htdemucs_ft.yaml").write_text("models: ['aaaa0001', 'aaaa0002']\n")
    eng = Separator(model_file_dir=str(tmp_path), ctx=emul, use_autocast=False, allow_synthetic=True)
    with pytest.raises(AlsepError, match="sources"):
        eng.load_model("htdemucs_ft.yaml")
    # ... and the runner refuses them too
    with pytest.raises(AlsepError):
        H.DemucsRunner([H.HTDemucs(c4, H.synthetic_state_dict(c4, 1), ctx=emul), H.HTDemucs(c3, H.synthetic_state_dict(c3, 2), ctx=emul)])
    # a bag with a member missing is an error even with allow_synthetic: never half synthetic
    (tmp_path / "htdemucs_ft.yaml").write_text("models: ['aaaa0001', 'aaaa0003']\n")
    with pytest.raises(AlsepError, match="aaaa0003"):
        eng.load_model("htdemucs_ft.yaml")


# ---- 2. the bag runner against the composed oracle (emulated kernels and GPU) ------------------------------------------------------
def test_bag_runner_weighted_two_members_vs_oracle(dev):
    from audiolab_amd.htdemucs import DemucsRunner
    ocfg = small_cfg()
    nets, sds = members(dev, ocfg, (7, 8))
    weights = [[1.0, 0.5, 0.0], [0.0, 1.0, 2.0]]
    mix = torch.randn(2, 4001, generator=torch.Generator().manual_seed(11)) * 0.2 + 0.01      # not a multiple of the stride (1920)
    want = bag_oracle([ocfg, ocfg], sds, weights, mix, shifts=2)
    runner = DemucsRunner(nets, shifts=2, overlap=0.25, seed=0, weights=weights)
    dev.launch_counts_reset()
    out = runner.separate(on(dev, mix))
    assert dev.launch_count("demucs_bag_finish_kernel") == 1
    assert list(out) == list(ocfg.sources)
    got = np.stack([host(out[k]) for k in ocfg.sources])
    err = float(np.max(np.abs(got - want)))
    print(f"bag of 2 (weights {weights}), shifts 2: max|delta| = {err:.3e}, peak {np.max(np.abs(want)):.3f}")
    assert got.shape == want.shape == (3, 2, 4001) and np.max(np.abs(want)) > 1e-3 and err < 1e-4
    # the views carry only the sources their member weighs: member 0 drums + bass, member 1 bass + other
    views, _ = runner.views(4001)
    assert [(v.m, v.rows) for v in views] == [(0, [0, 1]), (0, [0, 1]), (1, [1, 2]), (1, [1, 2])]


def test_bag_runner_identity_four_members_short_track_vs_oracle(dev):
    from audiolab_amd.htdemucs import DemucsRunner
    ocfg = small_cfg(sources=SRC4)
    nets, sds = members(dev, ocfg, (1, 2, 3, 4))
    mix = torch.randn(2, 1500, generator=torch.Generator().manual_seed(5)) * 0.2               # shorter than one segment (2560)
    want = bag_oracle([ocfg] * 4, sds, IDENTITY4, mix, shifts=1)
    runner = DemucsRunner(nets, shifts=1, overlap=0.25, seed=0, weights=IDENTITY4)
    dev.launch_counts_reset()
    out = runner.separate(on(dev, mix))
    assert dev.launch_count("demucs_bag_finish_kernel") == 1
    got = np.stack([host(out[k]) for k in SRC4])
    assert float(np.max(np.abs(got - want))) < 1e-4 and np.max(np.abs(want)) > 1e-3
    # a bag of one is the single-model runner, bit for bit (same path: no finishing kernel)
    one = DemucsRunner([nets[0]], shifts=1, overlap=0.25, seed=0, weights=[[1.0, 2.0, 3.0, 4.0]])
    plain = DemucsRunner(nets[0], shifts=1, overlap=0.25, seed=0)
    dev.launch_counts_reset()
    a, b = one.separate(on(dev, mix)), plain.separate(on(dev, mix))
    assert dev.launch_count("demucs_bag_finish_kernel") == 0
    for k in SRC4:
        assert torch.equal(a[k], b[k])


# ---- 3. the finishing kernel against a float64 evaluation of its formula ---------------------------------------------------------
def _finish_ref(accs, wsums, lds, cuts, row, coef, stats, V, S, L):
    out = torch.zeros(S, 2, L, dtype=torch.float64)
    for v in range(V):
        w = wsums[v][cuts[v]: cuts[v] + L].double()
        for s in range(S):
            r = row[v * S + s]
            if r < 0:
                continue
            for c in range(2):
                a = accs[v].reshape(-1)[(2 * r + c) * lds[v] + cuts[v]: (2 * r + c) * lds[v] + cuts[v] + L].double()
                q = torch.where(w != 0, a / torch.where(w != 0, w, torch.ones_like(w)), torch.zeros_like(a))
                out[s, c] += float(coef[v * S + s]) * q
    return out * float(stats[1]) + float(stats[0])


def test_bag_finish_kernel_vs_float64(dev):
    g = torch.Generator().manual_seed(3)
    S, L = 6, 3001
    spec = [(2500, 150, [0, 2, 5]), (3200, 0, [1, 2, 3, 4]), (3011, 10, [5]), (3001, 0, list(range(6)))]     # (ld, cut, carried sources)
    V = len(spec)
    accs, wsums, row, coef = [], [], [], []
    lds = [ld if ld >= cut + L else cut + L for ld, cut, _ in spec]
    cuts = [cut for _, cut, _ in spec]
    for (_, cut, rows), ld in zip(spec, lds):
        accs.append(torch.randn(len(rows) * 2, ld, generator=g))
        w = torch.rand(ld, generator=g) + 0.25
        w[torch.rand(ld, generator=g) < 0.1] = 0.0                                      # samples no unit covers
        wsums.append(w)
        j = {s: i for i, s in enumerate(rows)}
        row += [j.get(s, -1) for s in range(S)]
        coef += [float(torch.rand(1, generator=g)) if s in j else 0.0 for s in range(S)]
    stats = torch.tensor([0.03, 1.7])
    want = _finish_ref(accs, wsums, lds, cuts, row, coef, stats, V, S, L)
    d_acc, d_ws = [on(dev, a) for a in accs], [on(dev, w) for w in wsums]
    arrays = dict(acc=on(dev, torch.tensor([a.data_ptr() for a in d_acc], dtype=torch.int64)),
                  ws=on(dev, torch.tensor([w.data_ptr() for w in d_ws], dtype=torch.int64)),
                  ld=on(dev, torch.tensor(lds, dtype=torch.int64)), cut=on(dev, torch.tensor(cuts, dtype=torch.int32)),
                  row=on(dev, torch.tensor(row, dtype=torch.int32)), coef=on(dev, torch.tensor(coef, dtype=torch.float32)),
                  stats=on(dev, stats))
    out = dev.zeros((S, 2, L))
    from audiolab_amd import _lib
    P = {k: _lib.ptr(v) for k, v in arrays.items()}

    def call(V_, S_, L_, out_ptr=None):
        return dev.lib.alsep_demucs_bag_finish(dev.handle, P["acc"], P["ws"], P["ld"], P["cut"], P["row"], P["coef"], P["stats"],
                                               out_ptr if out_ptr is not None else _lib.ptr(out), V_, S_, L_)
    dev.launch_counts_reset()
    assert call(V, S, L) == 0
    dev.synchronize()
    assert dev.launch_count("demucs_bag_finish_kernel") == 1
    got = host(out).astype(np.float64)
    rel = float(np.max(np.abs(got - want.numpy())) / np.max(np.abs(want.numpy())))
    print(f"bag finish: V={V} S={S} L={L}: max relative error {rel:.2e}")
    assert rel < 1e-6
    # arguments out of range: ALSEP_ERR_ARG (-1), nothing launched
    for bad in ((V, 9, L), (V, 0, L), (65, S, L), (0, S, L), (V, S, 0), (V, S, -5), (V, S, 1 << 31)):
        assert call(*bad) == -1, bad
    assert call(V, S, L, out_ptr=C.c_void_p(None)) == -1
    assert dev.launch_count("demucs_bag_finish_kernel") == 1


# ---- 4. the engine end to end: htdemucs_ft / htdemucs from .th packages, and the synthetic bag ------------------------------------
def test_engine_loads_htdemucs_ft_bag(emul, tmp_path):
    from audiolab_amd import htdemucs as H
    from audiolab_amd.engine import MODEL_ROSTER, Separator
    cfg = H.HTDemucsConfig(sources=SRC4, channels=16, depth=2, nfft=256, bottom_channels=32, t_layers=2, t_heads=4, dconv_comp=4,
                           segment_samples=2560, samplerate=4000)
    sds = [H.synthetic_state_dict(cfg, 20 + i) for i in range(4)]
    sigs = ["f7e0c4bc", "d12395a8", "92cfc3b6", "04573f0d"]
    for sig, sd in zip(sigs, sds):
        _write_th(str(tmp_path / f"{sig}-{sig[::-1]}.th"), cfg, sd)
    (tmp_path / "htdemucs_ft.yaml").write_text(f"models: {sigs}\nweights: {IDENTITY4}\nsegment: 44\n")
    eng = Separator(model_file_dir=str(tmp_path), ctx=emul, use_autocast=False)
    eng.load_model("htdemucs_ft.yaml")
    runner = eng.model_instance.demucs
    assert eng.weights_provenance() == "real" and len(runner.nets) == 4 and runner.net is runner.nets[0] and runner.net.cfg == cfg
    assert (runner.shifts, runner.overlap) == (MODEL_ROSTER["htdemucs_ft.yaml"][2]["shifts"], MODEL_ROSTER["htdemucs_ft.yaml"][2]["overlap"])
    mix = torch.randn(2, 2200, generator=torch.Generator().manual_seed(2)) * 0.2
    emul.launch_counts_reset()
    out = eng.separate_array(mix)
    assert emul.launch_count("demucs_bag_finish_kernel") == 1
    assert list(out) == ["Drums", "Bass", "Other", "Vocals"]
    ocfg = ho.HTDemucsConfig(**dataclasses.asdict(cfg))
    want = bag_oracle([ocfg] * 4, [{k: v.half().float() for k, v in sd.items()} for sd in sds], IDENTITY4, mix, shifts=2)
    for i, k in enumerate(out):
        assert float(np.max(np.abs(out[k].numpy() - want[i]))) < 1e-4, k


def test_engine_loads_htdemucs_and_synthetic_bag(emul, tmp_path):
    from audiolab_amd import htdemucs as H
    from audiolab_amd.engine import MODEL_ROSTER, Separator
    cfg = H.HTDemucsConfig(sources=SRC4, channels=16, depth=2, nfft=256, bottom_channels=32, t_layers=2, t_heads=4, dconv_comp=4,
                           segment_samples=2560, samplerate=4000)
    _write_th(str(tmp_path / "955717e8-8726e21a.th"), cfg, H.synthetic_state_dict(cfg, 9))
    (tmp_path / "htdemucs.yaml").write_text("models: ['955717e8']\n")
    eng = Separator(model_file_dir=str(tmp_path), ctx=emul, use_autocast=False)
    eng.load_model("htdemucs.yaml")
    assert eng.weights_provenance() == "real" and eng.model_instance.demucs.net.cfg == cfg and len(eng.model_instance.demucs.nets) == 1
    assert MODEL_ROSTER["htdemucs.yaml"][1].sources == SRC4 and MODEL_ROSTER["htdemucs_ft.yaml"][1].sources == SRC4
    # allow_synthetic with an empty directory: the roster's published layout, four members seeded from "<name>#<i>"
    name = "htdemucs_ft.yaml"
    opts = MODEL_ROSTER[name][2]
    assert opts["members"] == 4 and opts["weights"] == IDENTITY4
    empty = tmp_path / "empty"
    empty.mkdir()
    eng = Separator(model_file_dir=str(empty), ctx=emul, use_autocast=False, allow_synthetic=True, roster={name: ("demucs", cfg, opts)})
    eng.load_model(name)
    runner = eng.model_instance.demucs
    assert eng.weights_provenance() == "synthetic" and len(runner.nets) == 4 and runner.weights == IDENTITY4
    for i, n in enumerate(runner.nets):
        seed = int.from_bytes(hashlib.sha256(f"{name}#{i}".encode()).digest()[:4], "little")
        assert torch.equal(n.enc[0]["conv"].w.cpu(), H.HTDemucs(cfg, H.synthetic_state_dict(cfg, seed), ctx=emul).enc[0]["conv"].w.cpu())
    # without allow_synthetic an empty directory is an error
    with pytest.raises(Exception):
        Separator(model_file_dir=str(empty), ctx=emul, use_autocast=False, roster={name: ("demucs", cfg, opts)}).load_model(name)


# ---- 6. GPU, full size --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def full_bag(gpu_ctx):
    from audiolab_amd.htdemucs import HTDemucs, HTDemucsConfig
    cfg = HTDemucsConfig(sources=SRC4)
    nets = [HTDemucs(cfg, ho.synthetic_state_dict(ho.HTDemucsConfig(sources=SRC4), 40 + i), ctx=gpu_ctx) for i in range(4)]
    mix = torch.randn(2, 44100 * 20, generator=torch.Generator().manual_seed(6)).cuda() * 0.3
    return nets, mix


@pytest.mark.gpu
def test_full_size_identity_bag_equals_its_members(gpu_ctx, full_bag):
    """htdemucs_ft's layout at the real HTDemucs size, 20 s, shifts 0: stem s of the identity bag is member s's own stem s"""
    from audiolab_amd.htdemucs import DemucsRunner
    nets, mix = full_bag
    bag = DemucsRunner(nets, shifts=0, overlap=0.25, seed=0, weights=IDENTITY4).separate(mix)
    for s, name in enumerate(SRC4):
        single = DemucsRunner(nets[s], shifts=0, overlap=0.25, seed=0).separate(mix)[name]
        peak = float(single.abs().max())
        err = float((bag[name] - single).abs().max())
        print(f"{name}: bag vs member {s}: max|delta| = {err:.3e}, peak {peak:.3f}")
        assert peak > 1e-3 and err < 2e-6 * peak, (name, err, peak)


@pytest.mark.gpu
def test_full_size_bag_lanes_reproducible(gpu_ctx, full_bag):
    """the bag's units of all members dealt over four lanes against one lane, three repeats"""
    from audiolab_amd.htdemucs import DemucsRunner
    nets, mix = full_bag
    one = DemucsRunner(nets, shifts=1, overlap=0.25, seed=0, weights=IDENTITY4, lanes=1).separate(mix)
    four = DemucsRunner(nets, shifts=1, overlap=0.25, seed=0, weights=IDENTITY4, lanes=4)
    peak = max(float(v.abs().max()) for v in one.values())
    for rep in range(3):
        out = four.separate(mix)
        for k in one:
            assert float((one[k] - out[k]).abs().max()) < 2e-6 * peak, (k, rep)
    assert peak > 1e-3
