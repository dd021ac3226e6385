"""HTDemucs' half-precision mode (HTDemucs(precision="f16"), csrc/nn_demucs_h.h): each new kernel against float64 on the same half
operands, the whole network against the half-precision restatement (tests/htdemucs_half_oracle.py) and the float32 oracle, batch
invariance, the runner (one lane, batched units, the float32 re-run of a non-finite track) and the engine switch."""
import dataclasses
import logging
import math
import time

import numpy as np
import pytest
import torch

from audiolab_amd import _lib
from oracle import htdemucs_oracle as ho
from tests import htdemucs_half_oracle as hh
from tests.conftest import host, on


def half_cfg(**kw):
    base = dict(sources=("drums", "bass", "other"), channels=16, nfft=256, depth=2, dconv_comp=4, bottom_channels=64, t_layers=3,
                t_heads=1, segment_samples=2560, samplerate=4000)
    base.update(kw)
    return ho.HTDemucsConfig(**base)


def build(dev, ocfg, seed=1, precision="f16"):
    from audiolab_amd.htdemucs import HTDemucs, HTDemucsConfig
    sd = ho.synthetic_state_dict(ocfg, seed)
    return HTDemucs(HTDemucsConfig(**dataclasses.asdict(ocfg)), sd, ctx=dev, precision=precision), sd


def half_ulp(v: np.ndarray) -> np.ndarray:
    """the spacing of IEEE half at |v| (subnormal spacing below 2^-14)"""
    e = np.floor(np.log2(np.maximum(np.abs(v), 2.0 ** -14)))
    return 2.0 ** (e - 10)


# ---- kernels -------------------------------------------------------------------------------------------------------------------------
def run_conv(dev, B, H, Hv, W, Cin, Cout, KH, KW, st, pd, dl, act, x_f16, y_f16, bias=True, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, Hv, W, Cin, generator=g)
    x = x.half() if x_f16 else x
    K = KH * KW * Cin
    Kp = -(-K // 32) * 32
    w = (torch.randn(Cout, KH, KW, Cin, generator=g) / math.sqrt(K)).half()
    wp = torch.zeros(Cout, Kp, dtype=torch.float16)
    wp[:, :K] = w.reshape(Cout, K)
    b = torch.randn(Cout, generator=g) if bias else None
    Ho = (H + 2 * pd[0] - dl[0] * (KH - 1) - 1) // st[0] + 1
    Wo = (W + 2 * pd[1] - dl[1] * (KW - 1) - 1) // st[1] + 1
    y_ld = Cout + 4                                        # a row stride wider than Cout: the layer writes into a padded operand
    y = torch.zeros(B * Ho * Wo, y_ld, dtype=torch.float16 if y_f16 else torch.float32)
    xd, wd, yd = on(dev, x), on(dev, wp), on(dev, y)
    bd = on(dev, b) if bias else None
    dev.check(dev.lib.alsep_nn_conv_h(dev.handle, _lib.ptr(xd), int(x_f16), _lib.ptr(wd), _lib.ptr(bd), _lib.ptr(yd), int(y_f16), y_ld, B, H, Hv,
                                      W, Cin, Cin, Cout, Kp, KH, KW, st[0], st[1], pd[0], pd[1], dl[0], dl[1], act), "alsep_nn_conv_h")
    # float64 on the same half operands; rows >= Hv are the zero padding on the right
    xf = torch.zeros(B, H, W, Cin, dtype=torch.float64)
    xf[:, :Hv] = x.half().double()
    ref = torch.nn.functional.conv2d(xf.permute(0, 3, 1, 2), w.double().permute(0, 3, 1, 2), b.double() if bias else None, stride=st,
                                     padding=pd, dilation=dl).permute(0, 2, 3, 1).reshape(B * Ho * Wo, Cout)
    if act == 3:
        ref = torch.nn.functional.gelu(ref)
    got = host(yd).astype(np.float64)
    assert np.all(got[:, Cout:] == 0), "the kernel wrote beyond Cout"
    # the scale of the float32 accumulation: sum |x| |w| per output
    mag = torch.nn.functional.conv2d(xf.abs().permute(0, 3, 1, 2), w.double().abs().permute(0, 3, 1, 2), b.double().abs() if bias else None,
                                     stride=st, padding=pd, dilation=dl).permute(0, 2, 3, 1).reshape(B * Ho * Wo, Cout).numpy()
    return got[:, :Cout], ref.numpy(), mag


CONV_SMALL = [  # (B, H, Hv, W, Cin, Cout, KH, KW, stride, pad, dil): enc0 freq / time, DConv c1 (both axes, dilation 2), c2 1x1, rewrite 3x3
    (2, 64, 64, 5, 4, 16, 8, 1, (4, 1), (2, 0), (1, 1)),
    (2, 70, 67, 1, 2, 16, 8, 1, (4, 1), (2, 0), (1, 1)),
    (1, 8, 8, 37, 48, 6, 1, 3, (1, 1), (0, 2), (1, 2)),
    (3, 41, 41, 1, 16, 4, 3, 1, (1, 1), (2, 0), (2, 1)),
    (2, 9, 9, 7, 6, 96, 1, 1, (1, 1), (0, 0), (1, 1)),
    (1, 6, 6, 7, 32, 72, 3, 3, (1, 1), (1, 1), (1, 1)),
    (2, 33, 33, 1, 96, 160, 1, 1, (1, 1), (0, 0), (1, 1)),
]


@pytest.mark.parametrize("case", range(len(CONV_SMALL)))
def test_conv_h_vs_float64(dev, case):
    B, H, Hv, W, Cin, Cout, KH, KW, st, pd, dl = CONV_SMALL[case]
    for act, x_f16, y_f16, bias in ((0, True, False, True), (3, False, True, True), (0, False, False, False), (3, True, True, True)):
        got, ref, mag = run_conv(dev, B, H, Hv, W, Cin, Cout, KH, KW, st, pd, dl, act, x_f16, y_f16, bias, seed=case)
        if y_f16:
            # within one half ulp of the float64 value (float32 accumulation is three orders finer)
            assert np.all(np.abs(got - ref) <= half_ulp(ref) + 4e-7 * mag)
        else:
            # float32 accumulation: 2^-22 per product, measured below 2^-23 of sum |x w| + |bias|
            assert np.max(np.abs(got - ref) / np.maximum(mag, 1e-30)) < 2e-6


def run_norm(dev, G, R, C, act, y_f16, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(G, R, C, generator=g) * 3 + 1.5
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    Co = C // 2 if act == 4 else C
    y = torch.zeros(G * R, Co, dtype=torch.float16 if y_f16 else torch.float32)
    ws = torch.zeros(int(dev.lib.alsep_nn_norm_h_workspace_bytes(G, R * C)), dtype=torch.uint8)
    xd, yd, gd, bd, wd = on(dev, x), on(dev, y), on(dev, gamma), on(dev, beta), on(dev, ws)
    dev.check(dev.lib.alsep_nn_norm_h(dev.handle, _lib.ptr(xd), _lib.ptr(yd), int(y_f16), _lib.ptr(gd), _lib.ptr(bd), G, R, C, 1e-5, act,
                                      _lib.ptr(wd)), "alsep_nn_norm_h")
    xd64 = x.double()
    m = xd64.mean(dim=(1, 2), keepdim=True)
    v = xd64.var(dim=(1, 2), unbiased=False, keepdim=True)
    n = (xd64 - m) / torch.sqrt(v + 1e-5) * gamma.double() + beta.double()
    if act == 3:
        n = torch.nn.functional.gelu(n)
    elif act == 4:
        n = torch.nn.functional.glu(n, dim=-1)
    return host(yd).astype(np.float64), n.reshape(G * R, Co).numpy(), x


@pytest.mark.parametrize("G,R,C", [(5, 37, 6), (2, 700, 24), (9, 1, 64), (2, 3000, 12)])
def test_norm_h_vs_float64(dev, G, R, C):
    for act in (0, 3, 4):
        got, ref, _ = run_norm(dev, G, R, C, act, True)
        assert np.all(np.abs(got - ref) <= half_ulp(ref) + 1e-6 * (1 + np.abs(ref)))
    got, ref, _ = run_norm(dev, G, R, C, 4, False)
    assert np.max(np.abs(got - ref)) < 2e-5 * max(1.0, np.max(np.abs(ref)))


def test_norm_h_batch_invariant(dev):
    """a group's statistics do not depend on how many groups the launch has"""
    got, _, x = run_norm(dev, 3, 5000, 12, 3, True, seed=7)
    for gidx in range(3):
        gamma_seed = torch.Generator().manual_seed(7)
        torch.randn(3, 5000, 12, generator=gamma_seed)
        gamma, beta = torch.rand(12, generator=gamma_seed) + 0.5, torch.randn(12, generator=gamma_seed)
        y = torch.zeros(5000, 12, dtype=torch.float16)
        ws = torch.zeros(int(dev.lib.alsep_nn_norm_h_workspace_bytes(1, 5000 * 12)), dtype=torch.uint8)
        xd, yd, gd, bd, wd = on(dev, x[gidx].contiguous()), on(dev, y), on(dev, gamma), on(dev, beta), on(dev, ws)
        dev.check(dev.lib.alsep_nn_norm_h(dev.handle, _lib.ptr(xd), _lib.ptr(yd), 1, _lib.ptr(gd), _lib.ptr(bd), 1, 5000, 12, 1e-5, 3,
                                          _lib.ptr(wd)), "alsep_nn_norm_h")
        assert np.array_equal(host(yd).astype(np.float64), got[gidx * 5000:(gidx + 1) * 5000])


def run_xattn(dev, n_seq, Lq, Lk, heads, seed=0):
    g = torch.Generator().manual_seed(seed)
    c = heads * 64
    q = (torch.randn(n_seq, Lq, c, generator=g)).half()
    kv = (torch.randn(n_seq, Lk, 2 * c, generator=g)).half()
    out = torch.zeros(n_seq * Lq, c, dtype=torch.float16)
    qd, kd, od = on(dev, q), on(dev, kv), on(dev, out)
    dev.check(dev.lib.alsep_nn_xattention_f16(dev.handle, _lib.ptr(qd), _lib.ptr(kd), _lib.ptr(od), n_seq, Lq, Lk, heads, 64, Lq * c, c, Lk * 2 * c,
                                              2 * c, Lq * c, c, 0.125), "alsep_nn_xattention_f16")
    qh = q.double().view(n_seq, Lq, heads, 64).transpose(1, 2)
    kh = kv[..., :c].double().view(n_seq, Lk, heads, 64).transpose(1, 2)
    vh = kv[..., c:].double().view(n_seq, Lk, heads, 64).transpose(1, 2)
    # float64 on the same half operands, with the kernel's one extra rounding: P = exp(s - max) stored as half for P V
    s2 = (qh * (0.125 * 1.4426950408889634)).float().half().double() @ kh.transpose(-1, -2)
    e = torch.exp2(s2 - s2.amax(-1, keepdim=True))
    ref = ((e.float().half().double() @ vh) / e.sum(-1, keepdim=True)).transpose(1, 2).reshape(n_seq * Lq, c)
    return host(od).astype(np.float64), ref.numpy()


def _check_xattn(dev, n_seq, Lq, Lk, heads):
    got, ref = run_xattn(dev, n_seq, Lq, Lk, heads)
    # the kernel rounds exp(s - RUNNING max) to half and rescales in float32 (the restatement: the final max); result half
    assert np.max(np.abs(got - ref)) < 3e-3 * float(np.max(np.abs(ref)))
    assert np.mean(np.abs(got - ref)) < 2e-4 * float(np.max(np.abs(ref)))


@pytest.mark.parametrize("n_seq,Lq,Lk,heads", [(2, 70, 45, 2), (1, 33, 130, 1)])
def test_xattention_vs_float64(dev, n_seq, Lq, Lk, heads):
    _check_xattn(dev, n_seq, Lq, Lk, heads)


@pytest.mark.gpu
@pytest.mark.parametrize("Lq,Lk", [(2688, 1344), (1344, 2688)])
def test_xattention_production_shapes(gpu_ctx, Lq, Lk):
    _check_xattn(gpu_ctx, 2, Lq, Lk, 8)


# ---- whole network -------------------------------------------------------------------------------------------------------------------
def test_precision_argument(emul):
    from audiolab_amd.htdemucs import HTDemucs, HTDemucsConfig
    ocfg = ho.HTDemucsConfig(sources=("a",), channels=8, nfft=256, depth=1, dconv_comp=4, bottom_channels=32, t_layers=1, t_heads=4,
                             segment_samples=2560, samplerate=4000)
    sd = ho.synthetic_state_dict(ocfg, 0)
    with pytest.raises(_lib.AlsepError, match="64"):
        HTDemucs(HTDemucsConfig(**dataclasses.asdict(ocfg)), sd, ctx=emul, precision="f16")
    with pytest.raises(_lib.AlsepError, match="precision"):
        HTDemucs(HTDemucsConfig(**dataclasses.asdict(ocfg)), sd, ctx=emul, precision="bf16")


def test_forward_half_vs_oracles(dev):
    ocfg = half_cfg()
    net, sd = build(dev, ocfg)
    x = torch.randn(2, ocfg.segment_samples, generator=torch.Generator().manual_seed(3)) * 0.3
    want_h = hh.forward(ocfg, sd, x[None])[0]
    want_32 = ho.forward(ocfg, sd, x[None])[0]
    dev.launch_counts_reset()
    got = torch.from_numpy(host(net.forward(on(dev, x))))
    assert dev.launch_count("nn_dconv_h_kernel") > 0 and dev.launch_count("nn_norm_h_apply_kernel") > 0
    assert dev.launch_count("nn_xattn_h_kernel") == ocfg.t_layers // 2 * 2
    assert dev.launch_count("nn_attn_h_kernel") == (ocfg.t_layers + 1) // 2 * 2
    for f32_kernel in ("alsep_nn_conv2d", "nn_conv2d_tiled_kernel", "vr_conv2d_kernel", "nn_gemm_tn_kernel", "nn_bgemm_kernel"):
        assert dev.launch_count(f32_kernel) == 0, f32_kernel
    r_h, r_32, r_oo = hh.rel(got, want_h), hh.rel(got, want_32), hh.rel(want_h, want_32)
    print(f"htdemucs half: vs half oracle {r_h:.3e}, vs fp32 oracle {r_32:.3e}, half oracle vs fp32 oracle {r_oo:.3e}")
    assert got.shape == (3, 2, ocfg.segment_samples)
    assert r_h < 0.9 * r_oo and r_32 < 1.25 * r_oo and r_32 < 5e-3


def test_batch_bit_identical_to_single(dev):
    ocfg = half_cfg()
    net, _ = build(dev, ocfg, seed=2)
    g = torch.Generator().manual_seed(5)
    xs = torch.randn(3, 2, ocfg.segment_samples, generator=g) * 0.3
    yb = host(net.forward(on(dev, xs)))
    assert yb.shape == (3, 3, 2, ocfg.segment_samples)
    for b in range(3):
        assert np.array_equal(yb[b], host(net.forward(on(dev, xs[b])))), b
    short = xs[:, :, :2001].contiguous()                  # shorter than the training length: padded inside, cut back
    ys = host(net.forward(on(dev, short)))
    assert ys.shape == (3, 3, 2, 2001)
    for b in range(3):
        assert np.array_equal(ys[b], host(net.forward(on(dev, short[b])))), b


@pytest.mark.gpu
def test_htdemucs_6s_full_size_segment_half(gpu_ctx):
    """htdemucs_6s at full size, one 7.8 s segment, half precision against both oracles; prints the mode's cost"""
    from audiolab_amd.htdemucs import HTDemucs, HTDemucsConfig
    from audiolab_amd.synth import synth_mix
    ocfg = ho.HTDemucsConfig()
    sd = ho.synthetic_state_dict(ocfg, 0)
    net = HTDemucs(HTDemucsConfig(), sd, ctx=gpu_ctx, precision="f16")
    x = torch.from_numpy(synth_mix(ocfg.segment_samples)) * 2.0
    x = (x - x.mean()) / x.std()
    got = net.forward(x.cuda())
    gpu_ctx.synchronize()
    t0 = time.perf_counter()
    got = net.forward(x.cuda())
    gpu_ctx.synchronize()
    dt = time.perf_counter() - t0
    got = got.cpu()
    want_h = hh.forward(ocfg, sd, x[None])[0]
    want_32 = ho.forward(ocfg, sd, x[None])[0]
    r_h, r_32, r_oo = hh.rel(got, want_h), hh.rel(got, want_32), hh.rel(want_h, want_32)
    print(f"htdemucs_6s half segment: vs half oracle {r_h:.3e}, vs fp32 oracle {r_32:.3e}, mode cost (half vs fp32 oracle) {r_oo:.3e}, "
          f"{dt * 1e3:.1f} ms")
    assert got.shape == (6, 2, ocfg.segment_samples)
    assert r_h < 0.9 * r_oo and r_32 < 1.25 * r_oo and r_32 < 5e-3


# ---- runner and engine ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shifts", [0, 1, 2])
def test_runner_half_vs_oracle(dev, shifts):
    from audiolab_amd.htdemucs import DemucsRunner
    ocfg = half_cfg()
    net, sd = build(dev, ocfg)
    n = 6000
    mix = torch.randn(2, n, generator=torch.Generator().manual_seed(11)) * 0.4
    r = DemucsRunner(net, shifts=shifts, overlap=0.25, lanes=4, batch=3)
    got = r.separate(on(dev, mix))
    units, _, _ = r.units(n)
    assert r.lanes == 1 and r.batch == 3 and r.batches_run == -(-len(units) // 3)
    want_h = ho.separate(ocfg, sd, mix, shifts=shifts, overlap=0.25, fwd=hh.half_forward(ocfg, sd))
    want_32 = ho.separate(ocfg, sd, mix, shifts=shifts, overlap=0.25)
    g = torch.stack([torch.from_numpy(host(got[s])) for s in ocfg.sources])
    r_h, r_32, r_oo = hh.rel(g, want_h), hh.rel(g, want_32), hh.rel(want_h, want_32)
    print(f"runner half shifts={shifts}: {r_h:.3e} / {r_32:.3e} / {r_oo:.3e}")
    assert r_h < 0.9 * r_oo and r_32 < 1.25 * r_oo


def test_runner_half_bag_and_rerun(dev, caplog):
    from audiolab_amd.htdemucs import DemucsRunner
    from tests.test_demucs_bag import bag_oracle
    ocfg = half_cfg()
    n1, sd1 = build(dev, ocfg, seed=1)
    n2, sd2 = build(dev, ocfg, seed=2)
    f32, _ = build(dev, ocfg, seed=3, precision="f32")
    with pytest.raises(_lib.AlsepError, match="precision"):
        DemucsRunner([n1, f32])
    weights = [[1.0, 0.0, 2.0], [0.5, 1.0, 0.0]]               # the members carry different sources; "drums" is weighed by both
    mix = torch.randn(2, 4000, generator=torch.Generator().manual_seed(12)) * 0.4
    r = DemucsRunner([n1, n2], shifts=2, weights=weights, batch=2)
    got = r.separate(on(dev, mix))
    units, _, _ = r.units(4000)
    views, _ = r.views(4000)
    per_member = [sum(1 for u in units if views[u[0]].m == m) for m in range(2)]
    assert r.lanes == 1 and r.batches_run == sum(-(-n // 2) for n in per_member)     # batches never mix members
    with hh._half_mode():
        want_h = bag_oracle([ocfg, ocfg], [sd1, sd2], weights, mix, shifts=2)
    want_32 = bag_oracle([ocfg, ocfg], [sd1, sd2], weights, mix, shifts=2)
    g = np.stack([host(got[s]) for s in ocfg.sources])
    r_h, r_32, r_oo = hh.rel(g, want_h), hh.rel(g, want_32), hh.rel(want_h, want_32)
    print(f"half bag: vs half bag oracle {r_h:.3e}, vs fp32 bag oracle {r_32:.3e}, half vs fp32 oracle {r_oo:.3e}")
    assert r_h < 0.9 * r_oo and r_32 < 1.25 * r_oo
    # the non-finite re-run: forced through the host hook, it runs the float32 weights with a WARNING (one lane, as a one-lane float32 runner)
    want32 = DemucsRunner([n1.as_f32(), n2.as_f32()], shifts=2, weights=weights, lanes=1).separate(on(dev, mix))
    r._stems_finite = lambda out: False
    with caplog.at_level(logging.WARNING):
        again = r.separate(on(dev, mix))
    assert any("again in float32" in m for m in caplog.messages)
    for s in ocfg.sources:
        assert np.array_equal(host(again[s]), host(want32[s])), s


def test_separator_demucs_precision(dev, tmp_path, caplog):
    """htdemucs_6s.yaml (one model) and htdemucs_ft.yaml (a bag of four) from .th packages, in half precision with demucs_precision="f16",
    in float32 -- with four lanes on a GPU -- by default; a head size other than 64 falls back to float32 with a WARNING"""
    from audiolab_amd.engine import Separator
    from audiolab_amd.htdemucs import HTDemucsConfig
    from tests.test_loaders import _write_th
    c6 = HTDemucsConfig(**dataclasses.asdict(half_cfg(sources=("drums", "bass", "other", "vocals", "guitar", "piano"))))
    c4 = HTDemucsConfig(**dataclasses.asdict(half_cfg(sources=("drums", "bass", "other", "vocals"))))
    _write_th(str(tmp_path / "5c90dfd2-2b27f3ec.th"), c6, ho.synthetic_state_dict(half_cfg(sources=c6.sources), 4))
    (tmp_path / "htdemucs_6s.yaml").write_text("models: ['5c90dfd2']\n")
    sigs = ["f7e0c4bc", "d12395a8", "92cfc3b6", "04573f0d"]
    for i, sig in enumerate(sigs):
        _write_th(str(tmp_path / f"{sig}-{sig[::-1]}.th"), c4, ho.synthetic_state_dict(half_cfg(sources=c4.sources), 30 + i))
    (tmp_path / "htdemucs_ft.yaml").write_text(f"models: {sigs}\n")
    mix = torch.randn(2, 3000, generator=torch.Generator().manual_seed(2)) * 0.2
    for prec in ("f16", None):
        kw = {"demucs_precision": prec} if prec else {}
        sep = Separator(model_file_dir=str(tmp_path), ctx=dev, **kw)
        assert sep.demucs_precision == (prec or "f32")
        for name, n in (("htdemucs_6s.yaml", 1), ("htdemucs_ft.yaml", 4)):
            sep.load_model(name)
            r = sep.model_instance.demucs
            assert len(r.nets) == n and all(m.precision == (prec or "f32") for m in r.nets) and r.precision == (prec or "f32")
            assert r.lanes == (1 if prec or dev.device.type != "cuda" else 4)
        out = sep.separate_array(mix)
        assert len(out) == 4 and all(np.isfinite(np.asarray(v.cpu() if torch.is_tensor(v) else v)).all() for v in out.values())
    c8 = HTDemucsConfig(**dataclasses.asdict(half_cfg(bottom_channels=32, t_heads=4)))
    _write_th(str(tmp_path / "955717e8-8726e21a.th"), c8, ho.synthetic_state_dict(half_cfg(bottom_channels=32, t_heads=4), 9))
    (tmp_path / "htdemucs.yaml").write_text("models: ['955717e8']\n")
    sep = Separator(model_file_dir=str(tmp_path), ctx=dev, demucs_precision="f16")
    with caplog.at_level(logging.WARNING):
        sep.load_model("htdemucs.yaml")                       # head size 8: float32 with a WARNING
    assert sep.model_instance.demucs.precision == "f32"
    assert any("head size" in m and "float32" in m for m in caplog.messages)
    with pytest.raises(_lib.AlsepError):
        Separator(model_file_dir=str(tmp_path), ctx=dev, demucs_precision="bf16")


# ---- production shapes on the GPU ----------------------------------------------------------------------------------------------------
def _prod_rows():
    """every convolution of htdemucs_6s: (name, H, Hv, W, Cin, Cout, KH, KW, stride, pad, dil, x half)"""
    C = [48, 96, 192, 384]
    Fr = [2048, 512, 128, 32, 8]
    Lt = [343980, 85995, 21499, 5375, 1344]
    rows = []
    for i in range(4):
        cin = 4 if i == 0 else C[i - 1]
        c = C[i]
        rows.append((f"enc{i} conv f", Fr[i], Fr[i], 336, cin, c, 8, 1, (4, 1), (2, 0), (1, 1), False))
        rows.append((f"enc{i} conv t", -(-Lt[i] // 4) * 4, Lt[i], 1, 2 if i == 0 else C[i - 1], c, 8, 1, (4, 1), (2, 0), (1, 1), False))
        for br, H, W in (("f", Fr[i + 1], 336), ("t", Lt[i + 1], 1)):
            for d in (1, 2):
                k, p, dl = ((1, 3), (0, d), (1, d)) if br == "f" else ((3, 1), (d, 0), (d, 1))
                rows.append((f"dconv{i} c1 d{d} {br}", H, H, W, c, c // 8, *k, (1, 1), p, dl, False))
            rows.append((f"dconv{i} c2 {br}", H, H, W, c // 8, 2 * c, 1, 1, (1, 1), (0, 0), (1, 1), True))
            rows.append((f"enc{i} rewrite {br}", H, H, W, c, 2 * c, 1, 1, (1, 1), (0, 0), (1, 1), False))
            k, p = ((3, 3), (1, 1)) if br == "f" else ((3, 1), (1, 0))
            rows.append((f"dec{i} rewrite {br}", H, H, W, c, 2 * c, *k, (1, 1), p, (1, 1), False))
    return rows


@pytest.mark.gpu
def test_conv_h_production_shapes(gpu_ctx):
    """every htdemucs_6s convolution at batch 1 and at the runner's default batch (images 0 and B-1 checked) against float64 on the same
    half operands (an im2col GEMM in float64 on the GPU); bias / GELU / output type cycle over the rows"""
    from audiolab_amd.htdemucs import DEFAULT_F16_BATCH
    dev = gpu_ctx
    t0 = time.perf_counter()
    worst = {}
    for idx, (name, H, Hv, W, Cin, Cout, KH, KW, st, pd, dl, x_f16) in enumerate(_prod_rows()):
        act, y_f16, bias = [(3, False, True), (0, True, True), (0, False, False), (3, True, True)][idx % 4]
        for B in (1, DEFAULT_F16_BATCH):
            g = torch.Generator(device="cuda").manual_seed(idx)
            x = torch.randn(B, Hv, W, Cin, generator=g, device="cuda")
            x = x.half() if x_f16 else x
            K = KH * KW * Cin
            Kp = -(-K // 32) * 32
            w = (torch.randn(Cout, KH, KW, Cin, generator=g, device="cuda") / math.sqrt(K)).half()
            wp = torch.zeros(Cout, Kp, dtype=torch.float16, device="cuda")
            wp[:, :K] = w.reshape(Cout, K)
            b = torch.randn(Cout, generator=g, device="cuda") if bias else None
            Ho = (H + 2 * pd[0] - dl[0] * (KH - 1) - 1) // st[0] + 1
            Wo = (W + 2 * pd[1] - dl[1] * (KW - 1) - 1) // st[1] + 1
            y = torch.empty(B * Ho * Wo, Cout, dtype=torch.float16 if y_f16 else torch.float32, device="cuda")
            dev.check(dev.lib.alsep_nn_conv_h(dev.handle, _lib.ptr(x), int(x_f16), _lib.ptr(wp), _lib.ptr(b), _lib.ptr(y), int(y_f16), Cout, B, H,
                                              Hv, W, Cin, Cin, Cout, Kp, KH, KW, st[0], st[1], pd[0], pd[1], dl[0], dl[1], act), "alsep_nn_conv_h")
            w2 = w.double().permute(0, 3, 1, 2).reshape(Cout, K)
            for img in sorted({0, B - 1}):
                xf = torch.zeros(1, Cin, H, W, dtype=torch.float64, device="cuda")
                xf[0, :, :Hv] = x[img].half().double().permute(2, 0, 1)
                cols = torch.nn.functional.unfold(xf, (KH, KW), dilation=dl, padding=pd, stride=st)[0]      # [Cin KH KW, Ho Wo]
                ref = (w2 @ cols).t()
                mag = (w2.abs() @ cols.abs()).t()
                if bias:
                    ref = ref + b.double()
                    mag = mag + b.double().abs()                # the bias add is rounded in float32 too
                if act == 3:
                    ref = torch.nn.functional.gelu(ref)
                got = y[img * Ho * Wo:(img + 1) * Ho * Wo].double()
                err = (got - ref).abs()
                if y_f16:
                    ulp = 2.0 ** (torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -14))) - 10)
                    q = float((err / (ulp + 4e-7 * mag)).max())
                    assert q <= 1.0, (name, B, img, q)
                else:
                    q = float((err / mag.clamp_min(1e-30)).max())
                    assert q < 2e-6, (name, B, img, q)
                worst[name] = max(worst.get(name, 0.0), q)
    print(f"conv_h production shapes: {len(worst)} rows, worst bound ratio {max(worst.values()):.3g}, {time.perf_counter() - t0:.1f} s")


@pytest.mark.gpu
def test_htdemucs_6s_batch8_bit_identical_full_size(gpu_ctx):
    """at full size the frequency-branch Linears (M = 2688) run on the persistent GEMM, whose tile height depends on the batch count:
    a batch of 8 different segments must still give each segment's single-forward bits"""
    from audiolab_amd.htdemucs import HTDemucs, HTDemucsConfig
    from audiolab_amd.synth import synth_mix
    cfg = HTDemucsConfig()
    net = HTDemucs(cfg, ho.synthetic_state_dict(ho.HTDemucsConfig(), 0), ctx=gpu_ctx, precision="f16")
    base = torch.from_numpy(synth_mix(cfg.segment_samples + 8 * 4410)).cuda()
    xs = torch.stack([base[:, 4410 * b: 4410 * b + cfg.segment_samples] * (1.0 + 0.1 * b) for b in range(8)]).contiguous()
    yb = net.forward(xs)
    for b in range(8):
        assert torch.equal(yb[b], net.forward(xs[b].contiguous())), b


@pytest.mark.gpu
def test_htdemucs_6s_ten_minutes_half(gpu_ctx):
    """htdemucs_6s f16 on the 10-minute synthetic track: two runs bit-identical, shapes, rel-L2 against the float32 mode within 2x of the
    3.0e-4 measured (profiles/demucs_half_bench.txt)"""
    from audiolab_amd.htdemucs import DemucsRunner, HTDemucs, HTDemucsConfig
    from audiolab_amd.synth import synth_mix
    cfg = HTDemucsConfig()
    net = HTDemucs(cfg, ho.synthetic_state_dict(ho.HTDemucsConfig(), 0), ctx=gpu_ctx, precision="f16")
    mix = torch.from_numpy(synth_mix(600 * cfg.samplerate)).cuda()
    r = DemucsRunner(net, shifts=2, overlap=0.25)
    t0 = time.perf_counter()
    a = r.separate(mix)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    b = r.separate(mix)
    c = DemucsRunner(net.as_f32(), shifts=2, overlap=0.25).separate(mix)
    assert list(a) == list(cfg.sources)
    for s in cfg.sources:
        assert a[s].shape == (2, mix.shape[-1]) and torch.equal(a[s], b[s]), s
    ga, gc = torch.stack([a[s] for s in cfg.sources]), torch.stack([c[s] for s in cfg.sources])
    rel = float((ga - gc).double().norm() / gc.double().norm())
    print(f"htdemucs_6s 10 min: f16 {dt:.2f} s (first run), f16 vs f32 rel-L2 {rel:.3e}")
    assert rel < 6e-4
