"""The VR networks' half-precision mode (``VRNet`` / ``VRNetNew(precision="f16")``, csrc/vrnet_h.h): each kernel alone against float64 on
the same half operands under a derived bound, the fused decoder input against the unfused half path bit for bit, every layer of the whole
network on the input the device network itself had, the whole network against the reference's own outputs (tests/golden/vrnet.npz), a
deliberately wrong layer, the runner and the engine, the untouched default, and on the GPU the production shapes, the launch counts and
the full-size roster models against the float32 engine.

Measured values (emulation and GPU): profiles/vr_half_accuracy.txt."""
import hashlib
import json
import logging
import os

import numpy as np
import pytest
import torch

from audiolab_amd import _lib
from tests import vr_half_oracle as vo
from tests.conftest import host, on

ACTS = {"none": 0, "relu": 1, "leaky": 2}


def worst(got, ref, bound):
    """max of |got - ref| / bound (<= 1 passes)"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.max(np.abs(got - ref) / bound))


# ---- 1. kernels alone ------------------------------------------------------------------------------------------------------------------
def make_conv(cin, cout, k, act, stride, pad, dil, seed):
    g = torch.Generator().manual_seed(seed)
    sd = {"c.weight": torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5,
          "bn.weight": 0.8 + 0.4 * torch.rand(cout, generator=g), "bn.bias": 0.1 * torch.randn(cout, generator=g),
          "bn.running_mean": 0.1 * torch.randn(cout, generator=g), "bn.running_var": 0.5 + torch.rand(cout, generator=g)}
    return sd, vo.Conv(sd, "c.weight", "bn", act, stride, pad, dil), g


def run_conv_h(dev, B, H, W, cin, cout, k, act, stride, pad, dil, y_f16, ct, c0, seed=0, bands=None):
    """alsep_vr_conv_h through vrnet._Conv's packing; returns worst |got - ref| / bound.  ``bands``: compare the first and the last
    ``bands`` output rows only (the float64 convolution of a production-size layer is recomputed on the rows those need)."""
    from audiolab_amd.vrnet import _Conv
    sd, ora, g = make_conv(cin, cout, k, act, stride, pad, dil, seed)
    L = _Conv(dev, sd, "c.weight", "bn", act, stride, pad, dil, precision="f16")
    x = (torch.randn(B, H, W, cin, generator=g) * 1.5).half()
    ho, wo = L.out_hw(H, W)
    y = torch.zeros(B, ho, wo, ct, dtype=torch.float16 if y_f16 else torch.float32)
    xd, yd = on(dev, x), on(dev, y)
    dev.check(dev.lib.alsep_vr_conv_h(dev.handle, _lib.ptr(xd), _lib.ptr(L.w), _lib.ptr(L.scale), _lib.ptr(L.shift), _lib.ptr(yd), int(y_f16), B, H,
                                      W, cin, cout, L.kp, k, k, stride, L.pad[0], L.pad[1], L.dil[0], L.dil[1], L.act, ct, c0), "alsep_vr_conv_h")
    got = host(yd).astype(np.float64)
    out = np.ones(ct, dtype=bool)
    out[c0:c0 + cout] = False
    assert not np.any(got[..., out]), "the kernel wrote outside its channel slice"
    got = got[..., c0:c0 + cout]
    xs = x.double()
    if bands is None:
        return worst(got, ora.value(xs).numpy(), vo.out_bound(ora.value(xs).numpy(), ora.arith(xs), y_f16))
    # input rows that the first / last `bands` output rows read, with a margin; rows of the cropped result near the cut are dropped
    need = bands * stride + (k - 1) * L.dil[0] + stride
    top, bot = xs[:, :need], xs[:, H - need - (H - need) % stride:]          # the bottom crop starts on the stride grid
    w1 = worst(got[:, :bands], ora.value(top).numpy()[:, :bands], vo.out_bound(ora.value(top).numpy(), ora.arith(top), y_f16)[:, :bands])
    vb, ab = ora.value(bot).numpy(), ora.arith(bot)
    w2 = worst(got[:, ho - bands:], vb[:, vb.shape[1] - bands:], vo.out_bound(vb, ab, y_f16)[:, vb.shape[1] - bands:])
    return max(w1, w2)


CONV_TOY = [  # (B, H, W, Cin, Cout, k, act, stride, pad, dil, y_f16, y_ctotal, c0)
    (2, 17, 13, 2, 16, 3, "leaky", 1, 1, 1, True, 16, 0),              # the first layer: Cin 2
    (2, 17, 13, 16, 32, 3, "leaky", 2, 1, 1, True, 32, 0),             # stride 2
    (1, 9, 11, 49, 2, 1, "none", 1, 0, 1, False, 2, 0),                # Cin 49, Cout 2, float32 out (the logits)
    (1, 9, 11, 40, 1, 1, "relu", 1, 0, 1, False, 1, 0),                # Cout 1, float32 out (the LSTM module's convolution)
    (2, 20, 9, 8, 24, 3, "relu", 1, 16, 16, True, 72, 28),             # dilation 16 into a slice, c0 > 0
    (2, 20, 9, 24, 24, 3, "relu", 1, (4, 2), (4, 2), True, 120, 48),   # nets_new ASPP: a dilation per axis, slice
    (1, 12, 10, 25, 8, 3, "relu", 1, 1, 1, True, 8, 0),                # nets_new dec1: 3 nout + 1 input channels
    (3, 8, 7, 16, 40, 1, "relu", 1, 0, 1, True, 45, 5),                # 1x1 into an odd slice offset (element stores)
    (1, 16, 24, 64, 136, 3, "leaky", 1, 1, 1, True, 136, 0),           # more than one channel tile
    (1, 6, 5, 18, 16, 1, "none", 1, 0, 1, True, 16, 0),                # no activation, half out
]


@pytest.mark.parametrize("case", range(len(CONV_TOY)))
def test_conv_h_vs_float64(dev, case):
    B, H, W, cin, cout, k, act, stride, pad, dil, y_f16, ct, c0 = CONV_TOY[case]
    for a, f16 in ((act, y_f16), ("none", not y_f16), ("relu", y_f16), ("leaky", not y_f16)):      # every activation, both output types
        w = run_conv_h(dev, B, H, W, cin, cout, k, a, stride, pad, dil, f16, ct, c0, seed=case)
        print(f"conv case {case} act {a} y_f16 {f16}: worst |delta| / bound = {w:.3f}")
        assert w <= 1.0


# scripts/bench_vr.py's window: n_fft 2048 (1024 bins), 768 frames.  nets_61968KB (stage 3, 64 channels) and nets_new with nout 48
CONV_PROD = [
    (1, 1024, 768, 32, 64, 3, "leaky", 1, 1, 1, True, 64, 0),          # stg3 enc1.conv1
    (1, 1024, 768, 64, 64, 3, "leaky", 2, 1, 1, True, 64, 0),          # stg3 enc1.conv2
    (1, 1024, 768, 192, 64, 3, "relu", 1, 1, 1, True, 64, 0),          # stg3 dec1 over the concatenated (unfused) input
    (1, 64, 48, 512, 512, 1, "relu", 1, 0, 1, True, 2560, 512),        # stg3 aspp.conv2 into its slice of the 5 x 512 tensor
    (1, 1024, 768, 64, 2, 1, "none", 1, 0, 1, False, 2, 0),            # out
    (1, 1024, 768, 145, 48, 3, "relu", 1, 1, 1, True, 48, 0),          # nets_new stg3 dec1: 3 nout + 1
    (1, 64, 48, 384, 384, 3, "relu", 1, (12, 6), (12, 6), True, 1920, 1536),   # nets_new stg3 aspp.conv5
    (1, 1024, 768, 38, 48, 3, "relu", 1, 1, 1, True, 48, 0),           # nets_new stg3 enc1: 3 nout / 4 + 2
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(len(CONV_PROD)))
def test_conv_h_production_shapes(gpu_ctx, case):
    B, H, W, cin, cout, k, act, stride, pad, dil, y_f16, ct, c0 = CONV_PROD[case]
    bands = None if H <= 64 else 6
    w = run_conv_h(gpu_ctx, B, H, W, cin, cout, k, act, stride, pad, dil, y_f16, ct, c0, seed=100 + case, bands=bands)
    print(f"production conv {CONV_PROD[case]}: worst |delta| / bound = {w:.3f}")
    assert w <= 1.0


def small_ops(dev, B, H, W, C, d, seed):
    """depthwise, mean, resize, copy on one random half tensor: worst |delta| / bound of each"""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(B, H, W, C, generator=g) * 2).half()
    dw = (torch.randn(C, 3, 3, generator=g) / 3).half()
    xd, wd = on(dev, x), on(dev, dw)
    res = {}
    y = on(dev, torch.zeros(B, H, W, C, dtype=torch.float16))
    dev.check(dev.lib.alsep_vr_depthwise_h(dev.handle, _lib.ptr(xd), _lib.ptr(wd), _lib.ptr(y), B, H, W, C, 3, 3, d, d), "alsep_vr_depthwise_h")
    v, a = vo.depthwise_value(x, dw, d)
    res["depthwise"] = worst(host(y), v.numpy(), vo.out_bound(v.numpy(), a))
    y = on(dev, torch.zeros(B, 1, W, C, dtype=torch.float16))
    dev.check(dev.lib.alsep_vr_mean_hh(dev.handle, _lib.ptr(xd), _lib.ptr(y), B, H, W, C), "alsep_vr_mean_hh")
    v, a = vo.mean_value(x)
    res["mean"] = worst(host(y), v.numpy(), vo.out_bound(v.numpy(), a))
    ho, wo, ct, c0 = 2 * H, 2 * W, C + 5, 3
    y = on(dev, torch.zeros(B, ho, wo, ct, dtype=torch.float16))
    dev.check(dev.lib.alsep_vr_resize_bilinear_h(dev.handle, _lib.ptr(xd), _lib.ptr(y), B, H, W, C, ho, wo, ct, c0), "alsep_vr_resize_bilinear_h")
    v, a = vo.resize_value(x, ho, wo)
    got = host(y)
    assert not np.any(got[..., :c0]) and not np.any(got[..., c0 + C:])
    res["resize"] = worst(got[..., c0:c0 + C], v.numpy(), vo.out_bound(v.numpy(), a))
    assert np.array_equal(got[..., c0:c0 + C].astype(np.float64), vo.resize_device(x, ho, wo).numpy()), "the oracle's float32 restatement of the resize"
    wy, off = W - 3, 1                                                          # an odd crop offset
    y = on(dev, torch.zeros(B, H, wy, ct, dtype=torch.float16))
    dev.check(dev.lib.alsep_vr_copy_slice_h(dev.handle, _lib.ptr(xd), _lib.ptr(y), B * H, W, C, off, wy, ct, c0), "alsep_vr_copy_slice_h")
    got = host(y)
    assert np.array_equal(got[..., c0:c0 + C], x[:, :, off:off + wy].numpy()) and not np.any(got[..., :c0]) and not np.any(got[..., c0 + C:])
    res["copy"] = 0.0
    return res


@pytest.mark.parametrize("B,H,W,C,d", [(2, 9, 7, 5, 4), (1, 20, 11, 16, 16), (2, 6, 10, 24, 8)])
def test_small_kernels_vs_float64(dev, B, H, W, C, d):
    res = small_ops(dev, B, H, W, C, d, seed=B + H)
    print(f"small kernels {B}x{H}x{W}x{C} dilation {d}: worst |delta| / bound {res}")
    assert all(v <= 1.0 for v in res.values())


@pytest.mark.gpu
def test_small_kernels_production_shapes(gpu_ctx):
    res = small_ops(gpu_ctx, 1, 64, 48, 512, 16, seed=7)                        # the ASPP level of stg3 at the production window
    print(f"small kernels 1x64x48x512: worst |delta| / bound {res}")
    assert all(v <= 1.0 for v in res.values())


# ---- 2. fused decoder input = unfused half path --------------------------------------------------------------------------------------------
def decoder_both(dev, B, hu, wu, cu, ws, cs, cout, seed):
    """the same decoder layer through alsep_vr_decoder_conv_h and through resize + copy + conv; also the float64 check of the fused one"""
    from audiolab_amd.vrnet import VRNet, _Conv
    sd, ora, g = make_conv(cu + cs, cout, 3, "relu", 1, 1, 1, seed)
    x = (torch.randn(B, hu, wu, cu, generator=g) * 1.5).half()
    skip = (torch.randn(B, 2 * hu, ws, cs, generator=g) * 1.5).half()
    net = VRNet.__new__(VRNet)                                                  # the layer methods without a network around them
    net.ctx = dev
    net._set_precision("f16", None)
    L = _Conv(dev, sd, "c.weight", "bn", "relu", 1, 1, 1, precision="f16")
    xd, sk = on(dev, x), on(dev, skip)
    fused = host(net._decoder(L, xd, sk))
    net.fuse_decoder = False
    plain = host(net._decoder(L, xd, sk))
    return fused, plain, ora, x, skip


@pytest.mark.parametrize("B,hu,wu,cu,ws,cs,cout", [
    (2, 5, 6, 16, 12, 8, 8),            # vector staging, no crop
    (1, 4, 5, 24, 13, 16, 40),          # vector staging, odd crop offset (13 - 10) // 2 = 1
    (2, 3, 4, 9, 11, 4, 4),             # element staging (nets_new dec1: 2 nout + 1), odd crop offset
    (1, 6, 3, 8, 9, 8, 136),            # more than one channel tile, crop 1
])
def test_fused_decoder_equals_unfused(dev, B, hu, wu, cu, ws, cs, cout):
    fused, plain, ora, x, skip = decoder_both(dev, B, hu, wu, cu, ws, cs, cout, seed=cu)
    assert np.array_equal(fused, plain), f"fused and unfused differ in {np.count_nonzero(fused != plain)} of {fused.size} values"
    a = vo.decoder_input(x, skip)
    w = worst(fused, ora.value(a).numpy(), vo.out_bound(ora.value(a).numpy(), ora.arith(a)))
    print(f"fused decoder {B}x{hu}x{wu} {cu}+{cs}->{cout}: worst |delta| / bound = {w:.3f}")
    assert w <= 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("B,hu,wu,cu,ws,cs,cout", [
    (1, 512, 384, 128, 768, 64, 64),    # nets_61968KB stg3 dec1
    (1, 256, 192, 256, 387, 128, 128),  # stg3 dec2 with a skip three frames wider: crop offset 1
    (1, 512, 384, 97, 768, 48, 48),     # nets_new stg3 dec1 (element staging)
    (1, 64, 40, 512, 83, 512, 512),     # stg3 dec4, crop offset 1
])
def test_fused_decoder_equals_unfused_production(gpu_ctx, B, hu, wu, cu, ws, cs, cout):
    fused, plain, *_ = decoder_both(gpu_ctx, B, hu, wu, cu, ws, cs, cout, seed=cu)
    assert np.array_equal(fused, plain), f"fused and unfused differ in {np.count_nonzero(fused != plain)} of {fused.size} values"


# ---- the five fixture cases ----------------------------------------------------------------------------------------------------------------
CASES = ["c0", "c1", "c2", "n0", "n1"]


def load_case(golden_dir, case):
    """(kind, state_dict, net kwargs, x, aggressiveness, the reference module's float32 output)"""
    from audiolab_amd.vrnet import WIDTHS, random_state_dict, random_state_dict_new
    z = np.load(os.path.join(golden_dir, "vrnet.npz"))
    if case[0] == "c":
        n_fft, frames, seed, split = (int(v) for v in z[f"{case}_cfg"])
        aggr = None if split < 0 else {"split_bin": split, "value": float(z[f"{case}_aggr"][0])}
        variant = str(z[f"{case}_variant"])
        return "old", random_state_dict(WIDTHS[variant], seed=seed), dict(n_fft=n_fft, variant=variant), z[f"{case}_x"], aggr, z[f"{case}_y"]
    n_fft, nout, nout_lstm, frames, seed = (int(v) for v in z[f"{case}_cfg"])
    return ("new", random_state_dict_new(n_fft, nout, nout_lstm, seed=seed), dict(n_fft=n_fft, nout=nout, nout_lstm=nout_lstm), z[f"{case}_x"],
            None, z[f"{case}_y"])


def build(dev, kind, sd, kw, precision="f16", trace=None):
    from audiolab_amd.vrnet import VRNet, VRNetNew
    if kind == "old":
        return VRNet(kw["n_fft"], sd, variant=kw["variant"], ctx=dev, precision=precision, trace=trace)
    return VRNetNew(kw["n_fft"], sd, nout=kw["nout"], nout_lstm=kw["nout_lstm"], ctx=dev, precision=precision, trace=trace)


def oracle_forward(kind, sd, kw, x, aggr):
    from audiolab_amd.vrnet import WIDTHS
    if kind == "old":
        return vo.vrnet_forward(sd, WIDTHS[kw["variant"]], kw["n_fft"], x, aggr)
    return vo.vrnet_new_forward(sd, kw["n_fft"], x)


# ---- 3. every layer on its own input ---------------------------------------------------------------------------------------------------------
def layer_report(dev, kind, sd, kw, x, aggr, spoil=None):
    """one traced f16 forward; {layer name: worst |device - float64| / bound over its calls}, each layer recomputed from the inputs the
    device network had.  ``spoil(net)`` changes the device network after construction."""
    from audiolab_amd.vrnet import WIDTHS
    calls = []

    def trace(name, layer_kind, inputs, out):
        cp = lambda t: t.detach().cpu().clone() if isinstance(t, torch.Tensor) else t
        calls.append((name, layer_kind, tuple(cp(t) for t in inputs), cp(out)))
    net = build(dev, kind, sd, kw, trace=trace)
    if spoil is not None:
        spoil(net)
    net.forward(torch.from_numpy(x), aggr)
    convs = vo.build_vrnet(sd, WIDTHS[kw["variant"]])[0] if kind == "old" else vo.build_vrnet_new(sd)
    report = {}
    for name, layer_kind, inputs, out in calls:
        y_f16 = out.dtype == torch.float16
        got = out.double().numpy()
        if layer_kind in ("conv", "decoder"):
            a = inputs[0].double() if layer_kind == "conv" else vo.decoder_input(inputs[0], inputs[1])
            ref, arith = convs[name].value(a).numpy(), convs[name].arith(a)
        elif layer_kind == "depthwise":
            assert np.array_equal(inputs[1].double().numpy(), vo.r16(sd[name + ".weight"].float().reshape(-1, 3, 3)).numpy())
            v, arith = vo.depthwise_value(inputs[0], inputs[1], inputs[2])
            ref = v.numpy()
        elif layer_kind == "mean":
            v, arith = vo.mean_value(inputs[0])
            ref = v.numpy()
        elif layer_kind == "resize":
            v, arith = vo.resize_value(inputs[0], out.shape[1], out.shape[2])
            ref = v.numpy()
        else:
            assert layer_kind == "lstm"
            ref, arith = vo.lstm_value(sd, name[:-len(".lstm_dec2.lstm")], inputs[0]).numpy(), vo.LSTM_ARITH
        report[name] = max(report.get(name, 0.0), worst(got, ref, vo.out_bound(ref, arith, y_f16)))
    return net, report


@pytest.mark.parametrize("case", CASES)
def test_every_layer_on_its_own_input(dev, golden_dir, case):
    kind, sd, kw, x, aggr, _ = load_case(golden_dir, case)
    net, report = layer_report(dev, kind, sd, kw, x, aggr)
    assert set(report) == set(net.layers) and len(net.layers) == len(set(net.layers)), set(net.layers) ^ set(report)
    kinds = {"old": 4 * (8 + 6 + 4 + 3 + 2) + 3, "new": 5 * (9 + 6 + 4 + 1 + 3) + 3}    # convs + ASPP + decoders (+ LSTM conv), dw / pool / resize
    assert len(report) == kinds[kind]
    bad = {n: round(v, 3) for n, v in report.items() if v > 1.0}
    print(f"{case}: {len(report)} layers, worst |delta| / bound = {max(report.values()):.3f} ({max(report, key=report.get)})")
    assert not bad, bad


# ---- 5. a wrong kernel is caught ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_a_wrong_shift_fails_its_layer_only(dev, golden_dir, case):
    kind, sd, kw, x, aggr, _ = load_case(golden_dir, case)

    def spoil(net):
        L = (net.nets if kind == "old" else net.base)["stg3_full_band_net"]["dec1"]
        L.shift.mul_(1.05)
    net, report = layer_report(dev, kind, sd, kw, x, aggr, spoil)
    name = "stg3_full_band_net.dec1.conv.conv.0" if kind == "old" else "stg3_full_band_net.dec1.conv1.conv.0"
    bad = {n for n, v in report.items() if v > 1.0}
    assert bad == {name}, bad


# ---- 4. the whole network against the reference's own outputs ----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_whole_network_vs_reference_outputs(dev, golden_dir, case):
    """rel. L2 to the float32 output of the reference module below twice the distance of the float64 restatement from it: one part is the
    rounding itself, the other the accumulation order (0.5 to 0.7 of the first between torch's float32 and float64 convolutions)"""
    kind, sd, kw, x, aggr, want = load_case(golden_dir, case)
    got = build(dev, kind, sd, kw).forward(torch.from_numpy(x), aggr)
    ora = oracle_forward(kind, sd, kw, x, aggr)
    d_ora, d_dev = vo.rel(ora, want), vo.rel(host(got), want)
    peak = float(np.max(np.abs(host(got) - want)))
    print(f"{case}: restatement vs reference {d_ora:.3e}, device vs reference {d_dev:.3e} (max abs {peak:.3e}, peak {np.max(np.abs(want)):.2f}), "
          f"device vs restatement {vo.rel(host(got), ora):.3e}")
    assert got.dtype == torch.float32 and got.shape == want.shape
    assert d_ora < 2e-3, "the fixture is not well conditioned in half"
    assert d_dev < 2.0 * d_ora


# ---- 7. default untouched ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_default_precision_is_the_parent_commits(emul, golden_dir, case):
    """SHA-256 of the float32 outputs on the emulated kernels, recorded on the commit before the half mode existed"""
    kind, sd, kw, x, aggr, want = load_case(golden_dir, case)
    net = build(emul, kind, sd, kw, precision="f32")
    assert net.precision == "f32" and not net.half
    got = np.ascontiguousarray(net.forward(torch.from_numpy(x), aggr).numpy())
    recorded = json.load(open(os.path.join(golden_dir, "vrnet_default_sha256.json")))
    assert hashlib.sha256(got.tobytes()).hexdigest() == recorded[case]


def test_precision_is_validated(emul):
    from audiolab_amd._lib import AlsepError
    from audiolab_amd.vrnet import WIDTHS, VRNet, random_state_dict
    with pytest.raises(AlsepError):
        VRNet(128, random_state_dict(WIDTHS["nets"], seed=1), variant="nets", ctx=emul, precision="bf16")


# ---- 6. runner and engine ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,tta,aggr", [("plain", False, None), ("tta", True, {"split_bin": 12, "value": 0.2})])     # as the fixture was made
def test_runner_in_half(dev, golden_dir, tag, tta, aggr):
    from audiolab_amd.vrnet import WIDTHS, VRNet, random_state_dict, vr_inference
    z = np.load(os.path.join(golden_dir, "vrnet.npz"))
    sd = random_state_dict(WIDTHS["nets"], seed=21)
    net = VRNet(64, sd, variant="nets", ctx=dev, precision="f16")
    net.offset = 8
    pred, mag, phase = vr_inference(net, torch.from_numpy(z["inf_x"]), aggr, window_size=48, tta=tta, max_batch=3)
    want = z[f"inf_{tag}_pred"]
    ora = vo.inference(lambda w: vo.vrnet_forward(sd, WIDTHS["nets"], 64, w, aggr), z["inf_x"], 48, 8, tta)
    d_ora, d_dev = vo.rel(ora, want), vo.rel(host(pred), want)
    print(f"runner {tag}: restatement vs reference {d_ora:.3e}, device vs reference {d_dev:.3e}")
    assert pred.shape == want.shape and net._twin is None
    assert d_ora < 2e-3 and d_dev < 2.0 * d_ora
    assert float(np.max(np.abs(host(mag) - z["inf_mag"]))) < 1e-6


def test_runner_redoes_a_non_finite_batch_in_float32(dev, golden_dir, caplog):
    """the first BatchNorm's weight times 1e6 and the next convolution's weights times 1e-6: finite in float32, beyond 65504 in half"""
    from audiolab_amd.vrnet import WIDTHS, VRNet, random_state_dict, vr_inference
    z = np.load(os.path.join(golden_dir, "vrnet.npz"))
    sd = random_state_dict(WIDTHS["nets"], seed=21)
    sd["stg1_low_band_net.enc1.conv1.conv.1.weight"] = sd["stg1_low_band_net.enc1.conv1.conv.1.weight"] * 1e6
    sd["stg1_low_band_net.enc1.conv2.conv.0.weight"] = sd["stg1_low_band_net.enc1.conv2.conv.0.weight"] * 1e-6
    x = torch.from_numpy(z["inf_x"])
    f32 = VRNet(64, sd, variant="nets", ctx=dev)
    f32.offset = 8
    want, *_ = vr_inference(f32, x, None, window_size=48, max_batch=3)
    assert bool(torch.isfinite(want).all())
    net = VRNet(64, sd, variant="nets", ctx=dev, precision="f16")
    net.offset = 8
    assert net._twin is None                                                    # built on first use
    with caplog.at_level(logging.WARNING):
        got, *_ = vr_inference(net, x, None, window_size=48, max_batch=3)
    assert any("not finite" in r.getMessage() and r.levelno == logging.WARNING for r in caplog.records)
    assert net._twin is not None and net._twin.precision == "f32"
    assert bool(torch.isfinite(got).all()) and torch.equal(got, want)


def test_engine_option(dev, tmp_path):
    from audiolab_amd._lib import AlsepError
    from audiolab_amd.engine import Separator
    sep = Separator(model_file_dir=str(tmp_path), ctx=dev, allow_synthetic=True, vr_precision="f16")
    sep.load_model("UVR-DeNoise-Lite.pth")
    net = sep.model_instance.vr.net
    assert net.precision == "f16" and net.out.w.dtype == torch.float16 and net.out.scale.dtype == torch.float32
    sep = Separator(model_file_dir=str(tmp_path), ctx=dev, allow_synthetic=True)
    assert sep.vr_precision == "f32"
    sep.load_model("UVR-DeNoise-Lite.pth")
    assert sep.model_instance.vr.net.precision == "f32" and sep.model_instance.vr.net.out.w.dtype == torch.float32
    assert Separator(model_file_dir=str(tmp_path), ctx=dev, use_autocast=True).vr_precision == "f32"     # autocast does not select it
    with pytest.raises(AlsepError):
        Separator(model_file_dir=str(tmp_path), ctx=dev, vr_precision="bf16")


def test_wrapper_takes_it_through_engine_options_only():
    from audiolab_amd.wrappers.separate import Separate
    assert "vr_precision" not in Separate.allowed_kwargs and "vr_precision" not in Separate.ENGINE_KNOBS
    import inspect
    from audiolab_amd.separator import stem_separator
    assert '"vr_precision": kwargs.get("vr_precision", "f32")' in inspect.getsource(stem_separator.separate_music)


# ---- GPU: launches, full size ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind,decoders", [("old", 16), ("new", 20)])
def test_f16_forward_launches_one_convolution_per_decoder(gpu_ctx, kind, decoders):
    from audiolab_amd.vrnet import WIDTHS, VRNet, VRNetNew, random_state_dict, random_state_dict_new
    ctx = gpu_ctx
    if kind == "old":
        net = VRNet(256, random_state_dict(WIDTHS["nets"], seed=3), variant="nets", ctx=ctx, precision="f16")
    else:
        net = VRNetNew(256, random_state_dict_new(256, 16, 64, seed=3), nout=16, nout_lstm=64, ctx=ctx, precision="f16")
    x = torch.rand((1, 129, 64, 2), device="cuda")
    ctx.launch_counts_reset()
    y = net.forward_nhwc(x)
    assert bool(torch.isfinite(y).all())
    bases = 4 if kind == "old" else 5
    assert ctx.launch_count("vr_decoder_conv_h_kernel") == decoders
    assert ctx.launch_count("vr_resize_kernel") == 0 and ctx.launch_count("vr_copy_slice_kernel") == 0
    assert ctx.launch_count("vr_resize_h_kernel") == bases                      # the ASPP pooled branch only
    assert ctx.launch_count("vr_copy_slice_h_kernel") == (4 if kind == "old" else 0)     # the two cascade concatenations
    convs = (4 * 14 + 3) if kind == "old" else (5 * 16 + 3)
    assert ctx.launch_count("vr_conv_h_kernel") == convs
    net.fuse_decoder = False
    ctx.launch_counts_reset()
    y2 = net.forward_nhwc(x)
    assert ctx.launch_count("vr_decoder_conv_h_kernel") == 0 and ctx.launch_count("vr_conv_h_kernel") == convs + decoders
    assert torch.equal(y, y2)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["17_HP-Wind_Inst-UVR.pth", "UVR-DeNoise-Lite.pth", "UVR-BVE-4B_SN-44100-1.pth"])
def test_engine_full_size_f16_vs_float32(gpu_ctx, tmp_path, name):
    """The roster's VR entries at their real size through Separator(vr_precision="f16") on the input of
    tests/test_vr_frontend.py::test_engine_runs_vr_models_full_size: finite, the two stems sum to the recombined mix as in float32, and
    each stem within 1e-2 rel. L2 of the float32 engine's (ten times the worst rounding distance of the small cases; the front and back
    end are float32 in both runs).  Measured: profiles/vr_half_accuracy.txt."""
    from audiolab_amd.engine import Separator
    from oracle.toy import synth_mix
    from audiolab_amd.vr_frontend import VRFrontEnd
    n = 44100 * 8 + 321
    wave = synth_mix(n, seed=17)
    outs = {}
    for prec in ("f32", "f16"):
        sep = Separator(model_file_dir=str(tmp_path), ctx=gpu_ctx, allow_synthetic=True, vr_precision=prec)
        sep.load_model(name)
        assert sep.model_instance.vr.net.precision == prec
        outs[prec] = {k: host(v) for k, v in sep.separate_array(wave).items()}
        assert sep.model_instance.vr.net._twin is None                          # no float32 re-run
    labels = sep.roster[name][2]["labels"]
    a, b = outs["f16"][labels[0]], outs["f16"][labels[1]]
    assert a.shape == b.shape == (2, n) and np.isfinite(a).all() and np.isfinite(b).all()
    f = VRFrontEnd(sep.roster[name][1]["params"], gpu_ctx)
    X, _ = f.analyse(on(gpu_ctx, wave))
    whole = host(f.synthesise(X))
    assert np.max(np.abs(a[:, :whole.shape[1]] + b[:, :whole.shape[1]] - whole)) < 1e-4 * max(1.0, float(np.max(np.abs(whole))))
    for label in labels:
        d = vo.rel(outs["f16"][label], outs["f32"][label])
        print(f"{name} {label}: f16 engine vs float32 engine rel. L2 {d:.3e}")
        assert d < 1e-2
