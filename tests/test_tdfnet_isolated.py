"""Each half-precision TFC-TDF kernel alone, at its production place and shape, against a tight oracle.

The full-size bf16 / f16 tests compare a random network whose 40 layers amplify one flipped rounding about 100x, so their
bounds are loose.  Here the network is structured (oracle/tdfnet_structured.py): every layer except one TARGET passes its
input through exactly, so the GPU forward differs from the storage oracle only where the target and the final 1x1
projection sum in another order.  Every case runs TDFNet.forward_nhwc at the bench geometry (A) or the kuielab geometry
(B) with the default dispatch, asserts by launch count that the intended kernel ran, and bounds
  - per (window, frame) row: max over rows of |got - want| / |want|;
  - per element: |got - want| <= a * (ulp(|want|) + ulp(rms(want))), ulp of the storage type.
All-passthrough networks on integer data are exact in any summation order: those forwards must be bit-identical.

The GPU cases compare against the storage oracle computed in float64 between the stores (on the GPU, for time): the
float32 oracle's own summation error is of the size of the kernels' (f16 level-2 TDF: 4.3e-4 per row, 4.8 ulp, all of it
the float32 oracle's), so bounds set against it would measure the oracle.

GPU (-m gpu): the case matrix.  CPU (-m "not gpu"): the same bounds against defects a kernel could plausibly have, oracle
against oracle at the same geometries; and one-block networks at the shapes of levels 3-5, all-passthrough, on the
emulated kernel sources (and on the GPU, through the ``dev`` fixture).
"""
import time

import pytest
import torch

from audiolab_amd.tdfnet import TDFNetConfig
from oracle import tdfnet_oracle
from oracle.tdfnet_structured import block_name, integer_input, structured_state_dict, target_layer

GEOM = {"A": TDFNetConfig(),                                                    # the bench's: 3072 x 256, g 48, L 11, bn 8
        "B": TDFNetConfig(dim_f=2048, dim_t=128, n_fft=4096, hop=1024)}        # kuielab: level 0 F % 48 != 0
DT = {"bf16": torch.bfloat16, "f16": torch.float16}
MANT = {"bf16": 7, "f16": 10}                                                   # explicit mantissa bits
SEL_SCALE = 0.5                                                                 # f16: skip products at the bench depth stay < 65504

# kernel (launch-count name) per kind and level, and its launches per forward, at the default dispatch
CONV_A = ["conv3x3_bf16_m0_kernel", "conv3x3_bf16_mq_kernel", "conv3x3_bf16_big_kernel<3>", "conv3x3_bf16_kernel<64>",
          "conv3x3_bf16_kernel<64>", "conv3x3_bf16_kernel<small>"]
TDF_A = [("tdf_bf16_wide_kernel<nores>", "tdf_bf16_wide_kernel<res>")] * 2 + [("tdf_bf16_kernel",)] * 4
DS_A = ["ds48_stream_kernel", "ds_split_stream_kernel<96>", "ds_split_stream_kernel<144>", "pix_gemm_kernel", "pix_gemm_kernel"]
US_A = ["us_stream_kernel<96,48>", "us_stream_kernel<144,96>", "us_stream_kernel<192,144>", "pix_gemm_kernel", "pix_gemm_kernel"]
COUNTS_A = {"conv3x3_bf16_m0_kernel": 6, "conv3x3_bf16_mq_kernel": 6, "conv3x3_bf16_big_kernel<3>": 6,
            "conv3x3_bf16_kernel<64>": 12, "conv3x3_bf16_kernel<small>": 3, "tdf_bf16_wide_kernel<nores>": 4,
            "tdf_bf16_wide_kernel<res>": 4, "tdf_bf16_kernel": 14, "ds_stream_kernel": 3, "us_stream_kernel": 3,
            "pix_gemm_kernel": 4, "ds48_stream_kernel": 1, "ds_split_stream_kernel<96>": 1, "ds_split_stream_kernel<144>": 1,
            "us_stream_kernel<96,48>": 1, "us_stream_kernel<144,96>": 1, "us_stream_kernel<192,144>": 1}
COUNTS_B = {"conv3x3_bf16_regw_kernel": 6, "conv3x3_bf16_mq_kernel": 6, "conv3x3_bf16_kernel<64>": 21, "tdf_bf16_kernel": 22,
            "ds_stream_kernel": 3, "us_stream_kernel": 3, "pix_gemm_kernel": 4}     # B = 1 (level 2: 32 tiles < 96, plain kernel)


def kernels_of(geom, kind, k):
    if geom == "B":
        return {"conv": ["conv3x3_bf16_regw_kernel", "conv3x3_bf16_mq_kernel"] + ["conv3x3_bf16_kernel<64>"] * 4,
                "tdf": [("tdf_bf16_kernel",)] * 6}[kind][k] if kind in ("conv", "tdf") else None
    if kind == "conv":
        return CONV_A[k]
    if kind == "tdf":
        return TDF_A[k]
    return DS_A[k] if kind == "ds" else US_A[k]


class Case:
    def __init__(self, storage, geom, target, batch, windows, branch):
        self.storage, self.geom, self.target, self.batch, self.windows, self.branch = storage, geom, target, batch, windows, branch
        t = "pass" if target is None else f"{target[0]}{target[1]}"
        self.id = f"{storage}-{geom}-{t}-{branch}-B{batch}"


# (kind, level, batch, compared windows, branch of the launcher that this batch takes)
_A_CELLS = [
    ("conv", 0, 1, [0], "m0"), ("conv", 1, 1, [0], "mq_partial_round"), ("conv", 1, 2, [1], "mq_full_rounds"),
    ("conv", 2, 1, [0], "big3_one_round"), ("conv", 2, 3, [2], "big3_partial_round"), ("conv", 3, 1, [0], "c64_nyfast"),
    ("conv", 4, 1, [0], "c64_nyfast_off"), ("conv", 4, 2, [1], "c64_nyfast"), ("conv", 5, 1, [0], "small_nyfast_off"),
    ("conv", 5, 8, [7], "small_nyfast"),
    ("tdf", 0, 1, [0], "wide8_nores_wide4_res_yfast"), ("tdf", 1, 1, [0], "wide4_yfast"), ("tdf", 2, 1, [0], "tdf_m96"),
    ("tdf", 3, 1, [0], "tdf_m48"), ("tdf", 4, 1, [0], "tdf_m24"), ("tdf", 5, 1, [0], "tdf_m12"),
    ("ds", 0, 1, [0], "ds48"), ("ds", 1, 1, [0], "ds_split96_partial_round"), ("ds", 1, 2, [1], "ds_split96_full_rounds"),
    ("ds", 2, 1, [0], "ds_split144_one_round"), ("ds", 2, 3, [2], "ds_split144_partial_round"), ("ds", 3, 1, [0], "pix_gemm"),
    ("ds", 4, 1, [0], "pix_gemm"),
    ("us", 0, 1, [0], "us96_48"), ("us", 1, 1, [0], "us144_96"), ("us", 2, 1, [0], "us192_144_partial_round"),
    ("us", 2, 2, [1], "us192_144_full_rounds"), ("us", 3, 1, [0], "pix_gemm"), ("us", 4, 1, [0], "pix_gemm"),
]
_F16_A = [c for c in _A_CELLS if c[2] == 1 and (c[1] <= 2 or (c[0] in ("conv", "tdf") and c[1] == 5))]
_B_CELLS = [("conv", 0, 1, [0], "regw"), ("tdf", 0, 1, [0], "tdf_m256")]

CASES = ([Case("bf16", "A", (k, l), b, w, br) for k, l, b, w, br in _A_CELLS]
         + [Case("f16", "A", (k, l), b, w, br) for k, l, b, w, br in _F16_A]
         + [Case(s, "B", (k, l), b, w, br) for s in ("bf16", "f16") for k, l, b, w, br in _B_CELLS])
PASS_CASES = [Case(s, g, None, 1, [0], "all") for g in ("A", "B") for s in ("bf16", "f16")]

# (row bound, element bound a): 2x what the kernels measured on an MI355X against the float64 oracle (the table that
# -m gpu -s prints), rounded up;
# floors 1e-4 (bf16) / 2e-5 (f16) on the row metric and 1 ulp on the element metric
BOUNDS = {
    "bf16-A-conv0-m0-B1": (0.00028, 1.4),
    "bf16-A-conv1-mq_partial_round-B1": (0.00031, 1.4),
    "bf16-A-conv1-mq_full_rounds-B2": (0.00042, 1.4),
    "bf16-A-conv2-big3_one_round-B1": (0.00048, 1.4),
    "bf16-A-conv2-big3_partial_round-B3": (0.00045, 1.6),
    "bf16-A-conv3-c64_nyfast-B1": (0.00055, 1.6),
    "bf16-A-conv4-c64_nyfast_off-B1": (0.0011, 1.6),
    "bf16-A-conv4-c64_nyfast-B2": (0.00046, 1.8),
    "bf16-A-conv5-small_nyfast_off-B1": (0.00029, 1.6),
    "bf16-A-conv5-small_nyfast-B8": (0.00039, 1.6),
    "bf16-A-tdf0-wide8_nores_wide4_res_yfast-B1": (0.0015, 4),
    "bf16-A-tdf1-wide4_yfast-B1": (0.00046, 1.8),
    "bf16-A-tdf2-tdf_m96-B1": (0.00028, 1.4),
    "bf16-A-tdf3-tdf_m48-B1": (0.00021, 1.6),
    "bf16-A-tdf4-tdf_m24-B1": (0.0001, 1.4),
    "bf16-A-tdf5-tdf_m12-B1": (0.0001, 1),
    "bf16-A-ds0-ds48-B1": (0.00037, 1.6),
    "bf16-A-ds1-ds_split96_partial_round-B1": (0.00089, 1.8),
    "bf16-A-ds1-ds_split96_full_rounds-B2": (0.0005, 1.6),
    "bf16-A-ds2-ds_split144_one_round-B1": (0.0013, 1.8),
    "bf16-A-ds2-ds_split144_partial_round-B3": (0.00057, 1.8),
    "bf16-A-ds3-pix_gemm-B1": (0.00085, 1.8),
    "bf16-A-ds4-pix_gemm-B1": (0.0004, 1.8),
    "bf16-A-us0-us96_48-B1": (0.00035, 1.6),
    "bf16-A-us1-us144_96-B1": (0.00018, 1.4),
    "bf16-A-us2-us192_144_partial_round-B1": (0.0011, 1.9),
    "bf16-A-us2-us192_144_full_rounds-B2": (0.00013, 1.4),
    "bf16-A-us3-pix_gemm-B1": (0.00041, 1.4),
    "bf16-A-us4-pix_gemm-B1": (0.0006, 1.6),
    "f16-A-conv0-m0-B1": (6.8e-05, 1.6),
    "f16-A-conv1-mq_partial_round-B1": (7.3e-05, 1.6),
    "f16-A-conv2-big3_one_round-B1": (0.00011, 1.8),
    "f16-A-conv5-small_nyfast_off-B1": (0.0002, 2),
    "f16-A-tdf0-wide8_nores_wide4_res_yfast-B1": (0.00013, 4),
    "f16-A-tdf1-wide4_yfast-B1": (0.00037, 5.4),
    "f16-A-tdf2-tdf_m96-B1": (0.00015, 2),
    "f16-A-tdf5-tdf_m12-B1": (0.00013, 1.8),
    "f16-A-ds0-ds48-B1": (7.1e-05, 2),
    "f16-A-ds1-ds_split96_partial_round-B1": (0.00014, 1.8),
    "f16-A-ds2-ds_split144_one_round-B1": (0.00023, 1.9),
    "f16-A-us0-us96_48-B1": (8.8e-05, 1.8),
    "f16-A-us1-us144_96-B1": (0.00025, 2),
    "f16-A-us2-us192_144_partial_round-B1": (0.00021, 1.9),
    "bf16-B-conv0-regw-B1": (0.00042, 1.4),
    "bf16-B-tdf0-tdf_m256-B1": (0.00034, 1.6),
    "f16-B-conv0-regw-B1": (7.1e-05, 1.6),
    "f16-B-tdf0-tdf_m256-B1": (0.00013, 1.8),
}


def ulp(v: torch.Tensor, storage: str) -> torch.Tensor:
    _, e = torch.frexp(v.abs().double())
    return torch.ldexp(torch.ones_like(v, dtype=torch.float64), (e - 1 - MANT[storage]).clamp(min=-24 if storage == "f16" else -133))


def metrics(got: torch.Tensor, want: torch.Tensor, storage: str):
    """-> (max per-(window, frame) row rel-L2, max element error in units of ulp(|want|) + ulp(rms(want))), layout [B,4,F,T]"""
    d = (got.double() - want.double())
    w = want.double()
    rows = d.pow(2).sum(dim=(1, 2)).sqrt() / w.pow(2).sum(dim=(1, 2)).sqrt().clamp(min=1e-300)
    rms = w.pow(2).mean().sqrt()
    elem = d.abs() / (ulp(w, storage) + ulp(rms.reshape(1), storage))
    return float(rows.max()), float(elem.max())


def oracle(sd, cfg, x, storage, target=None, perturb=None):
    """storage oracle on x [B,4,F,T]; with a target: also the fraction of exact zeros in its pre-store output"""
    name = None if target is None else target_layer(cfg, target)
    seen = {}

    def hook(n, y):
        if perturb is not None:
            y = perturb(n, y)
        if n == name or (target is not None and target[0] == "tdf" and n == name[:-1] + "0"):
            seen[n] = float((y == 0).double().mean())
        if target is not None and target[0] == "us" and n == f"{block_name(cfg, target[1])}.tdf.1":
            seen["skip"] = float((y == 0).double().mean())       # us: the skip multiply zeroes where its skip is zero
        return y
    with torch.no_grad():
        out = tdfnet_oracle.forward(sd, x, cfg.num_blocks, cfg.l, cfg.bn, storage=DT[storage], perturb=hook)
    return out.cpu(), seen


def case_input(cfg, case, seed=11):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn((case.batch, 4, cfg.dim_f, cfg.dim_t), generator=g)).to(DT[case.storage]).float()


def case_sd(cfg, case):
    return structured_state_dict(cfg, case.target, seed=3, sel_scale=SEL_SCALE if case.storage == "f16" else 1.0)


# ------------------------------------------------------------------------------------------------------------------------
# GPU: the case matrix
# ------------------------------------------------------------------------------------------------------------------------
_TABLE = []


@pytest.fixture(scope="module")
def ctx():
    from audiolab_amd import _lib
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    yield _lib.Context("cuda:0")
    if _TABLE:
        print("\nisolated-kernel cases: id | row rel-L2 (bound) | element ulps (bound) | target zeros | s")
        for r in _TABLE:
            print("  " + " | ".join(str(v) for v in r))


def run_gpu(ctx, cfg, sd, storage, x):
    from audiolab_amd.tdfnet import TDFNet
    net = TDFNet(cfg, sd, ctx=ctx, dtype=DT[storage], max_batch=x.shape[0])
    ctx.launch_counts_reset()
    got = net.forward_nhwc(x.permute(0, 3, 2, 1).contiguous().to(DT[storage]).cuda())
    torch.cuda.synchronize()
    del net
    return got.float().cpu().permute(0, 3, 2, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_isolated_kernel_vs_storage_oracle(ctx, case):
    t0 = time.time()
    cfg = GEOM[case.geom]
    sd = case_sd(cfg, case)
    x = case_input(cfg, case)
    got = run_gpu(ctx, cfg, sd, case.storage, x)
    kind, k = case.target
    counts = COUNTS_A if case.geom == "A" else COUNTS_B
    names = kernels_of(case.geom, kind, k)
    names = [names] if isinstance(names, str) else list(names)
    for nm in names:
        assert ctx.launch_count(nm) == counts[nm], (nm, ctx.launch_count(nm), counts[nm])
    if case.target == ("conv", 2) and case.batch == 1:
        assert ctx.launch_count("conv3x3_bf16_big_kernel<3>") == 6
    want, zeros = oracle(sd, cfg, x[case.windows].double().cuda(), case.storage, case.target)     # float64 between the stores
    row, elem = metrics(got[case.windows], want, case.storage)
    rb, eb = BOUNDS[case.id]
    _TABLE.append((case.id, f"{row:.2e} ({rb:.1e})", f"{elem:.2f} ({eb:.1f})", {n: round(z, 4) for n, z in zeros.items()},
                   f"{time.time() - t0:.1f}"))
    skip0 = zeros.pop("skip", 0.0)
    assert zeros and max(zeros.values()) <= skip0 + 0.01, (zeros, skip0)     # the target's ReLU hides almost nothing
    assert row < rb and elem < eb, (case.id, row, rb, elem, eb)


@pytest.mark.gpu
@pytest.mark.parametrize("case", PASS_CASES, ids=[c.id for c in PASS_CASES])
def test_all_passthrough_bit_identical(ctx, case):
    """every kernel's data movement in one forward: tiles, persistent rounds, ds / us channel maps, and -- the passthrough
    3x3 convs shifting by one frame / bin (SHIFT_TAPS) -- their halos and zero padding"""
    cfg = GEOM[case.geom]
    sd = structured_state_dict(cfg, None, final="dyadic", shift=True)
    x = integer_input(cfg, case.batch)
    got = run_gpu(ctx, cfg, sd, case.storage, x)
    want, _ = oracle(sd, cfg, x.double().cuda(), case.storage)
    want = want.float()
    assert want.abs().max() > 1 and float((want != 0).double().mean()) > 0.3
    assert torch.equal(got, want), (float((got != want).double().mean()), float((got - want).abs().max()))


# one-block networks at the shapes of levels 3, 4 and 5 of the bench network (channels, frames, bins; the first and final 1x1
# convs differ): the same conv / TDF dispatch, cheap enough for the emulated kernels
DEEP = [(192, 32, 384, "conv3x3_bf16_kernel<64>"), (240, 16, 192, "conv3x3_bf16_kernel<64>"), (288, 8, 96, "conv3x3_bf16_kernel<small>")]


@pytest.mark.parametrize("storage", ["bf16", "f16"])
@pytest.mark.parametrize("c,t,f,conv", DEEP, ids=["level3", "level4", "level5"])
def test_deep_level_shapes_passthrough_bit_identical(dev, storage, c, t, f, conv):
    """all-passthrough (shifting 3x3 convs, zero TDF) on integer data, B = 2: bit-identical on the emulated kernels (-m "not gpu")
    and on the GPU"""
    from audiolab_amd.tdfnet import TDFNet
    cfg = TDFNetConfig(dim_f=f, dim_t=t, g=c, num_blocks=1, n_fft=2 * f, hop=256)
    sd = structured_state_dict(cfg, None, final="dyadic", shift=True)
    x = integer_input(cfg, 2, seed=5)
    net = TDFNet(cfg, sd, ctx=dev, dtype=DT[storage], max_batch=2)
    dev.launch_counts_reset()
    got = net.forward_nhwc(x.permute(0, 3, 2, 1).contiguous().to(DT[storage]).to(dev.device)).float().cpu().permute(0, 3, 2, 1)
    assert dev.launch_count(conv) == 3 and dev.launch_count("tdf_bf16_kernel") == 2
    want, _ = oracle(sd, cfg, x, storage)
    assert float((want != 0).double().mean()) > 0.3
    assert torch.equal(got, want), (float((got != want).double().mean()), float((got - want).abs().max()))


# ------------------------------------------------------------------------------------------------------------------------
# CPU: the bounds reject defects a kernel could plausibly have (oracle against oracle, same geometry, same case)
# ------------------------------------------------------------------------------------------------------------------------
def _case(cid):
    return next(c for c in CASES if c.id == cid)


def _conv_defect(cfg, sd, case, defect, tile):
    """perturb hook: the target conv's output with one defect in one (TH x TW x all-channel) tile at (t0, f0), or its
    last partial persistent round (tiles >= n_full, row-major) left holding the buffer's stale content (the conv input)"""
    name = target_layer(cfg, case.target)
    prev = "first_conv" if case.target[1] == 0 else f"ds.{case.target[1] - 1}"
    q = name.replace(".tfc.0", ".tfc.H.0.0")
    (th, tw), (t0, f0) = tile
    dt = DT[case.storage]
    seen = {}

    def conv(x):
        return torch.relu(torch.nn.functional.conv2d(x, sd[q + ".weight"].to(dt).float(), sd[q + ".bias"], padding=1))

    def hook(n, y):
        if n == prev:
            seen["x"] = (y if n != "first_conv" else y.transpose(-1, -2)).to(dt).float()
        if n != name:
            return y
        y = y.clone()
        x = seen["x"]
        sl = (slice(None), slice(None), slice(t0, t0 + th), slice(f0, f0 + tw))
        if defect == "scale":
            y[sl] *= 1.01
        elif defect == "kslice":                                  # 16 input channels of one tile never accumulated
            xm = x.clone()
            xm[:, 16:32] = 0
            y[sl] = conv(xm)[sl]
        elif defect == "halo":                                    # the tile's upper halo row read one frame too early
            xh = x.clone()
            xh[:, :, t0 - 1] = x[:, :, t0 - 2]
            y[sl] = conv(xh)[sl]
        elif defect == "last_round":
            tiles_f = cfg.levels()[case.target[1]][2] // tw
            n_full = (y.shape[2] // th * tiles_f) // 256 * 256
            for tile_i in range(n_full, y.shape[2] // th * tiles_f):
                tt, tf = divmod(tile_i, tiles_f)
                s = (slice(None), slice(None), slice(tt * th, tt * th + th), slice(tf * tw, tf * tw + tw))
                y[s] = x[s]
        return y
    return hook


def _tile_scale(cfg, case, tile):
    name = target_layer(cfg, case.target)
    (th, tw), (t0, f0) = tile

    def hook(n, y):
        if n == name:
            y = y.clone()
            y[:, :, t0:t0 + th, f0:f0 + tw] *= 1.01
        return y
    return hook


def _reject(case, perturb_of):
    cfg = GEOM[case.geom]
    sd = case_sd(cfg, case)
    x = case_input(cfg, case)[case.windows]
    clean, _ = oracle(sd, cfg, x, case.storage)
    bad, _ = oracle(sd, cfg, x, case.storage, perturb=perturb_of(cfg, sd))
    row, elem = metrics(bad, clean, case.storage)
    rb, eb = BOUNDS[case.id]
    print(f"{case.id}: row {row:.2e} (bound {rb:.1e}), element {elem:.2f} ulp (bound {eb:.1f})")
    assert row > rb or elem > eb, (row, rb, elem, eb)


@pytest.mark.parametrize("defect", ["scale", "kslice", "halo", "last_round"])
def test_bounds_reject_conv_tile_defects(defect):
    """level-1 conv (conv3x3_bf16_mq_kernel, 8 x 64 tiles of 96 channels, 384 tiles at B = 1: a partial second round)"""
    case = _case("bf16-A-conv1-mq_partial_round-B1")
    _reject(case, lambda cfg, sd: _conv_defect(cfg, sd, case, defect, ((8, 64), (40, 640))))


@pytest.mark.parametrize("cid,tile", [("bf16-A-tdf0-wide8_nores_wide4_res_yfast-B1", ((4, 192), (100, 1536))),
                                      ("bf16-A-ds1-ds_split96_partial_round-B1", ((1, 64), (30, 256))),
                                      ("bf16-A-us2-us192_144_partial_round-B1", ((2, 64), (20, 128))),
                                      ("f16-A-conv0-m0-B1", ((8, 48), (64, 960)))])
def test_bounds_reject_one_scaled_tile(cid, tile):
    """one output tile of the kernel (its own tile shape, all channels) scaled by 1.01"""
    case = _case(cid)
    _reject(case, lambda cfg, sd: _tile_scale(cfg, case, tile))
