"""Each float32 TFC-TDF kernel alone -- split-half (csrc/tdfnet_f32s.h) and exact -- at small shapes, against a tight oracle.

The float32 parity mode was checked only through whole random networks (2e-4 of the output peak, 1e-4 PCM): 100 to 1000 times the
error its kernels claim (2^-22 per product).  Here, as in test_tdfnet_isolated.py, the network is structured
(oracle/tdfnet_structured.py): every layer except one TARGET passes its input through, so the forward differs from the float32
storage oracle, computed in float64 between the stores, only by what the target (and the roundings behind it) add.  Every case runs
TDFNet.forward_nhwc through the ``dev`` fixture -- the emulated kernel sources (-m "not gpu") and the GPU (-m gpu) -- at the smallest
geometries that reach every instance and every launcher branch of run_conv / run_tdf / run_pix for a float32 network, asserts by the
launchers' alias launch names that the intended instance and grid order ran, and bounds
  - per (window, frame) row: max over rows of |got - want| / |want|;
  - per element: |got - want| <= a * (ulp32(|want|) + ulp32(rms(want))).

Inputs carry 22 significant bits (the low two mantissa bits of randn cleared): hi + lo / 2^11 reproduces such a value exactly, so
the passthrough layers in front of the target stay exact in split mode, and the target still reads non-zero lo planes.  (An input
rounded to half precision has an all-zero lo plane everywhere: the a_lo w_hi products would not be tested at all.)

All-passthrough networks on integer data are exact in any summation order: those forwards must be bit-identical.

CPU only, oracle against oracle: the bounds reject defects a split or exact kernel could plausibly have.
"""
import functools
import time

import pytest
import torch
import torch.nn.functional as F

from audiolab_amd.tdfnet import TDFNet, TDFNetConfig
from oracle import tdfnet_oracle
from oracle.tdfnet_structured import block_name, integer_input, structured_state_dict, target_layer

MANT = 23


def _cfg(g, blocks, dim_f, dim_t, bn):
    return TDFNetConfig(dim_f=dim_f, dim_t=dim_t, n_fft=2 * dim_f, hop=dim_f // 2, num_blocks=blocks, g=g, bn=bn)


# levels (c, T, F):
GEOM = {"P": _cfg(48, 3, 88, 20, 4),      # (48, 20, 88), (96, 10, 44)
        "Q": _cfg(16, 5, 96, 24, 4),      # (16, 24, 96), (32, 12, 48), (48, 6, 24)
        "R": _cfg(16, 3, 40, 12, 4),      # (16, 12, 40), (32, 6, 20)
        "S": _cfg(48, 3, 128, 16, 8),     # (48, 16, 128), (96, 8, 64)
        "U": _cfg(16, 3, 128, 8, 4)}      # (16, 8, 128), (32, 4, 64)
CONTRACTIONS = ("split", "exact")


# ------------------------------------------------------------------------------------------------------------------------
# what the float32 launchers of tdfnet.hip do, restated: per layer launch, the alias names it is counted under
# ------------------------------------------------------------------------------------------------------------------------
def _cdiv(a, b):
    return -(-a // b)


def conv_names(contraction, c, B, T, Fw):
    if contraction == "split":                               # launch_conv_split
        kc, bn = (24, 48) if c % 48 == 0 else (16, 16)
        tw = 32 if Fw >= 32 else 16
        ntiles, nyc = B * _cdiv(T, 256 // tw) * _cdiv(Fw, tw), c // bn
        return [f"conv3x3_f32s_kernel<{kc},{bn},{tw}>"] + (["conv3x3_f32s_kernel<ny_fastest>"] if ntiles % 8 == 0 and nyc > 1 else [])
    bn = 48 if c % 48 == 0 else 16                           # run_conv / run_conv_tw
    tw = 64 if Fw % 64 == 0 else 32 if Fw >= 32 else 16
    return [f"conv3x3_kernel<f32,16,{bn},{tw}>"]


def tdf_names(contraction, residual, M, B, T, c):
    res = "res" if residual else "nores"
    if contraction == "exact":
        return [f"tdf_gemm_kernel<f32,{res}>"]
    gx, nrb = _cdiv(B * T * (c // 16), 8), _cdiv(M, 64)      # run_tdf_split
    return [f"tdf_gemm_f32s_kernel<{res}>"] + (["tdf_gemm_f32s_kernel<nrb_fast>"] if nrb > 1 and gx % 8 == 0 else [])


def pix_names(contraction, mode, M, ncols):
    if contraction == "exact":
        return [f"pix_gemm_kernel<f32,{mode}>"]
    gx, nrb = _cdiv(ncols, 128), _cdiv(M, 64)                # run_pix_split
    return [f"pix_gemm_f32s_kernel<{mode}>"] + (["pix_gemm_f32s_kernel<nrb_fast>"] if nrb > 1 and gx % 8 == 0 else [])


def layer_names(cfg, target, B, contraction):
    """the alias names of the launch(es) that serve ``target`` (tdf: linear A, then linear B)"""
    kind, k = target
    lv = cfg.levels()
    c, T, Fw = lv[k]
    if kind == "conv":
        return [conv_names(contraction, c, B, T, Fw)]
    if kind == "tdf":
        return [tdf_names(contraction, False, Fw // cfg.bn, B, T, c), tdf_names(contraction, True, Fw, B, T, c)]
    c1, T1, F1 = lv[k + 1]
    return [pix_names(contraction, kind, c1 if kind == "ds" else 4 * c, B * T1 * F1)]


def network_counts(cfg, B, contraction):
    """{name: launches} of one forward of B windows: every alias name, and the six pinned names"""
    counts = {}

    def add(names, times=1):
        for nm in names:
            counts[nm] = counts.get(nm, 0) + times
    lv = cfg.levels()
    for k, (c, T, Fw) in enumerate(lv):
        blocks = 1 if k == cfg.n else 2                       # encoder and decoder block; one bottleneck
        add(conv_names(contraction, c, B, T, Fw), blocks * cfg.l)
        add(tdf_names(contraction, False, Fw // cfg.bn, B, T, c), blocks)
        add(tdf_names(contraction, True, Fw, B, T, c), blocks)
        if k < cfg.n:
            c1, T1, F1 = lv[k + 1]
            add(pix_names(contraction, "ds", c1, B * T1 * F1))
            add(pix_names(contraction, "us", 4 * c, B * T1 * F1))
    s = "_f32s" if contraction == "split" else ""
    counts[f"conv3x3{s}_kernel"] = (2 * cfg.n + 1) * cfg.l
    counts[f"tdf_gemm{s}_kernel"] = (2 * cfg.n + 1) * 2
    counts[f"pix_gemm{s}_kernel"] = 2 * cfg.n
    return counts


ALIASES = ([f"conv3x3_f32s_kernel<{i}>" for i in ("24,48,32", "24,48,16", "16,16,32", "16,16,16", "ny_fastest")]
           + [f"conv3x3_kernel<f32,16,{bn},{tw}>" for bn in (48, 16) for tw in (64, 32, 16)]
           + [f"tdf_gemm_f32s_kernel<{i}>" for i in ("res", "nores", "nrb_fast")] + [f"pix_gemm_f32s_kernel<{i}>" for i in ("ds", "us", "nrb_fast")]
           + [f"tdf_gemm_kernel<f32,{i}>" for i in ("res", "nores")] + [f"pix_gemm_kernel<f32,{i}>" for i in ("ds", "us")])
PINNED = ["conv3x3_f32s_kernel", "tdf_gemm_f32s_kernel", "pix_gemm_f32s_kernel", "conv3x3_kernel", "tdf_gemm_kernel", "pix_gemm_kernel"]


# ------------------------------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, geom, target, batch, contraction, branch=None):
        """``branch``: per contraction, what the target's launch must be counted under -- names without their kernel prefix; a leading
        "!" = must NOT be counted (tdf: of linear B, the one with two row blocks where any has)"""
        self.geom, self.target, self.batch, self.contraction = geom, target, batch, contraction
        self.branch = (branch or {}).get(contraction, ())
        t = "pass" if target is None else f"{target[0]}{target[1]}"
        self.id = f"{geom}-{t}-B{batch}-{contraction}"


NYF, NRB = "ny_fastest", "nrb_fast"
# (geometry, kind, level, batch, {contraction: branch of the launcher the target takes})
_CELLS = [
    # P: 8 x 32 tiles partial on both axes at level 0 (20 = 8 + 8 + 4, 88 = 32 + 32 + 24) and level 1 (10 = 8 + 2, 44 = 32 + 12)
    ("P", "conv", 0, 1, {"split": ("24,48,32", "!" + NYF), "exact": ("f32,16,48,32",)}),             # two input chunks, one output group
    ("P", "conv", 0, 2, {"split": ("24,48,32", "!" + NYF), "exact": ("f32,16,48,32",)}),
    ("P", "conv", 1, 1, {"split": ("24,48,32", "!" + NYF), "exact": ("f32,16,48,32",)}),             # c 96: four chunks, two groups; 4 tiles
    ("P", "conv", 1, 2, {"split": ("24,48,32", NYF), "exact": ("f32,16,48,32",)}),                   # 8 tiles
    ("P", "tdf", 0, 1, {"split": ("res", NRB), "exact": ("f32,res",)}),     # A: K 88 (tail of Kp 128), M 22; B: K 22, M 88, two row blocks; 8 column tiles
    ("P", "tdf", 0, 2, {"split": ("res", "!" + NRB), "exact": ("f32,res",)}),                        # 15 column tiles
    ("P", "tdf", 1, 1, {"split": ("res", "!" + NRB), "exact": ("f32,res",)}),                        # A: K 44, M 11; B: K 11 (odd: the pair guard), M 44
    ("P", "tdf", 1, 2, {"split": ("res", "!" + NRB), "exact": ("f32,res",)}),
    ("P", "ds", 0, 1, {"split": ("ds", "!" + NRB), "exact": ("f32,ds",)}),                           # K 192, M 96 (two row blocks), 440 B columns
    ("P", "ds", 0, 2, {"split": ("ds", "!" + NRB), "exact": ("f32,ds",)}),
    ("P", "us", 0, 1, {"split": ("us", "!" + NRB), "exact": ("f32,us",)}),                           # K 96 (tail masked), M 192, three row blocks
    ("P", "us", 0, 2, {"split": ("us", "!" + NRB), "exact": ("f32,us",)}),
    ("S", "ds", 0, 2, {"split": ("ds", NRB), "exact": ("f32,ds",)}),                                 # 1024 columns: 8 column tiles
    ("S", "us", 0, 2, {"split": ("us", NRB), "exact": ("f32,us",)}),
    ("S", "conv", 0, 1, {"split": ("24,48,32",), "exact": ("f32,16,48,64",)}),
    ("S", "conv", 1, 1, {"split": ("24,48,32", "!" + NYF), "exact": ("f32,16,48,64",)}),
    ("Q", "conv", 0, 1, {"split": ("16,16,32", "!" + NYF), "exact": ("f32,16,16,32",)}),
    ("Q", "conv", 1, 2, {"split": ("16,16,32", NYF), "exact": ("f32,16,16,32",)}),                   # two output groups, 8 tiles
    ("Q", "conv", 2, 1, {"split": ("24,48,16", "!" + NYF), "exact": ("f32,16,48,16",)}),             # one partial 16-frame tile, 24 = 16 + 8 bins
    ("Q", "tdf", 2, 1, {"split": ("res", "!" + NRB), "exact": ("f32,res",)}),                        # A: K 24, M 6; B: K 6, M 24
    ("Q", "ds", 1, 1, {"split": ("ds", "!" + NRB), "exact": ("f32,ds",)}),                           # K 128, M 48, 144 columns
    ("Q", "us", 1, 1, {"split": ("us", "!" + NRB), "exact": ("f32,us",)}),                           # K 48, M 128
    ("R", "conv", 0, 1, {"split": ("16,16,32", "!" + NYF), "exact": ("f32,16,16,32",)}),             # 40 = 32 + 8 bins
    ("R", "conv", 1, 1, {"split": ("16,16,16", "!" + NYF), "exact": ("f32,16,16,16",)}),
    ("U", "conv", 0, 1, {"split": ("16,16,32", "!" + NYF), "exact": ("f32,16,16,64",)}),
]
CASES = [Case(g, (kind, k), b, con, br) for g, kind, k, b, br in _CELLS for con in CONTRACTIONS]
PASS_CASES = [Case(g, None, b, con) for g in GEOM for b in (1, 2) for con in CONTRACTIONS]
_PREFIX = {"conv": ("conv3x3_f32s_kernel", "conv3x3_kernel"), "tdf": ("tdf_gemm_f32s_kernel", "tdf_gemm_kernel"),
           "ds": ("pix_gemm_f32s_kernel", "pix_gemm_kernel"), "us": ("pix_gemm_f32s_kernel", "pix_gemm_kernel")}

FLOOR = (2e-7, 4.0)
# (row bound, element bound a): 2x what the kernels measured on an MI355X against the float64-between-stores oracle (the table that
# -m gpu -s prints; profiles/tdfnet_f32_isolated.txt), rounded up to two digits; floors 2e-7 on the row metric and 4 on the element
# metric.  The emulated kernels run under the same table (their MFMA sums in another order: up to 1.3e-7 and 4.0 where the GPU has
# 8.5e-8 and 2.67, Q-conv1-B2-split).
BOUNDS = {
    "P-conv0-B1-split": (2.4e-07, 5.4),
    "P-conv0-B1-exact": (2.5e-07, 6),
    "P-conv0-B2-split": (2.4e-07, 6),
    "P-conv0-B2-exact": (2.5e-07, 6),
    "P-conv1-B1-split": (2e-07, 4),
    "P-conv1-B1-exact": (2.3e-07, 5),
    "P-conv1-B2-split": (2e-07, 4),
    "P-conv1-B2-exact": (2.3e-07, 5),
    "P-tdf0-B1-split": (2.5e-07, 6.7),
    "P-tdf0-B1-exact": (2.4e-07, 6.7),
    "P-tdf0-B2-split": (2.5e-07, 6.7),
    "P-tdf0-B2-exact": (2.5e-07, 6.7),
    "P-tdf1-B1-split": (2.2e-07, 5.4),
    "P-tdf1-B1-exact": (2e-07, 6.7),
    "P-tdf1-B2-split": (2.2e-07, 5.4),
    "P-tdf1-B2-exact": (2.1e-07, 6.7),
    "P-ds0-B1-split": (2e-07, 4),
    "P-ds0-B1-exact": (2e-07, 4),
    "P-ds0-B2-split": (2e-07, 5.4),
    "P-ds0-B2-exact": (2e-07, 4),
    "P-us0-B1-split": (2e-07, 5.4),
    "P-us0-B1-exact": (2e-07, 5.4),
    "P-us0-B2-split": (2e-07, 5.4),
    "P-us0-B2-exact": (2e-07, 5.4),
    "S-ds0-B2-split": (2e-07, 5.4),
    "S-ds0-B2-exact": (2e-07, 5.4),
    "S-us0-B2-split": (2e-07, 5.4),
    "S-us0-B2-exact": (2e-07, 4.8),
    "S-conv0-B1-split": (2.3e-07, 6),
    "S-conv0-B1-exact": (2.4e-07, 5.4),
    "S-conv1-B1-split": (2e-07, 4),
    "S-conv1-B1-exact": (2e-07, 5.4),
    "Q-conv0-B1-split": (2e-07, 4),
    "Q-conv0-B1-exact": (2.1e-07, 5),
    "Q-conv1-B2-split": (2e-07, 5.4),
    "Q-conv1-B2-exact": (2.8e-07, 9.4),
    "Q-conv2-B1-split": (2.2e-07, 6.7),
    "Q-conv2-B1-exact": (2.1e-07, 7),
    "Q-tdf2-B1-split": (2.7e-07, 6.4),
    "Q-tdf2-B1-exact": (2e-07, 4.8),
    "Q-ds1-B1-split": (2e-07, 4.8),
    "Q-ds1-B1-exact": (2e-07, 4),
    "Q-us1-B1-split": (2e-07, 4),
    "Q-us1-B1-exact": (2e-07, 4),
    "R-conv0-B1-split": (2e-07, 4),
    "R-conv0-B1-exact": (2.1e-07, 5),
    "R-conv1-B1-split": (2e-07, 4),
    "R-conv1-B1-exact": (2e-07, 4),
    "U-conv0-B1-split": (2e-07, 5),
    "U-conv0-B1-exact": (2e-07, 4),
}
assert set(BOUNDS) == {c.id for c in CASES} and all(rb >= FLOOR[0] and eb >= FLOOR[1] for rb, eb in BOUNDS.values())


def target_names(case):
    """the alias names of the target's launch(es), by the launchers' arithmetic -- which must say what the branch table says"""
    names = layer_names(GEOM[case.geom], case.target, case.batch, case.contraction)
    prefix = _PREFIX[case.target[0]][case.contraction == "exact"]
    assert case.branch, case.id
    for want in case.branch:
        nm = f"{prefix}<{want.lstrip('!')}>"
        assert (nm in names[-1]) == (not want.startswith("!")), (case.id, want, names)
    return {nm for launch in names for nm in launch}


def test_every_float32_instance_and_branch_is_some_cases_target():
    """every alias name the float32 launchers can note is what some case's TARGET launch is counted under"""
    hit = set().union(*(target_names(case) for case in CASES))
    assert hit == set(ALIASES), sorted(set(ALIASES) ^ hit)


# ------------------------------------------------------------------------------------------------------------------------
# metrics, inputs, oracle
# ------------------------------------------------------------------------------------------------------------------------
def ulp(v: torch.Tensor) -> torch.Tensor:
    _, e = torch.frexp(v.abs().double())
    return torch.ldexp(torch.ones_like(v, dtype=torch.float64), (e - 1 - MANT).clamp(min=-149))


def metrics(got: torch.Tensor, want: torch.Tensor):
    """-> (max per-(window, frame) row rel-L2, max element error in units of ulp32(|want|) + ulp32(rms(want))), layout [B,4,F,T]"""
    d = (got.double() - want.double())
    w = want.double()
    rows = d.pow(2).sum(dim=(1, 2)).sqrt() / w.pow(2).sum(dim=(1, 2)).sqrt().clamp(min=1e-300)
    rms = w.pow(2).mean().sqrt()
    elem = d.abs() / (ulp(w) + ulp(rms.reshape(1)))
    return float(rows.max()), float(elem.max())


def case_input(cfg, batch, seed=11):
    """randn with 22 significant bits: exactly hi + lo / 2^11 (see the module docstring)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((batch, 4, cfg.dim_f, cfg.dim_t), generator=g)
    return (x.view(torch.int32) & ~3).view(torch.float32)


def input_layer(cfg, target):
    """the oracle's name of the layer whose stored output the target reads"""
    kind, k = target
    if kind == "conv":
        return "first_conv" if k == 0 else f"ds.{k - 1}"
    if kind == "tdf":
        return f"{block_name(cfg, k)}.tfc.{cfg.l - 1}"
    if kind == "ds":
        return f"{block_name(cfg, k)}.tdf.1"
    return "bottleneck_block.tdf.1" if k == cfg.n - 1 else f"decoding_blocks.{cfg.n - 2 - k}.tdf.1"


def oracle(sd, cfg, x, target=None, perturb=None):
    """float32-storage oracle on x [B,4,F,T] (float64: float64 between the stores); with a target: also the fraction of the non-zero
    values it reads that differ from their half rounding (their lo plane is not zero), and the exact zeros of its output"""
    src = None if target is None else input_layer(cfg, target)
    dst = None if target is None else target_layer(cfg, target)
    seen = {}

    def hook(n, y):
        if perturb is not None:
            y = perturb(n, y)
        if n == src:
            v = y.float()
            nz = v != 0
            seen["lo"] = float(((v.half().float() != v) & nz).sum()) / max(1, int(nz.sum()))
        if n == dst:
            seen["zeros"] = float((y == 0).double().mean())
        return y
    with torch.no_grad():
        out = tdfnet_oracle.forward(sd, x, cfg.num_blocks, cfg.l, cfg.bn, storage=torch.float32, perturb=hook)
    return out.cpu(), seen


@functools.lru_cache(maxsize=None)
def case_data(geom, target, batch, device):
    """(state dict, input, oracle output, what the oracle saw): computed once per (geometry, target, batch), shared by both
    contractions (and by the rejection tests, device "cpu"); read only"""
    cfg = GEOM[geom]
    if target is None:
        sd = structured_state_dict(cfg, None, final="dyadic", shift=True)
        x = integer_input(cfg, batch)
    else:
        sd = structured_state_dict(cfg, target, seed=3, final="random")
        x = case_input(cfg, batch)
    want, seen = oracle(sd, cfg, x.double().to(device), target)
    return sd, x, want, seen


def run_net(dev, cfg, sd, x, contraction):
    """-> (output [B,4,F,T] on the CPU, range word raised)"""
    net = TDFNet(cfg, sd, ctx=dev, dtype=torch.float32, max_batch=x.shape[0], contraction=contraction)
    dev.launch_counts_reset()
    got = net.forward_nhwc(x.permute(0, 3, 2, 1).contiguous().to(dev.device))
    dev.synchronize()
    raised = net.range_exceeded() or net._exact is not None      # forward_nhwc reads the word itself, and builds the exact twin if it was set
    del net
    return got.float().cpu().permute(0, 3, 2, 1), raised


def assert_counts(dev, cfg, batch, contraction):
    want = network_counts(cfg, batch, contraction)
    got = {nm: dev.launch_count(nm) for nm in ALIASES + PINNED}
    assert got == {nm: want.get(nm, 0) for nm in ALIASES + PINNED}, {nm: (got[nm], want.get(nm, 0)) for nm in got if got[nm] != want.get(nm, 0)}


_TABLE = []


@pytest.fixture(scope="module", autouse=True)
def _print_table():
    yield
    if _TABLE:
        print("\nisolated float32 kernels: backend | id | row rel-L2 (bound) | element units (bound) | lo planes | target zeros | s")
        for r in _TABLE:
            print("  " + " | ".join(str(v) for v in r))


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_isolated_f32_kernel_vs_storage_oracle(dev, case):
    t0 = time.time()
    cfg = GEOM[case.geom]
    sd, x, want, seen = case_data(case.geom, case.target, case.batch, str(dev.device))
    got, raised = run_net(dev, cfg, sd, x, case.contraction)
    for nm in target_names(case):                              # the branch table's instance and grid order: they ran,
        assert dev.launch_count(nm) > 0, (case.id, nm)
    assert_counts(dev, cfg, case.batch, case.contraction)     # as often as the launchers' arithmetic says, and nothing else did
    row, elem = metrics(got, want)
    rb, eb = BOUNDS[case.id]
    _TABLE.append(("emul" if dev.device.type == "cpu" else "gpu", case.id, f"{row:.2e} ({rb:.1e})", f"{elem:.2f} ({eb:.1f})",
                   f"{seen['lo']:.4f}", f"{seen['zeros']:.4f}", f"{time.time() - t0:.1f}"))
    assert seen["lo"] > 0.9, seen                              # the target reads non-zero lo planes
    assert not raised                                          # nothing left the half range: the split kernels' result is what was compared
    assert row < rb and elem < eb, (case.id, row, rb, elem, eb)


@pytest.mark.parametrize("case", PASS_CASES, ids=[c.id for c in PASS_CASES])
def test_all_passthrough_f32_bit_identical(dev, case):
    """every kernel's data movement in one forward: halos and zero padding (the passthrough 3x3 convs shift by one frame / bin),
    partial tiles, both grid orders, K tails, ds / us channel maps"""
    cfg = GEOM[case.geom]
    sd, x, want, _ = case_data(case.geom, None, case.batch, str(dev.device))
    got, raised = run_net(dev, cfg, sd, x, case.contraction)
    assert_counts(dev, cfg, case.batch, case.contraction)
    want = want.float()
    assert not raised
    assert want.abs().max() > 1 and float((want != 0).double().mean()) > 0.3
    assert torch.equal(got, want), (float((got != want).double().mean()), float((got - want).abs().max()))


# ------------------------------------------------------------------------------------------------------------------------
# CPU: the bounds reject defects a kernel could plausibly have (oracle against oracle, same geometry, same case)
# ------------------------------------------------------------------------------------------------------------------------
def _case(cid):
    return next(c for c in CASES if c.id == cid)


def split_half(v):
    """float32 values (held in float64) -> (hi, lo / 2^11) as the split kernels carry them: hi = half(v), lo = half((v - hi) 2^11)"""
    v32 = v.float()
    hi = v32.half().float()
    lo = ((v32 - hi) * 2048.0).half().float() / 2048.0
    return hi.double(), lo.double()


def _unit_mask(y, units):
    """y [B,C,T,*]: mask [B,C,T,1] of the TDF kernels' units (16 channels of one (b, t)), u = (b T + t) C / 16 + c / 16"""
    B, C, T = y.shape[:3]
    u = (torch.arange(B * T).reshape(B, 1, T) * (C // 16) + (torch.arange(C) // 16).reshape(1, C, 1))
    return ((u >= units[0]) & (u < units[1])).unsqueeze(-1)


def _defect_hook(cfg, sd, case, defect):
    """perturb hook: the target's pre-store output with one defect in the outputs of one workgroup"""
    kind, k = case.target
    src, dst = input_layer(cfg, case.target), target_layer(cfg, case.target)
    p = block_name(cfg, k)
    seen = {}

    def hook(n, y):
        if n == src:
            seen["x"] = (y.transpose(-1, -2) if n == "first_conv" else y).float().double()       # what the store leaves
        if defect == "tdf_hi_lo" and n == f"{p}.tdf.0":
            # split TDF, linear A: the a_hi w_lo products of K tile 0 (64 bins) missing in column tile 1 (units 8..15), its one row block
            x, w, b = seen["x"], sd[f"{p}.tdf.0.weight"].double(), sd[f"{p}.tdf.0.bias"].double()
            xh, _ = split_half(x)
            _, wl = split_half(w)
            bad = torch.relu(F.linear(x, w, b) - F.linear(xh[..., :64], wl[:, :64]))
            return torch.where(_unit_mask(y, (8, 16)), bad, y)
        if n != dst:
            return y
        y = y.clone()
        x = seen["x"]
        if kind == "conv":
            q = f"{p}.tfc.H.0.0"
            w, b = sd[q + ".weight"].double(), sd[q + ".bias"].double()
            t8 = (slice(None), slice(0, 48), slice(8, 16), slice(32, 64)) if k == 0 else (slice(None), slice(0, 48), slice(0, 8), slice(0, 32))
            if defect in ("conv_lo_hi", "conv_lo_lo"):
                xh, xl = split_half(x)
                wh, wl = split_half(w)
                if defect == "conv_lo_hi":                    # one k-group: input channels 8..15 of tap (1, 2)
                    xm, wm = torch.zeros_like(xl), torch.zeros_like(wh)
                    xm[:, 8:16] = xl[:, 8:16]
                    wm[:, 8:16, 1, 2] = wh[:, 8:16, 1, 2]
                    d = F.conv2d(xm, wm, padding=1)
                else:                                         # every a_lo w_lo product of the tile: the term the design drops
                    d = F.conv2d(xl, wl, padding=1)
                y[t8] = torch.relu(F.conv2d(x, w, b, padding=1) - d)[t8]
            elif defect == "conv_scale":
                y[t8] *= 1.0 + 2.0 ** -18
            elif defect == "conv_swap":                       # ny_fastest: the tiles of window 0 and window 1 exchanged
                a, b2 = (0,) + t8[1:], (1,) + t8[1:]
                y[a], y[b2] = y[b2].clone(), y[a].clone()
        elif kind == "ds" and defect == "pix_lo_scale":
            # split ds: the lo accumulator of column tile 1 (columns 128..255), row block 0, scaled by 2^-10 instead of 2^-11
            w, b = sd[f"ds.{k}.0.weight"].double(), sd[f"ds.{k}.0.bias"].double()
            xh, xl = split_half(x)
            wh, wl = split_half(w)
            lo = F.conv2d(xh, wl, stride=2) + F.conv2d(xl, wh, stride=2)
            bad = torch.relu(F.conv2d(x, w, b, stride=2) + lo)
            B, _, Tp, Fp = y.shape
            col = torch.arange(B * Tp * Fp).reshape(B, 1, Tp, Fp)
            m = ((col >= 128) & (col < 256)) & (torch.arange(y.shape[1]).reshape(1, -1, 1, 1) < 64)
            y = torch.where(m, bad, y)
        elif kind == "tdf" and defect == "tdf_swap":          # nrb_fast, linear B: column tiles 0 and 1 of row block 0 exchanged
            B, C, T, Fw = y.shape
            u = y.permute(0, 2, 1, 3).reshape(B * T * (C // 16), 16, Fw).clone()
            u[0:8, :, :64], u[8:16, :, :64] = u[8:16, :, :64].clone(), u[0:8, :, :64].clone()
            y = u.reshape(B, T, C, Fw).permute(0, 2, 1, 3)
        return y
    return hook


def _defect_error(cid, defect):
    case = _case(cid)
    cfg = GEOM[case.geom]
    sd, x, clean, _ = case_data(case.geom, case.target, case.batch, "cpu")
    bad, _ = oracle(sd, cfg, x.double(), perturb=_defect_hook(cfg, sd, case, defect))
    row, elem = metrics(bad, clean)
    rb, eb = BOUNDS[cid]
    print(f"{cid} {defect}: row {row:.2e} (bound {rb:.1e}), element {elem:.2f} (bound {eb:.1f})")
    return row, elem, rb, eb


@pytest.mark.parametrize("cid,defect", [("P-conv0-B1-split", "conv_lo_hi"), ("P-tdf0-B1-split", "tdf_hi_lo"), ("P-ds0-B1-split", "pix_lo_scale"),
                                        ("P-conv1-B1-exact", "conv_scale"), ("P-conv1-B2-split", "conv_swap"), ("P-tdf0-B1-split", "tdf_swap")])
def test_bounds_reject_defect(cid, defect):
    """conv_lo_hi: the a_lo w_hi products of one k-group (8 input channels, one tap) missing in one 8 x 32 tile; tdf_hi_lo: the
    a_hi w_lo products of one 64-wide K tile missing in one workgroup; pix_lo_scale: one workgroup's lo accumulator worth 2^-10;
    conv_scale: one tile scaled by 1 + 2^-18; conv_swap / tdf_swap: two tiles' outputs exchanged (a wrong 1-D grid decode)"""
    row, elem, rb, eb = _defect_error(cid, defect)
    assert row > rb or elem > eb, (row, rb, elem, eb)


def test_bounds_accept_the_dropped_lo_lo_term():
    """the a_lo w_lo products of a whole tile -- what the design drops, 2^-22 of a product -- stay inside the bound"""
    row, elem, rb, eb = _defect_error("P-conv0-B1-split", "conv_lo_lo")
    assert row < rb and elem < eb, (row, rb, elem, eb)
