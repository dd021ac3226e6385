"""Convolution reverb (audiolab_amd/reverb.py ``apply_reverb`` -> csrc/reverb.hip ``alsep_reverb_apply``) on the emulated kernels
(-m "not gpu") and on the GPU (-m gpu), same bodies: against tests/golden/reverb_apply.npz -- the reference's own ``apply_reverb``
(handlers/reverb.py:179-209) run by scripts/make_golden_reverb_apply.py on the cases of tests/reverb_apply_cases.py -- and against the
exact convolution (long-double dot products) stored beside it.

Tolerances.  Results are clipped to +-1, where one float32 ulp is 2^-24 and the rounding to float32 costs at most 2^-25.
  * against the exact value: 2^-24.  A float64 overlap-save rounded to float32 sits at the rounding alone (2.98e-8); a single-precision
    transform (~6e-8 and up) does not pass, on purpose.
  * against the reference: 2^-24 + 2 ref_err, ref_err = max|reference - exact| read from the fixture (3e-8 .. 1.5e-7: scipy's
    fftconvolve transforms the float32 dry signal in single precision).
  * the exact values travel as int16 distances from the reference in steps of 2^-36 (see the generator): 7e-12 of storage rounding."""
import json
import logging
import os
import struct

import numpy as np
import pytest
import torch

from tests.conftest import host, on
from tests.reverb_apply_cases import CASES, SAMPLED, WET_GAIN, chan_major, exact_final, make_case, positions

ULP = 2.0 ** -24
_RESULTS = {}                                                                # (device type, case, log2_block, blocks_per_batch) -> [C, N]
_GOLDEN = {}


def golden(golden_dir):
    if not _GOLDEN:
        with np.load(os.path.join(golden_dir, "reverb_apply.npz")) as z:
            _GOLDEN.update({k: z[k] for k in z.files})
    return _GOLDEN


def smallest_log2(taps: int) -> int:
    """the smallest legal block exponent: 2^k >= 2 L"""
    return max(1, (2 * taps - 1).bit_length())


def run_case(dev, name, log2_block=0, blocks_per_batch=0) -> np.ndarray:
    """ours on a case -> float32 [C, N] on the host (kept: several tests look at the same run)"""
    from audiolab_amd import reverb
    key = (dev.device.type, name, log2_block, blocks_per_batch)
    if key not in _RESULTS:
        dry, ir, pre_delay, sr = make_case(name)
        out = reverb.apply_reverb_array(on(dev, chan_major(dry)), ir, int(pre_delay * sr), log2_block=log2_block,
                                        blocks_per_batch=blocks_per_batch, ctx=dev)
        assert out.dtype == torch.float32 and out.device.type == dev.device.type and tuple(out.shape) == chan_major(dry).shape
        _RESULTS[key] = host(out)
    return _RESULTS[key]


def fixture_of(golden_dir, name):
    """-> (reference, exact) as float64 [C, positions], ref_err"""
    g = golden(golden_dir)
    ref = g[f"{name}_ref"]
    exact = ref + g[f"{name}_exact_q"].astype(np.float64) * 2.0 ** -36
    return chan_major(ref), chan_major(exact), float(g[f"{name}_ref_err"][0])


@pytest.mark.parametrize("name", list(CASES))
def test_against_the_reference(dev, golden_dir, name):
    """padding, crop, the 0.7 gain, the clip and the channel handling of handlers/reverb.py:186-206"""
    ref, _, ref_err = fixture_of(golden_dir, name)
    assert int(golden(golden_dir)[f"{name}_pre"][0]) == int(CASES[name][4] * CASES[name][0])
    got = run_case(dev, name)[:, positions(name)].astype(np.float64)
    err = float(np.max(np.abs(got - ref)))
    print(f"{name} [{dev.device.type}]: max|ours - reference| = {err:.3e} (ref_err {ref_err:.3e}, bound {ULP + 2 * ref_err:.3e})")
    assert err <= ULP + 2 * ref_err


# block length picked from L, forced to the smallest legal one, and twice that: the only geometries here whose transforms end in a
# radix-4 pass (2^11, and 2^2 for the one-tap response); not for the 88 200-tap case, where a 2^19-point block adds time, not coverage
MODES = [(name, mode) for name in CASES for mode in ("auto", "smallest", "plus1") if not (mode == "plus1" and name in SAMPLED)]


@pytest.mark.parametrize("name,mode", MODES)
def test_against_the_exact_convolution(dev, golden_dir, name, mode):
    _, exact, _ = fixture_of(golden_dir, name)
    k = {"auto": 0, "smallest": smallest_log2(CASES[name][3]), "plus1": smallest_log2(CASES[name][3]) + 1}[mode]
    got = run_case(dev, name, log2_block=k)[:, positions(name)].astype(np.float64)
    err = float(np.max(np.abs(got - exact)))
    print(f"{name} [{dev.device.type}, log2_block={k}]: max|ours - exact| = {err:.3e} (bound {ULP:.3e})")
    assert err <= ULP


@pytest.mark.parametrize("name", list(CASES))
def test_batch_size_does_not_change_a_bit(dev, name):
    """one block per batch (the minimum workspace) against as many as fit, at the smallest legal block length"""
    k = smallest_log2(CASES[name][3])
    one = run_case(dev, name, log2_block=k, blocks_per_batch=1)
    many = run_case(dev, name, log2_block=k)
    assert np.array_equal(one.view(np.uint32), many.view(np.uint32))
    if name == "tiny_stereo":
        assert np.array_equal(one.view(np.uint32), run_case(dev, name, log2_block=k, blocks_per_batch=4).view(np.uint32))


def test_delay_past_the_end_is_the_clipped_dry_signal(dev):
    dry, _, pre_delay, sr = make_case("delay_past_end")
    assert int(pre_delay * sr) >= len(dry)
    got = run_case(dev, "delay_past_end")
    assert np.array_equal(got, np.clip(chan_major(dry), -1.0, 1.0))


def test_unit_impulse_response(dev):
    """L = 1: the result is float32(clip(dry + 0.7 ir[0] dry)).  Bit for bit with blocks of two points (the smallest legal: the
    transforms are one exact butterfly each way).  With the block length picked from L (1024 points) the same holds at every sample
    where that float64 value decides its own rounding: 1.7 x lies within 1e-16 of a float32 rounding midpoint for about 6 % of all
    float32 x (17 m / 10 ends in .5 for every mantissa m = 5 mod 10; only the 4e-17 by which the double 0.7 misses 7/10 breaks the
    tie), which is below the rounding of any 1024-point transform pair (<= 2 log2(F) 2^-53 = 2^-48.7 for |x| <= 1).  There -- 97 of the
    6000 samples on the emulated kernels -- either float32 neighbour of the midpoint is accepted, nothing else."""
    dry, ir, _, _ = make_case("unit_ir")
    d = chan_major(dry).astype(np.float64)
    v = np.clip(d + WET_GAIN * ir[0] * d, -1.0, 1.0)
    want = v.astype(np.float32)
    assert np.array_equal(run_case(dev, "unit_ir", log2_block=1), want)
    got = run_case(dev, "unit_ir")
    other = np.nextafter(want, np.where(v > want, np.float32(2), np.float32(-2)).astype(np.float32))
    near_tie = np.abs(v - 0.5 * (want.astype(np.float64) + other.astype(np.float64))) <= 2.0 ** -48
    assert 0 < np.mean(near_tie) < 0.1
    assert np.array_equal(got[~near_tie], want[~near_tie])
    assert np.all((got[near_tie] == want[near_tie]) | (got[near_tie] == other[near_tie]))
    print(f"unit_ir [{dev.device.type}]: {int(np.sum(got != want))} of {got.size} samples took the other side of a rounding tie "
          f"({int(np.sum(near_tie))} samples within 2^-48 of one)")


def test_mono_1d_and_host_inputs(dev):
    """a 1-D signal takes the same path (:200-203); host arrays are accepted"""
    from audiolab_amd import reverb
    dry, ir, pre_delay, sr = make_case("mono_delay")
    assert dry.ndim == 1
    out = reverb.apply_reverb_array(dry, ir, int(pre_delay * sr), ctx=dev)
    assert tuple(out.shape) == (1, len(dry)) and np.array_equal(host(out), run_case(dev, "mono_delay"))


def _pcm16_header(path):
    with open(path, "rb") as f:
        data = f.read(44)
    tag, ch, sr, _, _, bits = struct.unpack("<HHIIHH", data[20:36])
    return tag, ch, sr, bits


def test_files_in_files_out(dev, tmp_path):
    """the reference's calling convention: apply_reverb(dry wav, params json, output wav) -> output path, 16-bit PCM (:208)"""
    from audiolab_amd import reverb, wavio
    dry, ir, pre_delay, sr = make_case("tiny_stereo")
    dry_path, param_path, out_path = str(tmp_path / "dry.wav"), str(tmp_path / "impulse_response.ir"), str(tmp_path / "out.wav")
    wavio.write_wav(dry_path, chan_major(dry), sr)
    params = {"sample_rate": sr, "pre_delay": 0.0126, "impulse_response": ir.tolist()}      # int(0.0126 * 8000) = int(100.8) = 100
    with open(param_path, "w") as f:
        json.dump(params, f, indent=2)
    assert reverb.load_params_from_file(param_path) == params
    assert reverb.apply_reverb(dry_path, param_path, out_path, ctx=dev) == out_path
    assert _pcm16_header(out_path) == (1, 2, sr, 16)
    audio, file_sr = wavio.read_wav(out_path)
    assert audio.shape == chan_major(dry).shape and file_sr == sr
    want = host(reverb.apply_reverb_array(on(dev, chan_major(dry)), ir, 100, ctx=dev))
    assert np.array_equal(want[:, :100], chan_major(dry)[:, :100])            # nothing arrives before the pre-delay (|dry| < 1 here)
    assert np.max(np.abs(audio - want)) <= 1.0 / 32768 + 1e-7                 # PCM_16: round to nearest, +1.0 clips to 32767
    # an in-memory signal with sr=, a loaded dict, float32 output
    f32_path = str(tmp_path / "out_f32.wav")
    assert reverb.apply_reverb(chan_major(dry), params, f32_path, sr=sr, ctx=dev, subtype="FLOAT") == f32_path
    assert np.array_equal(wavio.read_wav(f32_path)[0], want)


def test_ir_file_of_extract_reverb_goes_straight_in(dev, tmp_path):
    """stems/impulse_response.ir as extract_reverb writes it (wrappers/merge.py:118 hands exactly that file over)"""
    from scipy.signal import fftconvolve
    from audiolab_amd import reverb
    from oracle.reverb_cases import make_case as make_pair
    dry, wet, sr = make_pair("odd_stereo")
    ir_path, out_path = str(tmp_path / "impulse_response.ir"), str(tmp_path / "merged.wav")
    reverb.extract_reverb(on(dev, chan_major(dry)), on(dev, chan_major(wet)), ir_path, sr=sr, ctx=dev)
    assert reverb.apply_reverb(on(dev, chan_major(dry)), ir_path, out_path, sr=sr, ctx=dev, subtype="FLOAT") == out_path
    from audiolab_amd import wavio
    got = wavio.read_wav(out_path)[0].astype(np.float64)
    p = reverb.load_params_from_file(ir_path)
    h, pre = np.array(p["impulse_response"]), int(p["pre_delay"] * sr)
    d = chan_major(dry).astype(np.float64)
    wet64 = np.stack([np.pad(fftconvolve(d[c], h, mode="full"), (pre, 0))[: d.shape[1]] for c in range(d.shape[0])])
    assert np.max(np.abs(got - np.clip(d + WET_GAIN * wet64, -1.0, 1.0))) <= ULP


def test_process_song_writes_both_files(dev, tmp_path):
    """handlers/reverb.py:216-226"""
    from audiolab_amd import reverb, wavio
    from oracle.reverb_cases import make_case as make_pair
    dry, wet, sr = make_pair("odd_stereo")
    wavio.write_wav(str(tmp_path / "dry.wav"), chan_major(dry), sr)
    wavio.write_wav(str(tmp_path / "wet.wav"), chan_major(wet), sr)
    out = reverb.process_song(str(tmp_path / "dry.wav"), str(tmp_path / "wet.wav"), str(tmp_path), ctx=dev)
    assert out == os.path.join(str(tmp_path), "reverb_applied.wav") and os.path.exists(out)
    assert os.path.exists(os.path.join(str(tmp_path), "reverb_params.json"))
    assert _pcm16_header(out) == (1, 2, sr, 16) and wavio.read_wav(out)[0].shape == chan_major(dry).shape


def test_errors_and_the_sample_rate_warning(dev, tmp_path, caplog):
    import ctypes as C
    from audiolab_amd import _lib, reverb
    from audiolab_amd._lib import AlsepError
    dry, ir, _, sr = make_case("tiny_stereo")
    d = on(dev, chan_major(dry))
    with pytest.raises(ValueError):                                          # np.pad's ValueError on a negative pad width (:197)
        reverb.apply_reverb(d, {"pre_delay": -0.01, "impulse_response": ir.tolist()}, str(tmp_path / "x.wav"), sr=sr, ctx=dev)
    with pytest.raises(ValueError):
        reverb.apply_reverb_array(d, ir, -1, ctx=dev)
    with pytest.raises(AlsepError):                                          # above the 2^20-tap cap
        reverb.apply_reverb_array(d, np.zeros((1 << 20) + 1), 0, ctx=dev)
    reverb.apply_reverb_array(d[:, :64], np.ones(96000) / 96000, 0, ctx=dev)  # the 2 s cap extract_reverb writes at 48 kHz works
    with pytest.raises(AlsepError):                                          # a block shorter than 2 L
        reverb.apply_reverb_array(d, ir, 0, log2_block=9, ctx=dev)
    # the C entry point itself: geometry, workspace, aliasing
    lib = dev.lib
    assert lib.alsep_reverb_apply_workspace_bytes((1 << 20) + 1, 0, 1) == -1 and lib.alsep_reverb_apply_workspace_bytes(300, 9, 1) == -1
    assert lib.alsep_reverb_apply_workspace_bytes(300, 0, 0) == -1
    assert lib.alsep_reverb_apply_workspace_bytes(300, 0, 3) == 7 * 1024 * 16 and lib.alsep_reverb_apply_block_log2(88200, 0) == 18
    ir_t, out = on(dev, ir), torch.empty_like(d)
    need = int(lib.alsep_reverb_apply_workspace_bytes(len(ir), 0, 1))
    ws = torch.empty((need,), dtype=torch.uint8, device=dev.device)
    c, n = d.shape

    def call(dst, ws_bytes, pre=0):
        return lib.alsep_reverb_apply(dev.handle, _lib.ptr(d), c, n, n, _lib.ptr(ir_t), len(ir), pre, WET_GAIN, 0, _lib.ptr(dst), n, _lib.ptr(ws),
                                      ws_bytes)
    assert call(out, need) == 0
    assert call(out, need - 1) == -1 and call(d, need) == -1 and call(out, need, pre=-1) == -1
    _ = C
    # a parameter file extracted at another rate: the reference applies it sample by sample without a word; here a WARNING says so
    with caplog.at_level(logging.WARNING, logger="audiolab_amd.reverb"):
        reverb.apply_reverb(d, {"sample_rate": sr * 2, "pre_delay": 0.0, "impulse_response": ir.tolist()}, str(tmp_path / "y.wav"), sr=sr, ctx=dev)
    assert any(r.levelno == logging.WARNING and "apply_reverb" in r.getMessage() for r in caplog.records)
    caplog.clear()
    with caplog.at_level(logging.WARNING, logger="audiolab_amd.reverb"):
        reverb.apply_reverb(d, {"sample_rate": sr, "pre_delay": 0.0, "impulse_response": ir.tolist()}, str(tmp_path / "z.wav"), sr=sr, ctx=dev)
    assert not caplog.records


@pytest.mark.gpu
def test_long_track_in_several_batches(gpu_ctx):
    """60 s of stereo at 44.1 kHz against the 2 s impulse response extract_reverb stores (88 200 taps), pre-delay 0.02 s, the workspace
    capped at 4 blocks of 2^18 points: 16 blocks in 4 batches.  64 seeded positions per channel -- some in the first and in the last
    block -- against long-double dot products on the host."""
    from audiolab_amd import reverb
    sr, n, taps = 44100, 60 * 44100, 88200
    pre = int(0.02 * sr)
    rng = np.random.default_rng(21)
    dry = (0.2 * rng.standard_normal((n, 2)) * np.exp(-((np.arange(n)[:, None] / sr * 2.0) % 1.0) * 3.0)).astype(np.float32)
    ir = rng.standard_normal(taps) * np.exp(-np.arange(taps) / (taps / 6.9))
    ir[0] = 1.0
    ir /= np.sqrt(np.sum(ir ** 2))
    step = (1 << 18) - taps + 1
    n_blocks = -(-(n - pre) // step)
    assert n_blocks == 16
    pos = np.sort(np.concatenate([rng.integers(pre, pre + step, 8), rng.integers(pre + (n_blocks - 1) * step, n, 8), [0, pre - 1, pre, n - 1],
                                  rng.integers(0, n, 44)]))
    out = reverb.apply_reverb_array(torch.from_numpy(chan_major(dry)).cuda(), ir, pre, blocks_per_batch=4, ctx=gpu_ctx)
    got = out[:, torch.from_numpy(pos).cuda()].cpu().numpy().astype(np.float64)
    want = chan_major(exact_final(dry, ir, pre, pos))
    err = float(np.max(np.abs(got - want)))
    print(f"60 s stereo, 16 blocks in 4 batches: max|ours - exact| at 64 positions per channel = {err:.3e} (bound {ULP:.3e})")
    assert err <= ULP
