"""Reverb impulse-response extraction -- drop-in for ``extract_reverb`` of the reference's ``handlers/reverb.py`` (:112-172), which the
Separate engine calls after a de-reverb transform ran on the vocals with ``store_reverb_ir`` (modules/separator/stem_separator.py:822-829)
and whose JSON file ``stems/impulse_response.ir`` survives stem pruning (wrappers/separate.py:383) for the Merge wrapper to re-apply.

Same signature and the same output file (keys, order, ``indent=2``).  ``dry`` / ``wet`` may be paths (WAV, read by audiolab_amd.wavio) or
float32 device tensors ``[C, N]`` -- the engine hands over the two stems it holds in HBM, no file round trip.  The whole-track work runs
in libalsep.so in double precision (csrc/reverb.hip): circular cross-correlation of the mono signals through one packed complex FFT
(``fft_xcorr`` :55-66), the Wiener quotient and its inverse transform for ANY track length (Bluestein; ``wiener_deconvolution`` :94-106),
the decay envelope (:74-81) and the magnitude spectrum of the impulse response (:155).  On the host: the Levenberg-Marquardt fit of
``estimate_rt60`` (scipy's ``curve_fit``, exactly the reference's call -- the fitted value depends on MINPACK's iteration path) and the
four scalar statistics of the <= 2 s impulse response that is brought to the host for the JSON file anyway.

Reference behaviours kept (oracle/reverb_oracle.py lists them; pinned by tests/golden/reverb.npz): the pre-delay is
``max(argmax - (len(dry) - 1), 0)`` of a correlation stored in circular order, i.e. 0 for realistic inputs; an odd-length wet signal
yields n - 1 samples.  One reference behaviour NOT kept: with numpy >= 2 (the reference pins 2.0.2) its ``json.dump`` raises on the
np.float32 ratios and leaves a truncated file behind (the call site logs "Error extracting IR"); this build writes the values.

``apply_reverb`` (:179-209) is the consumer of that file -- wrappers/merge.py:7,118 puts the room back on a processed vocal stem with it:
``clip(dry + 0.7 * pad(fftconvolve(dry_c, ir, "full"), (pre_delay_samples, 0))[:len(dry)], -1, 1)`` per channel.  Here the convolution is
overlap-save in double precision on the device (``alsep_reverb_apply``: blocks of 2^k >= 2 len(ir) points, two channels per complex
transform, a bounded workspace whatever the track length); ``apply_reverb_array`` is the entry point for stems already in device memory.
Kept: the pre-delay is ``int(params["pre_delay"] * sr)`` with the DRY file's rate (:187), whatever ``params["sample_rate"]`` says (a
WARNING is logged when they differ); a negative one raises ValueError as ``np.pad`` does (:197); the 0.7 wet gain and the clip (:205-206);
a ``.wav`` output is 16-bit PCM, ``sf.write``'s default for that extension (:208).  The reference's float32 transform of the dry signal
(scipy.fft keeps single precision) is not reproduced: this result is the exact convolution rounded to float32.
"""
from __future__ import annotations

import ctypes as C
import json
import logging
import os
from typing import Optional, Tuple, Union

import numpy as np
import torch

from . import _lib, wavio
from ._lib import AlsepError, Context

logger = logging.getLogger(__name__)

Audio = Union[str, torch.Tensor, np.ndarray]


def _load(x: Audio, ctx: Context, sr: Optional[int]) -> Tuple[torch.Tensor, int]:
    """-> (float32 [C, N] on the context's device, sample rate)"""
    if isinstance(x, str):
        audio, file_sr = wavio.read_wav(x)
        return torch.from_numpy(audio).to(ctx.device).contiguous(), file_sr
    if sr is None:
        raise AlsepError("extract_reverb: pass sr= with in-memory signals")
    t = torch.as_tensor(x, dtype=torch.float32)
    if t.dim() == 1:
        t = t[None]
    if t.dim() != 2:
        raise AlsepError("extract_reverb: signals are [channels, samples]")
    return t.to(ctx.device).contiguous(), int(sr)


def xcorr_argmax(ctx: Context, wet: torch.Tensor, dry: torch.Tensor, ws: torch.Tensor, probe_idx=None):
    """index of the first maximum of ``fft_xcorr(wet_mono, dry_mono)`` (:55-66, :130-131) [, the correlation at ``probe_idx``]"""
    out = C.c_int64()
    n_probe = 0 if probe_idx is None else len(probe_idx)
    pv = (C.c_double * max(n_probe, 1))()
    pi = (C.c_int64 * max(n_probe, 1))(*([int(i) for i in probe_idx] if n_probe else [0]))
    ctx.check(ctx.lib.alsep_reverb_xcorr_argmax(ctx.handle, _lib.ptr(wet), wet.shape[0], wet.shape[1], wet.shape[1], _lib.ptr(dry), dry.shape[0],
                                                dry.shape[1], dry.shape[1], _lib.ptr(ws), ws.numel(), C.byref(out), pv, pi, n_probe),
              "alsep_reverb_xcorr_argmax")
    return (int(out.value), np.array(pv[:n_probe])) if n_probe else int(out.value)


def wiener_ir(ctx: Context, wet: torch.Tensor, dry: torch.Tensor, eps: float, n_out: int, ws: torch.Tensor) -> torch.Tensor:
    """``wiener_deconvolution(wet_mono, dry_mono, eps)[:n_out]`` (:94-106, :142-143) as a float64 device tensor"""
    ir = ctx.empty((n_out,), torch.float64)
    written = C.c_int64()
    ctx.check(ctx.lib.alsep_reverb_wiener_ir(ctx.handle, _lib.ptr(wet), wet.shape[0], wet.shape[1], wet.shape[1], _lib.ptr(dry), dry.shape[0],
                                             dry.shape[1], dry.shape[1], float(eps), _lib.ptr(ws), ws.numel(), _lib.ptr(ir), n_out, C.byref(written)),
              "alsep_reverb_wiener_ir")
    return ir[: int(written.value)]


def envelope_db(ctx: Context, x: torch.Tensor) -> torch.Tensor:
    out = ctx.empty((x.shape[1],), torch.float32)
    ctx.check(ctx.lib.alsep_reverb_envelope_db(ctx.handle, _lib.ptr(x), x.shape[0], x.shape[1], x.shape[1], _lib.ptr(out)), "alsep_reverb_envelope_db")
    return out


def rfft_mag(ctx: Context, x: torch.Tensor) -> torch.Tensor:
    n = x.numel()
    need = 2 * n * 16 + int(ctx.lib.alsep_dft_f64_workspace_bytes(n))
    ws = ctx.empty((need,), torch.uint8)
    out = ctx.empty((n // 2 + 1,), torch.float64)
    ctx.check(ctx.lib.alsep_rfft_mag_f64(ctx.handle, _lib.ptr(x.contiguous()), n, _lib.ptr(ws), need, _lib.ptr(out)), "alsep_rfft_mag_f64")
    return out


def fit_decay(env_db: np.ndarray, sr: int, maxfev: int) -> float:
    """estimate_rt60's fit (:82-91): a exp(-b t) + c through the dB envelope by scipy's curve_fit from its default start; 3 / b"""
    from scipy.optimize import curve_fit
    time = np.linspace(0, len(env_db) / sr, len(env_db))

    def exp_decay(x, a, b, c):
        return a * np.exp(-b * x) + c
    popt, _ = curve_fit(exp_decay, time, env_db, maxfev=maxfev)
    decay_time = 3.0 / popt[1] if popt[1] != 0 else 0.5
    logger.info(f"Estimated decay time: {decay_time} sec (using maxfev={maxfev})")
    return float(max(decay_time, 0.01))


def extract_reverb_params(dry: Audio, wet: Audio, wiener_epsilon: float = 1e-6, curve_fit_maxfev: int = 5000, sr: Optional[int] = None,
                          ctx: Optional[Context] = None) -> dict:
    """the dictionary ``extract_reverb`` saves (:159-168)"""
    ctx = ctx if ctx is not None else _lib.default_context(None)
    dry_t, sr_d = _load(dry, ctx, sr)
    wet_t, sr_w = _load(wet, ctx, sr)
    if sr_d != sr_w:
        raise ValueError("Dry and wet sample rates must match.")
    sr = sr_d
    n_wet, n_dry = wet_t.shape[1], dry_t.shape[1]
    if n_wet < 2 or n_dry < 1:
        raise AlsepError("extract_reverb: signals are too short")
    need = int(ctx.lib.alsep_reverb_workspace_bytes(n_wet, n_dry))
    if need < 0:
        raise AlsepError(f"extract_reverb: {n_wet} / {n_dry} samples exceed the 2^27-point transform limit")
    ws = ctx.empty((need,), torch.uint8)
    best = xcorr_argmax(ctx, wet_t, dry_t, ws)
    best_shift = max(best - (n_dry - 1), 0)                                  # :131-132
    pre_delay_sec = best_shift / sr
    logger.info(f"Estimated pre-delay: {pre_delay_sec} sec")
    decay_time = fit_decay(envelope_db(ctx, wet_t).cpu().numpy(), sr, curve_fit_maxfev)
    ir_dev = wiener_ir(ctx, wet_t, dry_t, wiener_epsilon, int(sr * 2), ws)   # :142-143
    del ws
    mag = rfft_mag(ctx, ir_dev).cpu().numpy()
    ir = ir_dev.cpu().numpy()
    early = int(0.05 * sr)                                                   # :146-157 on the <= 2 s response
    early_energy = np.sum(np.square(ir[:early]))
    total_energy = np.sum(np.square(ir)) + 1e-10
    freqs = np.fft.rfftfreq(len(ir), d=1.0 / sr)
    return {
        "sample_rate": sr,
        "pre_delay": float(pre_delay_sec),
        "decay_time": float(decay_time),
        "early_reflection_ratio": float(early_energy / total_energy),
        "late_reverb_ratio": float((total_energy - early_energy) / total_energy),
        "diffusion": float(np.var(np.abs(ir))),
        "spectral_centroid": float(np.sum(freqs * mag) / (np.sum(mag) + 1e-10)),
        "impulse_response": ir.tolist(),
    }


def extract_reverb(dry_path: Audio, wet_path: Audio, param_output_path: str, wiener_epsilon: float = 1e-6, curve_fit_maxfev: int = 5000,
                   sr: Optional[int] = None, ctx: Optional[Context] = None) -> str:
    """handlers/reverb.py:112-172"""
    params = extract_reverb_params(dry_path, wet_path, wiener_epsilon, curve_fit_maxfev, sr=sr, ctx=ctx)
    with open(param_output_path, "w") as f:                                  # save_params_to_file, :39-42
        json.dump(params, f, indent=2)
    logger.info(f"Extracted parameters saved: {param_output_path}")
    return param_output_path


# ---- apply_reverb (:179-209) --------------------------------------------------------------------------------------------------------
WET_GAIN = 0.7                                                               # :205
MAX_WORKSPACE_BYTES = 1 << 30                                                # default batch: as many blocks as fit in 1 GiB


def load_params_from_file(param_path: str) -> dict:
    """handlers/reverb.py:44-46"""
    with open(param_path, "r") as file:
        return json.load(file)


def apply_reverb_array(dry, ir, pre_delay_samples: int, wet_gain: float = WET_GAIN, *, log2_block: int = 0, blocks_per_batch: int = 0,
                       ctx: Optional[Context] = None) -> torch.Tensor:
    """``clip(dry + wet_gain * pad(fftconvolve(dry_c, ir, "full"), (pre_delay_samples, 0))[:N], -1, 1)`` per channel (:192-206) as a
    float32 ``[C, N]`` device tensor.  ``dry``: float32 ``[C, N]`` or ``[N]``, tensor or array, device or host; ``ir``: float64 taps.
    ``log2_block`` forces the overlap-save block length (0: from len(ir)), ``blocks_per_batch`` the blocks transformed side by side
    (0: what a 1 GiB workspace holds); neither changes the result's value, the second not a bit of it."""
    ctx = ctx if ctx is not None else _lib.default_context(None)
    pre = int(pre_delay_samples)
    if pre < 0:
        raise ValueError("apply_reverb: the pre-delay can't be negative")    # np.pad's ValueError (:197)
    dry_t = torch.as_tensor(dry, dtype=torch.float32)
    if dry_t.dim() == 1:
        dry_t = dry_t[None]
    if dry_t.dim() != 2 or dry_t.shape[1] < 1:
        raise AlsepError("apply_reverb: signals are [channels, samples]")
    dry_t = dry_t.to(ctx.device).contiguous()
    ir_t = torch.as_tensor(ir, dtype=torch.float64).reshape(-1).to(ctx.device).contiguous()
    n_ir, (c, n) = ir_t.numel(), dry_t.shape
    k = int(ctx.lib.alsep_reverb_apply_block_log2(n_ir, log2_block))
    if k < 0:
        raise AlsepError(f"apply_reverb: an impulse response of {n_ir} taps with block exponent {log2_block} is not supported "
                         f"(1 .. 2^20 taps, 2^k >= 2 taps)")
    n_blocks = max(1, -(-(n - min(pre, n)) // ((1 << k) - n_ir + 1)))
    if blocks_per_batch <= 0:
        blocks_per_batch = max(1, (MAX_WORKSPACE_BYTES // (16 << k) - 1) // 2)
    need = int(ctx.lib.alsep_reverb_apply_workspace_bytes(n_ir, k, min(int(blocks_per_batch), n_blocks)))
    ws = ctx.empty((need,), torch.uint8)
    out = ctx.empty((c, n), torch.float32)
    ctx.check(ctx.lib.alsep_reverb_apply(ctx.handle, _lib.ptr(dry_t), c, n, n, _lib.ptr(ir_t), n_ir, pre, float(wet_gain), k, _lib.ptr(out), n,
                                         _lib.ptr(ws), need), "alsep_reverb_apply")
    return out


def apply_reverb(dry_path: Audio, param_path: Union[str, dict], output_path: str, sr: Optional[int] = None, ctx: Optional[Context] = None,
                 subtype: str = "PCM_16") -> str:
    """handlers/reverb.py:179-209.  ``dry_path``: a WAV path, or an in-memory signal with ``sr=``; ``param_path``: the JSON file
    ``extract_reverb`` wrote, or its dictionary.  Writes ``output_path`` (16-bit PCM as ``sf.write`` does for a .wav path, :208;
    ``subtype="FLOAT"`` for float32) and returns it."""
    ctx = ctx if ctx is not None else _lib.default_context(None)
    dry_t, sr = _load(dry_path, ctx, sr)
    params = param_path if isinstance(param_path, dict) else load_params_from_file(param_path)
    impulse_response = np.array(params["impulse_response"], dtype=np.float64)                # :186
    pre_delay_samples = int(params["pre_delay"] * sr)                                        # :187 -- the dry file's rate
    if "sample_rate" in params and params["sample_rate"] != sr:
        logger.warning(f"apply_reverb: the impulse response was extracted at {params['sample_rate']} Hz, the dry signal has {sr} Hz; "
                       f"applied sample by sample as the reference does")
    final = apply_reverb_array(dry_t, impulse_response, pre_delay_samples, WET_GAIN, ctx=ctx)
    wavio.write_wav(output_path, final.cpu().numpy(), sr, subtype=subtype)
    return output_path


def process_song(dry_path: str, wet_path: str, output_dir: str, ctx: Optional[Context] = None) -> str:
    """handlers/reverb.py:216-226"""
    param_file = os.path.join(output_dir, "reverb_params.json")
    output_file = os.path.join(output_dir, "reverb_applied.wav")
    extract_reverb(dry_path, wet_path, param_file, ctx=ctx)
    apply_reverb(dry_path, param_file, output_file, ctx=ctx)
    return output_file
