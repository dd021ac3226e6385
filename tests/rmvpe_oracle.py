"""The specification of audiolab_amd.rmvpe on the CPU: numpy and functional torch, written from the semantics of the reference's RMVPE
(log-mel front end, frame padding, the E2E network, the decode), pinned to the reference's own outputs by tests/golden/rmvpe.npz
(tests/test_rmvpe_oracle.py).  Weights come from ``audiolab_amd.rmvpe.synthetic_state_dict``: the one seeded helper the product's
``allow_synthetic`` path uses too, so no fixture has to hold weights."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from audiolab_amd.rmvpe import (BINS, BN_EPS, CENTS_OFFSET, GRU_HIDDEN, HOP, N_CLASS, N_FFT, N_MELS, RMVPEConfig, hann_window,
                                mel_filterbank_htk, param_shapes, synthetic_state_dict)

REDUCED = RMVPEConfig(n_blocks=1, n_gru=1, kernel_size=(2, 2), en_de_layers=2, inter_layers=1, in_channels=1, en_out_channels=4)
FULL = RMVPEConfig()


def test_signal(n=5280, seed=0):
    """a chirp upwards from 220 Hz plus noise, float32"""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64) / 16000.0
    phase = 2.0 * np.pi * (220.0 * t + 0.5 * 400.0 * t * t)
    return (0.5 * np.sin(phase) + 0.05 * rng.standard_normal(n)).astype(np.float32)


def mel_linear(audio):
    """float32 [n] -> float32 [128, T]: the filterbank product of the float32 magnitudes, before the clamp and the log.  The track is
    reflected by 512 samples (numpy folds as often as a short track needs), the transform is the product with the windowed float32 basis"""
    x = np.pad(np.asarray(audio, dtype=np.float32), N_FFT // 2, mode="reflect")
    T = len(audio) // HOP + 1
    frames = np.lib.stride_tricks.as_strided(x, (T, N_FFT), (HOP * x.strides[0], x.strides[0]))
    k = np.arange(BINS, dtype=np.float64)[:, None] * np.arange(N_FFT, dtype=np.float64)[None, :]
    ang = 2.0 * np.pi * (k % N_FFT) / N_FFT
    win = hann_window()
    re_b, im_b = np.cos(ang).astype(np.float32) * win, (-np.sin(ang)).astype(np.float32) * win
    fr = torch.from_numpy(np.ascontiguousarray(frames))
    re, im = fr @ torch.from_numpy(re_b).t(), fr @ torch.from_numpy(im_b).t()
    mag = torch.sqrt(re * re + im * im)                                       # [T, 513]
    return (torch.from_numpy(mel_filterbank_htk()) @ mag.t()).numpy()


def log_mel(audio):
    return np.log(np.maximum(mel_linear(audio), np.float32(1e-5)))


def padded_frames(T):
    pad = min(32 * ((T - 1) // 32 + 1) - T, T)
    if pad > T - 1:
        raise ValueError(f"{T} frames cannot be reflected by {pad}")
    return pad


def _bn(sd, p, x):
    return F.batch_norm(x, sd[p + ".running_mean"], sd[p + ".running_var"], sd[p + ".weight"], sd[p + ".bias"], False, 0.0, BN_EPS)


def _block(sd, p, x, trace):
    y = F.relu(_bn(sd, p + ".conv.1", F.conv2d(x, sd[p + ".conv.0.weight"], padding=1)))
    y = F.relu(_bn(sd, p + ".conv.4", F.conv2d(y, sd[p + ".conv.3.weight"], padding=1)))
    if (p + ".shortcut.weight") in sd:
        x = F.conv2d(x, sd[p + ".shortcut.weight"], sd[p + ".shortcut.bias"])
    out = y + x
    if trace is not None:
        trace.append((p, out))
    return out


@functools.lru_cache(maxsize=None)
def _gru_module(device):
    return torch.nn.GRU(3 * N_MELS, GRU_HIDDEN, num_layers=1, batch_first=True, bidirectional=True).eval().to(device)


def network(sd, cfg, logmel, trace=None, device="cpu"):
    """the log-mel float32 [128, T] -> the salience float32 [T, 360]; ``trace`` collects (name, activation) of every block; ``device``: where
    torch runs it (the benchmark times this restatement on the GPU too; ``sd`` must live there)"""
    with torch.no_grad():
        m = torch.from_numpy(np.ascontiguousarray(logmel, dtype=np.float32))[None].to(device)   # [1, 128, T]
        T = m.shape[-1]
        m = F.pad(m, (0, padded_frames(T)), mode="reflect")
        x = _bn(sd, "unet.encoder.bn", m.transpose(-1, -2).unsqueeze(1))                       # [1, 1, Tp, 128]
        skips = []
        for i in range(cfg.en_de_layers):
            for b in range(cfg.n_blocks):
                x = _block(sd, f"unet.encoder.layers.{i}.conv.{b}", x, trace)
            skips.append(x)
            x = F.avg_pool2d(x, 2)
        for i in range(cfg.inter_layers):
            for b in range(cfg.n_blocks):
                x = _block(sd, f"unet.intermediate.layers.{i}.conv.{b}", x, trace)
        for i in range(cfg.en_de_layers):
            p = f"unet.decoder.layers.{i}"
            x = F.relu(_bn(sd, p + ".conv1.1", F.conv_transpose2d(x, sd[p + ".conv1.0.weight"], stride=2, padding=1, output_padding=1)))
            if trace is not None:
                trace.append((p + ".conv1", x))
            x = torch.cat((x, skips[-1 - i]), dim=1)
            for b in range(cfg.n_blocks):
                x = _block(sd, f"{p}.conv2.{b}", x, trace)
        x = F.conv2d(x, sd["cnn.weight"], sd["cnn.bias"], padding=1)                           # [1, 3, Tp, 128]
        x = x.transpose(1, 2).flatten(-2)                                                     # [1, Tp, 384], channel major
        g = _gru_module(str(device))
        g.load_state_dict({k[len("fc.0.gru."):]: v for k, v in sd.items() if k.startswith("fc.0.gru.")})
        h = g(x)[0]
        sal = torch.sigmoid(F.linear(h, sd["fc.1.weight"], sd["fc.1.bias"]))
        return sal[0, :T].cpu().numpy()


def decode(salience, thred=0.03):
    """float32 [T, 360] -> float64 [T]: the argmax (lowest index on a tie), the salience-weighted mean of the cents of the 9 bins around it
    (zeros beyond the ends) -- the products and their sum in float64, the sum of the weights in float32, as numpy does both for a float32
    salience -- f0 = 10 2^(cents / 1200); 0 where the largest salience <= thred (compared in float32) and where f0 is exactly 10"""
    s = np.asarray(salience, dtype=np.float32)
    cents = np.pad(20.0 * np.arange(N_CLASS) + CENTS_OFFSET, 4)
    sp = np.pad(s, ((0, 0), (4, 4)))
    c = np.argmax(s, axis=1)
    idx = c[:, None] + np.arange(9)[None, :]
    w = np.ascontiguousarray(np.take_along_axis(sp, idx, axis=1))
    num = np.sum(w * cents[idx], 1)
    den = np.sum(w, 1)
    with np.errstate(invalid="ignore", divide="ignore"):
        v = num / den
    v[np.max(s, axis=1) <= np.float32(thred)] = 0
    f0 = 10.0 * 2.0 ** (v / 1200.0)
    f0[f0 == 10] = 0
    return f0


def margins(salience):
    """the lead of every frame's largest salience over its second largest"""
    top = np.sort(np.asarray(salience), axis=1)
    return top[:, -1] - top[:, -2]


@functools.lru_cache(maxsize=None)
def weights(full=False, seed=0):
    return synthetic_state_dict(FULL if full else REDUCED, seed)
