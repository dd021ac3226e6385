"""demucs LocalState on the kernels: the fused distance-decay bias / diagonal mask / softmax (alsep_nn_localstate_softmax) alone, and the
whole operator (one 1x1 projection, two strided batched GEMMs around that kernel, the output projection) against the float64 restatement.
Both on the CPU emulation and on the GPU through ``dev``; T 1723 (hdemucs_mmi's layer 4 at 40 s) of the whole operator on the GPU only."""
import math

import numpy as np
import pytest
import torch

from tests.conftest import host, on
from tests.hdemucs_oracle import local_state as local_state_ref


def _softmax_ref(scores: torch.Tensor, qd: torch.Tensor, heads: int, nd: int) -> torch.Tensor:
    """float64: scores [B, heads, T(s), T(t)], qd [B, T, heads * nd] -> softmax over t of scores + bias, diagonal -100"""
    B, _, T, _ = scores.shape
    idx = torch.arange(T, dtype=torch.float64)
    dist = (idx[None, :] - idx[:, None]).abs()                                        # [s, t]
    f = torch.arange(1, nd + 1, dtype=torch.float64)
    dq = torch.sigmoid(qd.view(B, T, heads, nd)) / 2                                   # [B, s, h, f]
    D = (dq * f / math.sqrt(nd)).sum(-1).permute(0, 2, 1)                              # [B, h, s]
    v = scores - dist[None, None] * D[..., None]
    v = v.masked_fill(torch.eye(T, dtype=torch.bool), -100)
    return torch.softmax(v, dim=-1)


@pytest.mark.parametrize("T", [1, 2, 200, 1723])
@pytest.mark.parametrize("bias", [-6.0, 0.0, 4.0])
def test_localstate_softmax_kernel(dev, T, bias):
    """query_decay outputs around -6 (sigmoid ~ 0: almost no decay), 0 and +4 (strong decay)"""
    B, heads, nd = 2, 4, 4
    g = torch.Generator().manual_seed(T)
    Tp = -(-T // 4) * 4
    scores = torch.randn(B, heads, T, T, generator=g, dtype=torch.float64) * 3
    qd = bias + torch.randn(B, T, heads * nd, generator=g, dtype=torch.float64)
    padded = torch.zeros(B * heads * T, Tp)
    padded[:, :T] = scores.reshape(-1, T).float()
    x, qd_d = on(dev, padded), on(dev, qd.float().contiguous())              # device tensors kept alive across the call
    dev.check(dev.lib.alsep_nn_localstate_softmax(dev.handle, x.data_ptr(), qd_d.data_ptr(), B, heads, T, Tp, nd, heads * nd),
              "alsep_nn_localstate_softmax")
    got = host(x)[:, :T].reshape(B, heads, T, T)
    want = _softmax_ref(scores.float().double(), qd.float().double(), heads, nd).numpy()
    err = float(np.max(np.abs(got - want)))
    assert err < 2e-6, f"T={T} bias={bias}: max |delta| = {err:.3e}"
    np.testing.assert_allclose(got.sum(-1), 1.0, atol=1e-5)
    if T > 1:
        assert np.all(np.diagonal(got, axis1=2, axis2=3) < 1e-30 + np.exp(-90.0))   # the masked diagonal


def _ls_sd(C: int, seed: int, decay_bias: float):
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for n, co in (("content", C), ("query", C), ("key", C), ("proj", C), ("query_decay", 16)):
        sd[f"a.{n}.weight"] = (torch.rand(co, C, 1, generator=g, dtype=torch.float64) * 2 - 1) / math.sqrt(C)
        sd[f"a.{n}.bias"] = (torch.rand(co, generator=g, dtype=torch.float64) * 2 - 1) / math.sqrt(C)
    sd["a.query_decay.bias"] = sd["a.query_decay.bias"] + decay_bias
    return sd


@pytest.mark.parametrize("dh", [48, 96])
@pytest.mark.parametrize("T", [1, 2, 200, 1723])
@pytest.mark.parametrize("decay_bias", [-2.0, 0.0, 3.0])
def test_localstate_operator(dev, dh, T, decay_bias):
    if dev.device.type == "cpu" and (T > 200 or dh > 48):
        pytest.skip("the emulation covers T <= 200 and head size 48")
    from audiolab_amd.hdemucs import DConvOps, localstate_params
    C, G = 4 * dh, 2
    sd = _ls_sd(C, dh + T, decay_bias)
    x = torch.randn(G, C, T, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    ops = DConvOps(dev)
    P = localstate_params(dev, {k: v.float() for k, v in sd.items()}, "a")
    got = host(ops._local_state(on(dev, x.permute(0, 2, 1).float().contiguous()), G, T, C, P)).reshape(G, T, C).transpose(0, 2, 1)
    want = local_state_ref(sd, "a", x).numpy()
    err = float(np.max(np.abs(got - want)))
    assert err < 1e-4, f"LocalState dh={dh} T={T} decay bias {decay_bias}: max |delta| = {err:.3e} (peak {np.max(np.abs(want)):.2f})"
