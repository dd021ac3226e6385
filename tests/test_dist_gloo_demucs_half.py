"""CPU (-m "not gpu"): the half-precision Demucs runner sharded over world 2 (gloo, kernels emulated on the CPU) -- batched units of each
rank's shard, the seam all-gather and the finished-span all-gather -- against the single-process half-precision runner; and the float32
re-run of a track whose half-precision stems are not finite, agreed across the ranks: a non-finite result on rank 0 alone makes EVERY
rank run the track again in float32 (a rank-local re-run would issue its collectives alone and wait for ever)."""
import dataclasses
import datetime
import os
import socket

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, emul_so, out_path):
    import sys
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=120))
    from audiolab_amd import _lib
    _lib._LIB = _lib.bind(emul_so)
    _lib.DEVICE_TYPE = "cpu"
    ctx = _lib.Context("cpu")
    from audiolab_amd.htdemucs import DemucsRunner, HTDemucs, HTDemucsConfig
    from oracle import htdemucs_oracle as ho
    ocfg = ho.HTDemucsConfig(sources=("drums", "bass", "other"), channels=16, nfft=256, depth=2, dconv_comp=4, bottom_channels=64, t_layers=2,
                             t_heads=1, segment_samples=2560, samplerate=4000)
    sds = [ho.synthetic_state_dict(ocfg, s) for s in (5, 6)]
    nets = [HTDemucs(HTDemucsConfig(**dataclasses.asdict(ocfg)), sd, ctx=ctx, precision="f16") for sd in sds]
    weights = [[1.0, 0.5, 0.0], [0.0, 1.0, 2.0]]
    hm = torch.randn(2, 3100, generator=torch.Generator().manual_seed(8)) * 0.2
    want = DemucsRunner(nets, shifts=2, seed=3, weights=weights, batch=3).separate(hm)               # one process
    want32 = DemucsRunner([n.as_f32() for n in nets], shifts=2, seed=3, weights=weights, lanes=1).separate(hm)
    res = []
    r = DemucsRunner(nets, shifts=2, seed=3, sharded=True, weights=weights, batch=3)
    out = r.separate(hm)
    res.append(float(max(np.max(np.abs(out[k].numpy() - want[k].numpy())) for k in ocfg.sources)))
    res.append(float(r.batches_run))
    # non-finite stems on rank 0 only: both ranks run the track a second time, in float32
    runs = [0]
    real_separate = DemucsRunner._separate

    def counting(self, mix):
        runs[0] += 1
        return real_separate(self, mix)
    DemucsRunner._separate = counting
    r2 = DemucsRunner(nets, shifts=2, seed=3, sharded=True, weights=weights, batch=3)
    if rank == 0:
        r2._stems_finite = lambda o: False
    out = r2.separate(hm)
    res.append(float(max(np.max(np.abs(out[k].numpy() - want32[k].numpy())) for k in ocfg.sources)))
    res.append(float(runs[0]))
    t = torch.tensor(res).reshape(1, -1)
    got = [torch.zeros_like(t) for _ in range(world)]
    dist.all_gather(got, t)
    if rank == 0:
        np.save(out_path, torch.cat(got).numpy())
    dist.barrier()
    dist.destroy_process_group()


def test_sharded_half_runner_world2_gloo(emul_lib_path, tmp_path):
    out_path = str(tmp_path / "half2.npy")
    mp.spawn(_worker, args=(2, _free_port(), emul_lib_path, out_path), nprocs=2, join=True)
    r = np.load(out_path)                                        # [rank, (err, batches, err of the float32 re-run, runs of the track)]
    assert np.all(r[:, 0] < 1e-5), f"sharded half runner vs one process: {r[:, 0]}"
    assert np.all(r[:, 1] >= 1), f"batched forwards per rank: {r[:, 1]}"
    assert np.all(r[:, 2] < 1e-5), f"sharded float32 re-run: {r[:, 2]}"
    assert np.all(r[:, 3] == 2), f"runs of the track per rank: {r[:, 3]}"
