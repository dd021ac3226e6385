"""CPU (-m "not gpu"): the Demucs bag runner sharded over world 2 (gloo, kernels emulated on the CPU) -- units of all views split over the
ranks, one seam all-gather, one all-gather of the finished spans -- against the single-process bag oracle; and the split-contraction
re-run agreed across the ranks: a rank whose operands left the half range makes EVERY rank run the track again (a rank-local re-run
would issue its collectives alone and wait for ever)."""
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


def _worker_bag(rank, world, port, emul_so, out_path):
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
    from tests.test_demucs_bag import bag_oracle
    ocfg = ho.HTDemucsConfig(sources=("drums", "bass", "other"), channels=16, nfft=256, depth=2, dconv_comp=4, bottom_channels=32, t_layers=2,
                             t_heads=4, segment_samples=2560, samplerate=4000)
    sds = [ho.synthetic_state_dict(ocfg, s) for s in (5, 6)]
    nets = [HTDemucs(HTDemucsConfig(**dataclasses.asdict(ocfg)), sd, ctx=ctx) for sd in sds]
    weights = [[1.0, 0.5, 0.0], [0.0, 1.0, 2.0]]                   # the views carry different sources
    hm = torch.randn(2, 3100, generator=torch.Generator().manual_seed(8)) * 0.2
    want = bag_oracle([ocfg, ocfg], sds, weights, hm, shifts=2, seed=3)
    res = []
    ctx.launch_counts_reset()
    out = DemucsRunner(nets, shifts=2, overlap=0.25, seed=3, sharded=True, weights=weights).separate(hm)
    res.append(float(max(np.max(np.abs(out[k].numpy() - want[i])) for i, k in enumerate(ocfg.sources))))
    res.append(float(ctx.launch_count("demucs_bag_finish_kernel")))
    # contraction="split", the half range left on rank 0 only: both ranks must run the track a second time
    runs = [0]
    real_separate = DemucsRunner._separate

    def counting(self, mix):
        runs[0] += 1
        return real_separate(self, mix)
    DemucsRunner._separate = counting
    if rank == 0:
        _lib.Context.nn_range_exceeded = lambda self: True
    out = DemucsRunner(nets, shifts=2, overlap=0.25, seed=3, sharded=True, weights=weights, contraction="split").separate(hm)
    res.append(float(max(np.max(np.abs(out[k].numpy() - want[i])) for i, k in enumerate(ocfg.sources))))
    res.append(float(runs[0]))
    t = torch.tensor(res).reshape(1, -1)
    got = [torch.zeros_like(t) for _ in range(world)]
    dist.all_gather(got, t)
    if rank == 0:
        np.save(out_path, torch.cat(got).numpy())
    dist.barrier()
    dist.destroy_process_group()


def test_sharded_bag_world2_gloo(emul_lib_path, tmp_path):
    out_path = str(tmp_path / "bag2.npy")
    mp.spawn(_worker_bag, args=(2, _free_port(), emul_lib_path, out_path), nprocs=2, join=True)
    r = np.load(out_path)                                        # [rank, (err, finish launches, err split, runs of the track)]
    assert np.all(r[:, 0] < 1e-4), f"sharded bag runner: {r[:, 0]}"
    assert np.all(r[:, 1] == 1)
    assert np.all(r[:, 2] < 1e-4), f"sharded bag runner, split contraction re-run: {r[:, 2]}"
    assert np.all(r[:, 3] == 2), f"runs of the track per rank: {r[:, 3]}"
