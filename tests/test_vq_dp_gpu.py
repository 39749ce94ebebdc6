"""The codebook under data parallel, rehearsed on ONE GPU like tests/test_dp_gpu.py: two ranks share cuda:0 and exchange through gloo.
Each rank initialises the codebook with k-means and runs two training-mode forwards on its half of a batch: the ranks end bit-identical
(packed counts | sums all-reduced, re-seed rows and initial means from rank 0) and equal to one rank on the whole batch up to the order
of the fp32 additions.  A one-rank process group issues no collective."""
import os
import socket
import time

import numpy as np
import pytest
import torch

from tests import vq_ref as VR

pytestmark = pytest.mark.gpu
BUFFERS = ("embed", "embed_avg", "cluster_size")
TIMEOUT = 180.0


@pytest.fixture(autouse=True)
def _keep_compute_dtype():
    import frankenstein_amd as fa
    from frankenstein_amd import engine as E
    before = E.compute_dtype()
    yield
    fa.set_compute_dtype(before)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run(rank, world, rows):
    """planted data, 8 codes, given initial means (nothing random decides the result: comparable with one rank on the whole batch), then a
    64-code quantiser on the same rows whose many unused codes are re-seeded at random (comparable between the ranks only)"""
    import frankenstein_amd as fa
    from frankenstein_amd.models import vq_brain as vq
    fa.set_compute_dtype("fp32")
    x, init, _ = VR.planted()
    x = torch.from_numpy(x).cuda()
    mine = x[rank * rows:(rank + 1) * rows].view(1, rows, -1)
    out = {}
    torch.manual_seed(0)
    small, big = vq.VectorQuantize(16, 8, kmeans_init=True).cuda().train(), vq.VectorQuantize(16, 64, kmeans_init=True).cuda().train()
    torch.manual_seed(100 + rank)                       # from here on every rank draws its own random numbers
    small.init_codebook_(mine, iters=3, init_means=torch.from_numpy(init))
    big.init_codebook_(mine, iters=3)
    for name, m in (("small", small), ("big", big)):
        for _ in range(2):
            q, idx, commit = m(mine)
            assert torch.isfinite(commit) and q.shape == mine.shape
        torch.cuda.synchronize()
        for b in BUFFERS:
            out[f"{name}.{b}"] = getattr(m._codebook, b).detach().cpu().numpy()
    return out


def _worker(rank, world, port, out):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    calls = []
    for fn in ("all_reduce", "broadcast"):
        orig = getattr(dist, fn)
        setattr(dist, fn, lambda *a, _o=orig, _n=fn, **k: (calls.append(_n), _o(*a, **k))[1])
    res = _run(rank, world, 400 // world)
    res["calls"] = list(calls)
    out[rank] = res
    dist.destroy_process_group()


def _spawn(world):
    import torch.multiprocessing as mp
    out = mp.get_context("spawn").Manager().dict()
    ctx = mp.spawn(_worker, args=(world, _free_port(), out), nprocs=world, join=False)
    deadline = time.monotonic() + TIMEOUT
    while not ctx.join(timeout=2.0):
        if time.monotonic() > deadline:
            for p in ctx.processes:
                p.kill()
            pytest.fail(f"the {world}-rank rehearsal did not finish within {TIMEOUT:.0f} s")
    assert len(out) == world
    return [out[r] for r in range(world)]


def test_two_ranks_hold_one_codebook():
    r0, r1 = _spawn(2)
    for name in ("small", "big"):
        for b in BUFFERS:
            np.testing.assert_array_equal(r0[f"{name}.{b}"], r1[f"{name}.{b}"], err_msg=f"{name}.{b} differs between the ranks")
    # 3 k-means rounds + 2 EMA steps per quantiser: one all-reduce each; the means once and the seed rows of every EMA step from rank 0
    assert r0["calls"].count("all_reduce") == 10 and r0["calls"].count("broadcast") == 6, r0["calls"]
    one = _run(0, 1, 400)                                # this process: no process group, the whole batch
    for b in BUFFERS:
        err = np.abs(r0[f"small.{b}"].astype(np.float64) - one[f"small.{b}"]) / np.maximum(1.0, np.abs(one[f"small.{b}"]))
        print(f"two ranks vs one rank, {b}: {err.max():.3g}")
        assert err.max() <= 1e-5


def test_one_rank_group_issues_no_collective():
    (r0,) = _spawn(1)
    assert r0["calls"] == []
    assert np.isfinite(r0["small.embed"]).all() and r0["small.cluster_size"].shape == (1, 8)
