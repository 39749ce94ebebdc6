"""run_train_model and GraphedTrainStep as a data-parallel run, rehearsed on ONE GPU: two spawned ranks share cuda:0 and exchange
through gloo (FK_DIST_BACKEND=gloo: RCCL refuses two ranks on one device).  The ranks get nothing but the launcher's environment
(RANK, WORLD_SIZE, LOCAL_RANK, MASTER_ADDR/PORT): run_train_model creates and destroys the process group itself, splits each
global batch on the host, evaluates every rank's shard, and only rank 0 logs and saves.  The same run as one process is the
yardstick (2 ranks x half batch == 1 rank x full batch, tests/test_dp_gpu.py's tolerances)."""
import math
import os

import numpy as np
import pytest
import torch

from tests.test_dp_gpu import _build, _free_port

# torch's DataLoader pins with a `device` argument that torch itself has deprecated (pin_memory=True, the TrainConfig default)
pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore:The argument 'device' of Tensor:DeprecationWarning")]


@pytest.fixture(autouse=True)
def _restore_dtype():
    yield
    import frankenstein_amd as fa
    fa.set_compute_dtype("bf16")


class _DS(torch.utils.data.Dataset):
    """sample i: (inputs [32, 16], targets [8, 12], i) — the index rides in the date_info slot, which BrainFormer ignores"""

    def __init__(self, n, seed):
        g = torch.Generator().manual_seed(seed)
        self.x = torch.randn(n, 32, 16, generator=g)
        self.y = torch.randn(n, 8, 12, generator=g)

    def __len__(self):
        return len(self.x)

    def __getitem__(self, i):
        return self.x[i], self.y[i], torch.tensor(i)


def _run(n_train, max_steps, eval_interval, save_folder):
    """run_train_model on the small L1 BrainFormer; every forward recorded as [training, input shape, sample ids, loss]"""
    from frankenstein_amd.utils import train_utils as tu
    m = _build()
    rec, logs = [], []

    def pre(mod, args, kwargs):
        ids = kwargs["date_info"] if "date_info" in kwargs else args[2]
        rec.append([mod.training, tuple(args[0].shape), ids.tolist(), None])

    def post(mod, args, kwargs, out):
        rec[-1][3] = float(out[0].detach())

    m.register_forward_pre_hook(pre, with_kwargs=True)
    m.register_forward_hook(post, with_kwargs=True)
    cfg = tu.TrainConfig(exp_name="dp", batch_size=4, max_steps=max_steps, eval_interval=eval_interval, num_workers=0, pin_memory=True,
                         mixed_precision=False, use_scheduler=False, learning_rate=3e-4)
    tu.run_train_model(m, (_DS(n_train, 0), _DS(4, 1)), cfg, save_folder=save_folder, logger=lambda d, s: logs.append((s, dict(d))))
    flat = torch.cat([p.detach().reshape(-1) for p in m.parameters()]).cpu().numpy()
    return dict(rec=rec, logs=logs, flat=flat)


def _driver_worker(rank, world, port, folder, n_train, max_steps, eval_interval, out):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      FK_DIST_BACKEND="gloo")
    import torch.distributed as dist
    r = _run(n_train, max_steps, eval_interval, folder)
    r["group_after"] = dist.is_initialized()
    out[rank] = r


def _spawn(world, *args):
    import torch.multiprocessing as mp
    out = mp.get_context("spawn").Manager().dict()
    mp.spawn(_driver_worker, args=(world, _free_port(), *args, out), nprocs=world, join=True)
    assert sorted(out.keys()) == list(range(world))
    return [out[r] for r in range(world)]


def _forwards(r, training):
    return [x for x in r["rec"] if x[0] == training]


def _logged(r, key):
    return [(s, d[key]) for s, d in r["logs"] if key in d]


def test_run_train_model_two_ranks_equal_one_process(tmp_path):
    import safetensors.torch
    import torch.distributed as dist
    world, n_steps = 2, 7                               # max_steps 6: the loop stops once overall_step > 6
    ranks = _spawn(world, str(tmp_path / "dp"), 12, 6, 3)
    one = _run(12, 6, 3, tmp_path / "one")
    assert not dist.is_initialized()
    # the replicas are one model, and the one-process model up to rounding (Adam turns rounding-level gradient differences of
    # (near-)zero-gradient entries into +-lr updates: tests/test_dp_gpu.py's robust comparison)
    np.testing.assert_array_equal(ranks[0]["flat"], ranks[1]["flat"])
    diff = np.abs(ranks[0]["flat"] - one["flat"])
    assert np.quantile(diff, 0.99) < 2e-5 and diff.max() < 5e-3, (np.quantile(diff, 0.99), diff.max())
    # the group run_train_model created is gone; rank 1 logged nothing
    assert [r["group_after"] for r in ranks] == [False, False]
    assert ranks[1]["logs"] == []
    # each rank's forward saw its half of the global batch, in order: rank 0's ids then rank 1's are the one-process batch
    one_train, one_eval = _forwards(one, True), _forwards(one, False)
    assert len(one_train) == n_steps and len(one_eval) == 2
    assert {x[1] for x in one_train + one_eval} == {(4, 32, 16)}
    for r in ranks:
        assert len(_forwards(r, True)) == n_steps and len(_forwards(r, False)) == 2
        assert {x[1] for x in r["rec"]} == {(2, 32, 16)}
    for s in range(n_steps):
        assert _forwards(ranks[0], True)[s][2] + _forwards(ranks[1], True)[s][2] == one_train[s][2], s
    for e in range(2):
        assert _forwards(ranks[0], False)[e][2] + _forwards(ranks[1], False)[e][2] == one_eval[e][2]
    # rank 0 logged its own shard's loss; the two shards' mean is the one-process loss
    logged = _logged(ranks[0], "train/loss")
    assert [s for s, _ in logged] == list(range(1, n_steps + 1))
    assert [l for _, l in logged] == [x[3] for x in _forwards(ranks[0], True)]
    for s, (_, want) in enumerate(_logged(one, "train/loss")):
        mean = (_forwards(ranks[0], True)[s][3] + _forwards(ranks[1], True)[s][3]) / 2
        assert abs(mean - want) <= 1e-5 * abs(want), (s, mean, want)
    # the validation loss is all ranks' shards averaged: the one-process value
    val, one_val = _logged(ranks[0], "val/loss"), _logged(one, "val/loss")
    assert [s for s, _ in val] == [s for s, _ in one_val] == [3, 6]
    for (_, got), (_, want) in zip(val, one_val):
        assert abs(got - want) <= 1e-5 * abs(want), (got, want)
    # one checkpoint per improving evaluation, written once, loadable into a fresh model
    best, want_files = math.inf, []
    for s, v in val:
        if v < best:
            best = v
            want_files.append(f"step_{s}_loss_{v:.4f}.safetensors")
    folder = tmp_path / "dp" / "dp"
    assert sorted(p.name for p in folder.iterdir()) == sorted(want_files)
    m2 = _build()
    for name in want_files:
        safetensors.torch.load_model(m2, str(folder / name))
        assert set(safetensors.torch.load_file(str(folder / name))) == set(m2.state_dict())


def test_run_train_model_last_partial_batch_wraps_around_like_accelerate(tmp_path):
    """10 samples, global batch 4: the last step of every epoch gives rank 0 that epoch's samples 9 and 10 and rank 1 its first two,
    in that epoch's order (accelerate's even_batches); the epoch order is the one-process run's"""
    world = 2
    ranks = _spawn(world, str(tmp_path / "dp"), 10, 5, 10 ** 6)
    one = _run(10, 5, 10 ** 6, tmp_path / "one")
    ids = [[x[2] for x in _forwards(r, True)] for r in ranks]
    one_ids = [x[2] for x in _forwards(one, True)]
    assert len(ids[0]) == len(ids[1]) == len(one_ids) == 6          # two epochs of three steps
    for e in range(2):
        s = 3 * e
        order = ids[0][s] + ids[1][s] + ids[0][s + 1] + ids[1][s + 1] + ids[0][s + 2]
        assert sorted(order) == list(range(10))
        assert order == one_ids[s] + one_ids[s + 1] + one_ids[s + 2]
        assert ids[0][s + 2] == order[8:10] and ids[1][s + 2] == order[0:2]
    assert ids[0][0] + ids[1][0] != ids[0][3] + ids[1][3]             # shuffled anew each epoch


def _graphed_worker(rank, world, port, out):
    """eager DP (train_step: buckets all-reduced from the backward's hooks) against GraphedTrainStep (replay, then every bucket
    at once) on the same shards"""
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      FK_DIST_BACKEND="gloo")
    import torch.distributed as dist
    from frankenstein_amd.utils import train_utils as tu
    assert tu.init_distributed() == (rank, world, True)
    cfg = tu.TrainConfig(mixed_precision=False, use_scheduler=False, learning_rate=1e-3)
    g = torch.Generator().manual_seed(7)
    batches = [(torch.randn(4, 32, 16, generator=g), torch.randn(4, 8, 12, generator=g), None) for _ in range(3)]
    shards = [tuple(t.cuda() if torch.is_tensor(t) else t for t in tu.shard_batch(b, rank, world)) for b in batches]
    res = {}
    for mode in ("eager", "graphed"):
        m = _build()
        opt = tu.FusedAdamW(m, lr=cfg.learning_rate, weight_decay=cfg.weight_decay, grad_clip=cfg.grad_clip, bucket_bytes=64 << 10)
        assert opt.sync.world == world and len(opt.sync.buckets) > 1
        if mode == "graphed":
            step = tu.GraphedTrainStep(m, shards[0], opt, cfg)
            losses = [float(step(b, i)) for i, b in enumerate(shards)]
        else:
            losses = [float(tu.train_step(m, b, opt, i, cfg)) for i, b in enumerate(shards)]
        torch.cuda.synchronize()
        assert opt.t == len(shards)
        res[mode] = (losses, opt.arena.flat.cpu().numpy(), opt.m.cpu().numpy())
    out[rank] = res
    dist.destroy_process_group()


def test_graphed_train_step_data_parallel_is_bit_identical_to_eager():
    import torch.multiprocessing as mp
    world = 2
    out = mp.get_context("spawn").Manager().dict()
    mp.spawn(_graphed_worker, args=(world, _free_port(), out), nprocs=world, join=True)
    for r in range(world):
        eager, graphed = out[r]["eager"], out[r]["graphed"]
        assert eager[0] == graphed[0], (r, eager[0], graphed[0])
        np.testing.assert_array_equal(eager[1], graphed[1])
        np.testing.assert_array_equal(eager[2], graphed[2])
    np.testing.assert_array_equal(out[0]["graphed"][1], out[1]["graphed"][1])       # the replicas stay one model
    assert out[0]["graphed"][0] != out[1]["graphed"][0]                              # ... trained on different shards
