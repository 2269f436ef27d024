"""Gradient clipping under data parallelism, with spawned workers and the helpers of tests/test_dp_rccl_gpu.py: with clipping on the step
takes the all-reduce scheme (the layer-segmented overlap stays), so after the exchange every rank holds the whole reduced gradient and
computes the same norm bits with no further collective.
  * one rank, backend "nccl" (MTN_FORCE_DIST=1), every slice really all-reduced through RCCL: weights, moments, losses and norms equal,
    BIT FOR BIT, the same schedule with the collectives skipped; and the two-graph schedule (overlap=False: monolithic backward, the
    whole-buffer all-reduce, the optimiser) equals the plain clipped TrainStep without any grad_sync, bit for bit;
  * asking for the sharded optimiser together with clipping raises, naming it;
  * two ranks, one GPU each — skipped unless the box has two GPUs, as in that file: both ranks report identical norm bits, and N ranks x half
    batch == one rank x whole batch at that file's tolerance."""
import os
import sys

import numpy as np
import pytest
import torch

from tests.test_dp_rccl_gpu import _batch, _cfg, _free_port, _make, _run_steps

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = 2


def _clipped_steps(model, batch, c, sync, use_graph, C, **kw):
    """_run_steps with clipping at C, plus the norm bits of the last step and the stats block."""
    step, losses, st = _run_steps(model, batch, c, sync, use_graph, n=STEPS, clip_grad_norm=C, **kw)
    assert step.clipping and step.sharded is None
    st = dict(st, losses=losses, norm=step.last_grad_norm.detach().cpu().clone(), stats=step.opt.optimizer.clip_stats())
    return step, st


def _measure(c, raw, dev, dtype, drop, sync=None):
    """Half of step 1's gradient norm on this batch, as a float32: a cap that clips."""
    torch.manual_seed(0)
    model = _make(c, dev, dtype, drop)
    step, _, _ = _run_steps(model, _batch(c, raw, dev), c, sync, False, n=1, clip_grad_norm=float("inf"))
    return float(np.float32(0.5 * float(step.last_grad_norm)))


def _one_rank_worker(rank, port, out_dir, use_graph):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", MTN_FORCE_DIST="1",
                      MTN_DIST_BACKEND="nccl", MTN_EMBED_DETERMINISTIC="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    os.environ.pop("MTN_DP_SHARDED", None)
    os.environ.pop("MTN_DP_OVERLAP", None)
    import torch.distributed as dist
    from mtn_amd import dp
    from mtn_amd.train_step import TrainStep
    from oracle import fixtures as fx
    r, w, _ = dp.init_distributed()
    assert (r, w) == (0, 1) and dist.is_initialized() and dist.get_backend() == "nccl"
    dev = torch.device("cuda:0")
    c = _cfg()
    raw = fx.det_batch(c["vocab"], c["B"], c["Q"], c["H"], c["C"], c["T"], c["frames"], c["ft_sizes"], seed=3)
    dtype, drop = "bf16", 0.1
    C = _measure(c, raw, dev, dtype, drop)
    res = {"C": C}

    def variant(force, **kw):
        torch.manual_seed(0)
        model = _make(c, dev, dtype, drop)
        sync = None
        if force is not None:
            sync = dp.GradSync(lambda: model.flat_buffers()[2], n_buckets=3, force=force)
            assert sync.force == force
            sync.broadcast_(model._flat)
        step, st = _clipped_steps(model, _batch(c, raw, dev), c, sync, use_graph, C, **kw)
        return step, st

    step, res["rccl"] = variant(True)                        # every slice all-reduced through RCCL, overlapped with the backward
    assert step.overlap and step.grad_sync.force
    step, res["skipped"] = variant(False)                    # the same schedule, collectives skipped
    assert step.overlap
    step, res["simple"] = variant(True, overlap=False)       # monolithic backward, the whole-buffer all-reduce, the optimiser
    assert not step.overlap
    _, res["plain"] = variant(None)                          # no grad_sync at all: the clipped single-rank step
    # asking for the sharded optimiser with clipping raises, and says why
    os.environ["MTN_DP_SHARDED"] = "1"
    model = _make(c, dev, dtype, drop)
    sync = dp.GradSync(lambda: model.flat_buffers()[2], n_buckets=3)
    try:
        TrainStep(model, _batch(c, raw, dev), c["vocab"], pad=fx.PAD, warmup=10, grad_sync=sync, clip_grad_norm=C)
        res["sharded_error"] = None
    except ValueError as e:
        res["sharded_error"] = str(e)
    ts = TrainStep(model, _batch(c, raw, dev), c["vocab"], pad=fx.PAD, warmup=10, grad_sync=sync)      # without clipping it is what it was
    res["sharded_without_clipping"] = ts.sharded is not None
    torch.save(res, os.path.join(out_dir, "one_rank.pt"))
    dist.barrier()
    dist.destroy_process_group()


def _bits_equal(a, b):
    view = {8: torch.int64, 4: torch.int32}
    return a.shape == b.shape and torch.equal(a.contiguous().view(view[a.element_size()]), b.contiguous().view(view[b.element_size()]))


@pytest.mark.timeout(600)
@pytest.mark.parametrize("use_graph", [True, False], ids=["graphs", "eager"])
def test_one_rank_rccl_equals_the_plain_clipped_schedule_bitwise(tmp_path, use_graph):
    import torch.multiprocessing as mp
    assert torch.cuda.is_available()
    mp.start_processes(_one_rank_worker, args=(_free_port(), str(tmp_path), use_graph), nprocs=1, join=True, start_method="spawn")
    res = torch.load(tmp_path / "one_rank.pt")
    for a, b in (("rccl", "skipped"), ("simple", "plain")):
        for k in ("flat", "m", "v", "norm"):
            assert _bits_equal(res[a][k], res[b][k]), f"{k}: {a} differs from {b}"
        assert res[a]["losses"] == res[b]["losses"] and res[a]["stats"] == res[b]["stats"]
    for key in ("rccl", "simple"):
        st = res[key]["stats"]
        assert st["steps"] == STEPS and st["clipped"] >= 1 and st["nonfinite"] == 0 and st["max"] > res["C"]
    # the segmented backward computes the parameter gradients with other tilings than the monolithic one: the same norm up to fp32
    # summation order (tests/test_dp_rccl_gpu.py holds the losses of these two schedules to 3e-3 in bf16)
    a, b = float(res["rccl"]["norm"]), float(res["plain"]["norm"])
    assert abs(a - b) < 3e-3 * b, (a, b)
    assert res["sharded_error"] is not None and "clipping" in res["sharded_error"] and "sharded" in res["sharded_error"]
    assert res["sharded_without_clipping"]


def _two_rank_worker(rank, world, port, out_dir, use_graph):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank),
                      MTN_DIST_BACKEND="nccl", HSA_ENABLE_IPC_MODE_LEGACY="0")
    os.environ.pop("MTN_DP_SHARDED", None)
    import torch.distributed as dist
    from mtn_amd import dp
    from oracle import fixtures as fx
    dp.init_distributed()
    dev = torch.device("cuda", rank)
    c = _cfg()
    raw = fx.det_batch(c["vocab"], c["B"], c["Q"], c["H"], c["C"], c["T"], c["frames"], c["ft_sizes"], seed=3)
    s, e = dp.shard_range(c["B"], rank, world)
    shard = {k: (v[s:e] if k != "fts" else [f[s:e] for f in v]) for k, v in raw.items()}

    def fresh():
        model = _make(c, dev, "fp32", 0.0)
        sync = dp.GradSync(lambda: model.flat_buffers()[2], n_buckets=3)
        sync.broadcast_(model._flat)
        return model, sync

    model, sync = fresh()                                    # step 1's norm over both ranks (the same bits on both): the cap is half of it
    step, _, _ = _run_steps(model, _batch(c, shard, dev), c, sync, False, n=1, clip_grad_norm=float("inf"))
    C = float(np.float32(0.5 * float(step.last_grad_norm)))
    model, sync = fresh()
    _, st = _clipped_steps(model, _batch(c, shard, dev), c, sync, use_graph, C)
    torch.save(dict(st, C=C), os.path.join(out_dir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(600)
@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs (RCCL allows one rank per device)")
@pytest.mark.parametrize("use_graph", [True, False], ids=["graphs", "eager"])
def test_two_ranks_share_the_norm_bits_and_equal_one_rank_on_the_concatenated_batch(tmp_path, use_graph):
    import torch.multiprocessing as mp
    from oracle import fixtures as fx
    mp.start_processes(_two_rank_worker, args=(2, _free_port(), str(tmp_path), use_graph), nprocs=2, join=True, start_method="spawn")
    r0, r1 = torch.load(tmp_path / "rank0.pt"), torch.load(tmp_path / "rank1.pt")
    assert r0["C"] == r1["C"] and _bits_equal(r0["norm"], r1["norm"]) and r0["stats"] == r1["stats"]      # identical norm bits
    assert _bits_equal(r0["flat"], r1["flat"]) and _bits_equal(r0["m"], r1["m"])                         # replicas stay identical
    assert r0["stats"]["clipped"] >= 1 and r0["stats"]["steps"] == STEPS
    dev = torch.device("cuda:0")
    c = _cfg()
    raw = fx.det_batch(c["vocab"], c["B"], c["Q"], c["H"], c["C"], c["T"], c["frames"], c["ft_sizes"], seed=3)
    model = _make(c, dev, "fp32", 0.0)
    _, one = _clipped_steps(model, _batch(c, raw, dev), c, None, False, r0["C"])
    dp_losses = [a + b for a, b in zip(r0["losses"], r1["losses"])]          # every rank normalises by the GLOBAL token counts
    for a, b in zip(dp_losses, one["losses"]):
        assert abs(a - b) < 2e-3 * abs(b), (dp_losses, one["losses"])
    assert abs(float(r0["norm"]) - float(one["norm"])) < 2e-3 * float(one["norm"])
    cos = float((r0["m"].double() * one["m"].double()).sum() / (r0["m"].double().norm() * one["m"].double().norm()))
    assert cos > 0.99999, cos
    assert one["stats"]["clipped"] == r0["stats"]["clipped"]
