"""R-Drop under data parallelism, with spawned workers and the helpers of tests/test_dp_rccl_gpu.py: the paired loss head is local to the
rank and the normalisers (both passes' tokens) are all-reduced as ever, so nothing new is exchanged.
  * one rank, backend "nccl" (MTN_FORCE_DIST=1), every slice really going through RCCL with rdrop on: weights, moments, losses and last_rd
    equal, BIT FOR BIT, the same schedule with the collectives skipped; the two-graph schedule and the fused
    single-rank step (no grad_sync at all) reproduce its losses at that file's tolerance, and the divergence is really there;
  * two ranks, one GPU each — skipped unless the box has two GPUs, as in that file: on a pre-paired batch (each rank holds its dialogues'
    two passes) N ranks x half batch == one rank x whole batch at that file's tolerance."""
import os
import sys

import numpy as np
import pytest
import torch

from tests.test_dp_rccl_gpu import _batch, _cfg, _free_port, _make, _run_steps

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = 2
ALPHA = 1.0


def _rd_steps(model, batch, c, sync, use_graph, **kw):
    step, losses, st = _run_steps(model, batch, c, sync, use_graph, n=STEPS, rdrop=ALPHA, **kw)
    return step, dict(st, losses=losses, rd=float(step.last_rd))


def _one_rank_worker(rank, port, out_dir, use_graph):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", MTN_FORCE_DIST="1",
                      MTN_DIST_BACKEND="nccl", MTN_EMBED_DETERMINISTIC="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    os.environ.pop("MTN_DP_SHARDED", None)
    os.environ.pop("MTN_DP_OVERLAP", None)
    import torch.distributed as dist
    from mtn_amd import dp
    from oracle import fixtures as fx
    r, w, _ = dp.init_distributed()
    assert (r, w) == (0, 1) and dist.is_initialized() and dist.get_backend() == "nccl"
    dev = torch.device("cuda:0")
    c = _cfg()
    raw = fx.det_batch(c["vocab"], c["B"], c["Q"], c["H"], c["C"], c["T"], c["frames"], c["ft_sizes"], seed=3)
    dtype, drop = "bf16", 0.1
    res = {}

    def variant(with_sync, **kw):
        torch.manual_seed(0)
        model = _make(c, dev, dtype, drop)
        sync = None
        if with_sync:
            sync = dp.GradSync(lambda: model.flat_buffers()[2], n_buckets=3)
            assert sync.force
            sync.broadcast_(model._flat)
        step, st = _rd_steps(model, _batch(c, raw, dev), c, sync, use_graph, **kw)
        assert step.batch.trg_y.size(0) == 2 * c["B"]
        return step, st

    step, res["rccl"] = variant(True)                        # the sharded chain, every slice through RCCL
    assert step.sharded is not None and step.sharded.native and step.sharded.collective and step.overlap
    _, res["skipped"] = variant(True, collective=False)      # the same schedule, collectives skipped
    step, res["simple"] = variant(True, overlap=False)       # monolithic backward, the whole-buffer exchange
    assert not step.overlap
    _, res["fused"] = variant(False)                         # no grad_sync at all: the one-rank step
    torch.save(res, os.path.join(out_dir, "one_rank.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(600)
@pytest.mark.parametrize("use_graph", [True, False], ids=["graphs", "eager"])
def test_one_rank_rccl_chain_with_rdrop_reproduces_the_one_rank_step(tmp_path, use_graph):
    import torch.multiprocessing as mp
    assert torch.cuda.is_available()
    mp.start_processes(_one_rank_worker, args=(_free_port(), str(tmp_path), use_graph), nprocs=1, join=True, start_method="spawn")
    res = torch.load(tmp_path / "one_rank.pt")
    rccl = res["rccl"]
    for k in ("flat", "m", "v"):
        assert torch.equal(rccl[k], res["skipped"][k]), f"{k}: the RCCL chain differs from the collective-free schedule"
    assert rccl["losses"] == res["skipped"]["losses"] and rccl["rd"] == res["skipped"]["rd"]
    # the two-graph schedule and the fused single-rank step compute the parameter gradients with other tilings: the same step up to
    # fp32 summation order (tests/test_dp_rccl_gpu.py holds these schedules' bf16 losses to 3e-3)
    for other in ("simple", "fused"):
        for a, b in zip(rccl["losses"], res[other]["losses"]):
            assert abs(a - b) < 3e-3 * abs(b), (rccl["losses"], res[other]["losses"])
        assert abs(rccl["rd"] - res[other]["rd"]) < 3e-3 * max(1.0, res[other]["rd"])
    assert rccl["rd"] > 0 and np.isfinite(rccl["rd"])       # dropout 0.1: the two passes do differ


def _paired_raw(c, fx):
    """2 B dialogues in pair layout: the second half shares the first half's questions, captions and targets, with the histories and
    features of another batch."""
    a = fx.det_batch(c["vocab"], c["B"], c["Q"], c["H"], c["C"], c["T"], c["frames"], c["ft_sizes"], seed=3)
    b = fx.det_batch(c["vocab"], c["B"], c["Q"], c["H"], c["C"], c["T"], c["frames"], c["ft_sizes"], seed=4)
    out = {k: ([np.concatenate([f, g]) for f, g in zip(v, b["fts"])] if k == "fts" else np.concatenate([v, v])) for k, v in a.items()}
    out["his"][c["B"]:] = b["his"]
    return out


def _pair_shard(raw, N, s, e):
    """rows s..e-1 of both halves: a rank's dialogues with their second passes, in pair layout"""
    rows = np.r_[s:e, N + s:N + e]
    return {k: ([f[rows] for f in v] if k == "fts" else v[rows]) for k, v in raw.items()}


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
    raw = _paired_raw(c, fx)
    s, e = dp.shard_range(c["B"], rank, world)
    model = _make(c, dev, "fp32", 0.0)
    sync = dp.GradSync(lambda: model.flat_buffers()[2], n_buckets=3)
    sync.broadcast_(model._flat)
    step, st = _rd_steps(model, _batch(c, _pair_shard(raw, c["B"], s, e), dev), c, sync, use_graph, rdrop_paired=True)
    opt_state = step.opt.optimizer.state_dict()               # every rank: gathers the sharded moments (collective)
    torch.save(dict(st, exp_avg=opt_state["exp_avg"]), os.path.join(out_dir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(600)
@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs (RCCL allows one rank per device)")
@pytest.mark.parametrize("use_graph", [True, False], ids=["graphs", "eager"])
def test_two_ranks_equal_one_rank_on_the_whole_paired_batch(tmp_path, use_graph):
    import torch.multiprocessing as mp
    from oracle import fixtures as fx
    mp.start_processes(_two_rank_worker, args=(2, _free_port(), str(tmp_path), use_graph), nprocs=2, join=True, start_method="spawn")
    r0, r1 = torch.load(tmp_path / "rank0.pt"), torch.load(tmp_path / "rank1.pt")
    assert torch.equal(r0["flat"], r1["flat"])                                          # replicas stay identical
    dev = torch.device("cuda:0")
    c = _cfg()
    model = _make(c, dev, "fp32", 0.0)
    step, one = _rd_steps(model, _batch(c, _paired_raw(c, fx), dev), c, None, False, rdrop_paired=True)
    dp_losses = [a + b for a, b in zip(r0["losses"], r1["losses"])]                     # every rank normalises by the GLOBAL token counts
    for a, b in zip(dp_losses, one["losses"]):
        assert abs(a - b) < 2e-3 * abs(b), (dp_losses, one["losses"])
    assert one["rd"] > 1e-3                                                             # the perturbed halves do diverge
    assert abs(r0["rd"] + r1["rd"] - one["rd"]) < 2e-3 * one["rd"]                      # last_rd: the rank's rows over the global count
    for k in r0["exp_avg"]:
        assert torch.equal(r0["exp_avg"][k], r1["exp_avg"][k]), k                       # gathered moments complete on both ranks
    want = step.opt.optimizer.state_dict()["exp_avg"]
    ma = torch.cat([r0["exp_avg"][k].double().flatten().cpu() for k in sorted(want)])
    mb = torch.cat([want[k].double().flatten().cpu() for k in sorted(want)])
    cos = float((ma * mb).sum() / (ma.norm() * mb.norm()))
    assert cos > 0.99999, cos
