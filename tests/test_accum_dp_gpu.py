"""Gradient accumulation under data parallelism, with spawned workers and the helpers of tests/test_dp_rccl_gpu.py, as
tests/test_clip_dp_gpu.py uses them: with accumulation on the step takes the whole-buffer, non-overlapped all-reduce, once per window,
after the launch that closes it.
  * one rank, backend "nccl" (MTN_FORCE_DIST=1), the window's gradient really all-reduced through RCCL: a K = 2 window with grad_sync
    gives the weights, moments and losses of the same window without it, BIT FOR BIT, captured and eager; grad_sync ran exactly once per
    window; asking for the sharded optimiser together with accumulation raises, naming it;
  * two ranks, one GPU each — skipped unless the box has two GPUs, as in that file: the replicas stay identical, the exchange ran once
    per window, and N ranks x half batch == one rank x whole batch at that file's tolerance."""
import os
import sys

import pytest
import torch

from tests.test_dp_rccl_gpu import _batch, _cfg, _free_port, _make

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WINDOWS = 2


def _shorter(raw, keep=3):
    """The same rows with every answer but the first cut to ``keep`` target positions: another target-token count."""
    from oracle import fixtures as fx
    out = dict(raw, trg=raw["trg"].copy(), trg_y=raw["trg_y"].copy())
    out["trg"][1:, keep:] = fx.PAD
    out["trg_y"][1:, keep:] = fx.PAD
    return out


def _counting(dp, model, **kw):
    class Counting(dp.GradSync):
        calls = 0

        def __call__(self):
            self.calls += 1
            return super().__call__()
    return Counting(lambda: model.flat_buffers()[2], n_buckets=3, **kw)


def _run_windows(model, c, raws, dev, sync, use_graph, **kw):
    """WINDOWS windows of K = 2 over the two batches, one TrainStep each over one optimiser; every variant starts its counted
    micro-steps from the same dropout seed (capture's warm-up passes advance it)."""
    from mtn_amd.train_step import TrainStep
    from oracle import fixtures as fx
    first = TrainStep(model, _batch(c, raws[0], dev), c["vocab"], pad=fx.PAD, warmup=10, grad_sync=sync, use_graph=use_graph, accumulate=True, **kw)
    second = TrainStep(model, _batch(c, raws[1], dev), c["vocab"], pad=fx.PAD, warmup=10, grad_sync=sync, use_graph=use_graph, opt=first.opt, **kw)
    assert first.accumulating and second.accumulating and first.sharded is None and not first.overlap and not second.overlap
    if use_graph:
        first._capture()
        second._capture()
    torch.cuda.synchronize()
    model._seed.fill_(4242)
    losses = []
    for _ in range(WINDOWS):
        losses.append(float(first(False)))
        losses.append(float(second(True)))
    torch.cuda.synchronize()
    adam = first.opt.optimizer
    return dict(flat=model._flat.detach().cpu().clone(), m=adam.m.cpu().clone(), v=adam.v.cpu().clone(), losses=losses,
                steps=first.opt.step_count(), calls=getattr(sync, "calls", None), w=[float(first._norms[0]), float(second._norms[0])])


def _one_rank_worker(rank, port, out_dir):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", MTN_FORCE_DIST="1",
                      MTN_DIST_BACKEND="nccl", MTN_EMBED_DETERMINISTIC="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    os.environ.pop("MTN_DP_SHARDED", None)
    os.environ.pop("MTN_DP_OVERLAP", None)
    import torch.distributed as dist
    from mtn_amd import dp
    from mtn_amd.train_step import BucketedTrainer, TrainStep
    from oracle import fixtures as fx
    r, w, _ = dp.init_distributed()
    assert (r, w) == (0, 1) and dist.is_initialized() and dist.get_backend() == "nccl"
    dev = torch.device("cuda:0")
    c = _cfg()
    raw = fx.det_batch(c["vocab"], c["B"], c["Q"], c["H"], c["C"], c["T"], c["frames"], c["ft_sizes"], seed=3)
    raws = [raw, _shorter(raw)]
    res = {}
    for use_graph in (True, False):
        for key, force in (("rccl", True), ("plain", None)):
            torch.manual_seed(0)
            model = _make(c, dev, "bf16", 0.1)
            sync = None
            if force is not None:
                sync = _counting(dp, model, force=force)
                assert sync.force
                sync.broadcast_(model._flat)
            res[(key, use_graph)] = _run_windows(model, c, raws, dev, sync, use_graph)
    # asking for the sharded optimiser with accumulation raises, and says why
    os.environ["MTN_DP_SHARDED"] = "1"
    model = _make(c, dev, "bf16", 0.1)
    sync = dp.GradSync(lambda: model.flat_buffers()[2], n_buckets=3)
    for name, build in (("step", lambda: TrainStep(model, _batch(c, raw, dev), c["vocab"], pad=fx.PAD, warmup=10, grad_sync=sync, accumulate=True)),
                        ("trainer", lambda: BucketedTrainer(model, None, c["vocab"], pad=fx.PAD, grad_sync=sync, accum_steps=2))):
        try:
            build()
            res["sharded_error_" + name] = None
        except ValueError as e:
            res["sharded_error_" + name] = str(e)
    model = _make(c, dev, "bf16", 0.1)
    sync = dp.GradSync(lambda: model.flat_buffers()[2], n_buckets=3)
    ts = TrainStep(model, _batch(c, raw, dev), c["vocab"], pad=fx.PAD, warmup=10, grad_sync=sync)      # without accumulation it is what it was
    res["sharded_without_accumulation"] = ts.sharded is not None
    torch.save(res, os.path.join(out_dir, "one_rank.pt"))
    dist.barrier()
    dist.destroy_process_group()


def _bits_equal(a, b):
    view = {8: torch.int64, 4: torch.int32}
    return a.shape == b.shape and torch.equal(a.contiguous().view(view[a.element_size()]), b.contiguous().view(view[b.element_size()]))


@pytest.mark.timeout(600)
def test_one_rank_rccl_window_equals_the_window_without_an_exchange_bitwise(tmp_path):
    import torch.multiprocessing as mp
    assert torch.cuda.is_available()
    mp.start_processes(_one_rank_worker, args=(_free_port(), str(tmp_path)), nprocs=1, join=True, start_method="spawn")
    res = torch.load(tmp_path / "one_rank.pt")
    for use_graph in (True, False):
        a, b = res[("rccl", use_graph)], res[("plain", use_graph)]
        for k in ("flat", "m", "v"):
            assert _bits_equal(a[k], b[k]), f"{k}: the exchanged window differs from the plain one (use_graph={use_graph})"
        assert a["losses"] == b["losses"] and a["steps"] == b["steps"] == WINDOWS
        assert a["calls"] == WINDOWS and b["calls"] is None                   # once per window, never on the other micro-steps
        assert a["w"][0] != a["w"][1]
    for name in ("step", "trainer"):
        err = res["sharded_error_" + name]
        assert err is not None and "accumulation" in err and "sharded" in err and "MTN_DP_SHARDED" in err
    assert res["sharded_without_accumulation"]


def _two_rank_worker(rank, world, port, out_dir):
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
    shards = [{k: (v[s:e] if k != "fts" else [f[s:e] for f in v]) for k, v in r.items()} for r in (raw, _shorter(raw))]
    model = _make(c, dev, "fp32", 0.0)
    sync = _counting(dp, model)
    sync.broadcast_(model._flat)
    st = _run_windows(model, c, shards, dev, sync, False)
    torch.save(st, os.path.join(out_dir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(600)
@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs (RCCL allows one rank per device)")
def test_two_ranks_exchange_once_per_window_and_equal_one_rank_on_the_concatenated_batches(tmp_path):
    import torch.multiprocessing as mp
    from oracle import fixtures as fx
    mp.start_processes(_two_rank_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True, start_method="spawn")
    r0, r1 = torch.load(tmp_path / "rank0.pt"), torch.load(tmp_path / "rank1.pt")
    assert _bits_equal(r0["flat"], r1["flat"]) and _bits_equal(r0["m"], r1["m"])                         # replicas stay identical
    assert r0["calls"] == r1["calls"] == WINDOWS and r0["steps"] == r1["steps"] == WINDOWS and r0["w"] == r1["w"]
    dev = torch.device("cuda:0")
    c = _cfg()
    raw = fx.det_batch(c["vocab"], c["B"], c["Q"], c["H"], c["C"], c["T"], c["frames"], c["ft_sizes"], seed=3)
    model = _make(c, dev, "fp32", 0.0)
    one = _run_windows(model, c, [raw, _shorter(raw)], dev, None, False)
    assert one["w"] == r0["w"]                                               # every rank weights by the GLOBAL token counts
    dp_losses = [a + b for a, b in zip(r0["losses"], r1["losses"])]
    for a, b in zip(dp_losses, one["losses"]):
        assert abs(a - b) < 2e-3 * abs(b), (dp_losses, one["losses"])
    cos = float((r0["m"].double() * one["m"].double()).sum() / (r0["m"].double().norm() * one["m"].double().norm()))
    assert cos > 0.99999, cos
