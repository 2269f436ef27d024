"""The exponential moving average of the weights inside the training step (FusedAdam.enable_ema, TrainStep(ema_decay=...)) on the small
configurations of tests/test_model_gpu.py, with the helpers of tests/test_distill_step_gpu.py:
  (a) the average is read-only on the training state: loss, masters and moments after 3 steps are those of the step without it, bit for bit;
  (b) the recurrence: the average equals tests/average_refs.py ema_run of the masters snapshotted after every step, bit for bit — the
      fused schedule, the separate optimiser pass, the captured step;
  (c) averaged_weights(): inside, the model computes what a fresh model built from ema_state_dict() computes; after it every buffer
      is what it was and training goes on as if nothing had happened;
  (d) the checkpoint round trip, and a file from before the average existed;
  (e) the one-rank RCCL chain and two gloo ranks with the sharded optimiser (child processes)."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import fixtures as fx
from tests import average_refs as R
from tests.step_helpers import _student, deterministic_embed  # noqa: F401  (fixture)
from tests.test_distill_step_gpu import _config, _free_port, dev  # noqa: F401  (fixture)
from tests.test_model_gpu import build_model, dev_batch, raw_batch
from tests.util import DTYPES

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["small_shared", "cfg1_query"]


def _bits(t):
    return t.detach().contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _np(t):
    return t.detach().float().cpu().numpy()


def _step(c, dtype, dev, ema_decay, dropout=0.0, **kw):
    from mtn_amd.train_step import TrainStep
    model = _student(c, dtype, dev, dropout)
    return model, TrainStep(model, dev_batch(raw_batch(c), dev), c["vocab"], pad=fx.PAD, warmup=10, ema_decay=ema_decay, **kw)


# ------------------------------------------------------------------------------------------ (a)
@pytest.mark.parametrize("use_graph", [True, False], ids=["captured", "eager"])
@pytest.mark.parametrize("name", NAMES)
def test_the_average_is_read_only_on_the_training_state(dev, name, use_graph, deterministic_embed):
    c = _config(name)

    def run(decay):
        model, ts = _step(c, torch.bfloat16, dev, decay, dropout=0.1, use_graph=use_graph)
        losses = [ts().clone() for _ in range(3)]
        torch.cuda.synchronize()
        adam = ts.opt.optimizer
        return losses, model._flat.clone(), adam.m.clone(), adam.v.clone(), adam

    off_l, off_p, off_m, off_v, off_adam = run(0.0)
    on_l, on_p, on_m, on_v, on_adam = run(0.99)
    assert off_adam.ema is None and on_adam.ema is not None and on_adam.ema_decay == 0.99
    for a, b in zip(off_l, on_l):
        assert _same(a, b), (float(a), float(b))
    assert _same(off_p, on_p) and _same(off_m, on_m) and _same(off_v, on_v)
    assert off_l[0].item() != off_l[2].item()                                     # the steps did train
    assert not torch.equal(on_adam.ema, on_p) and bool(torch.isfinite(on_adam.ema).all())


def test_enable_ema_checks_its_decay(dev):
    from mtn_amd import FusedAdam
    c = _config("small_shared")
    model = _student(c, torch.bfloat16, dev, 0.0)
    for bad in (0.0, 1.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            FusedAdam(model).enable_ema(bad)
    adam = FusedAdam(model)
    assert adam.ema is None and "ema" not in adam.state_dict()
    adam.enable_ema(0.5)
    assert _same(adam.ema, model._flat) and adam.ema.data_ptr() != model._flat.data_ptr()
    sd = adam.state_dict()
    assert sd["ema_decay"] == 0.5 and set(sd["ema"]) == set(sd["exp_avg"])


# ------------------------------------------------------------------------------------------ (b)
def _stepped(c, dtype, dev, decay, n=3, **kw):
    """(optimiser, masters before the first step, masters after each of n steps)"""
    model, ts = _step(c, dtype, dev, decay, **kw)
    start = model._flat.clone()
    snaps = []
    for _ in range(n):
        ts()
        snaps.append(model._flat.clone())
    torch.cuda.synchronize()
    return ts.opt.optimizer, start, snaps


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", NAMES)
def test_the_average_follows_the_recurrence(dev, name, dtype, deterministic_embed):
    # decay 0.25: the coefficient is the warm-up's 9/11 at t = 1, both terms (0.75) at t = 2 and 1 - decay at t = 3; 0.999: the warm-up's
    decay = 0.25 if dtype == torch.float32 else 0.999
    c = _config(name)
    emas = {}
    for key, kw in (("fused", dict(use_graph=False)), ("separate", dict(use_graph=False, fuse_optimizer=False)), ("captured", dict(use_graph=True))):
        adam, start, snaps = _stepped(c, dtype, dev, decay, **kw)
        assert float(adam.state[0]) == 3.0
        want = R.ema_run([_np(s) for s in snaps], decay, start=_np(start))
        got = adam.ema.cpu().numpy()
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), (key, int((got != want).sum()), got.size)
        assert not np.array_equal(got, _np(snaps[-1]))
        emas[key] = adam.ema.clone()
    assert _same(emas["captured"], emas["fused"])                                 # the captured step is the eager one, bit for bit


# ------------------------------------------------------------------------------------------ (c)
@pytest.mark.parametrize("dtype,use_graph", [(torch.bfloat16, True), (torch.bfloat16, False), (torch.float32, False)], ids=["bf16-captured", "bf16-eager", "fp32-eager"])
def test_averaged_weights_swaps_in_the_average_and_back(dev, dtype, use_graph, deterministic_embed):
    c = _config("cfg1_query")

    def forward_eval(model, batch):
        model.eval()
        with torch.no_grad():
            out, ae = model.forward(batch)
        model.train()
        return [out.clone()] + [a.clone() for a in (ae or []) if torch.is_tensor(a)]

    model, ts = _step(c, dtype, dev, 0.9, use_graph=use_graph)
    for _ in range(3):
        ts()
    adam = ts.opt.optimizer
    copies = lambda: [model._flat, adam.ema, model._flat_lp] + ([model._flat_lpT] if model._flat_lpT is not None else [])
    before = [t.clone() for t in copies()]
    ema_sd = adam.ema_state_dict()
    assert list(ema_sd) == list(model.state_dict())
    with adam.averaged_weights():
        assert _same(model._flat, before[1]) and _same(adam.ema, before[0])
        inside = forward_eval(model, ts.batch)
    torch.cuda.synchronize()
    for t, b in zip(copies(), before):                                           # masters, average, compute-dtype copy, transposed copies
        assert _same(t, b)
    fresh = build_model(c, dtype, dev, seed=5)
    fresh.load_state_dict(ema_sd, strict=False)
    ref = forward_eval(fresh.train(), ts.batch)
    assert len(ref) == len(inside) >= 1
    for a, b in zip(inside, ref):
        assert _same(a, b)
    raw = forward_eval(model, ts.batch)
    assert not _same(raw[0], inside[0])                                          # the average is not the raw weights
    after = ts().clone()
    # the same four steps without the detour
    model2, ts2 = _step(c, dtype, dev, 0.9, use_graph=use_graph)
    for _ in range(3):
        ts2()
    straight = ts2().clone()
    torch.cuda.synchronize()
    assert _same(after, straight), (float(after), float(straight))
    assert _same(model._flat, model2._flat) and _same(adam.ema, ts2.opt.optimizer.ema) and _same(adam.m, ts2.opt.optimizer.m)


def test_the_average_needs_enabling(dev):
    from mtn_amd import FusedAdam, lib
    adam = FusedAdam(_student(_config("small_shared"), torch.bfloat16, dev, 0.0))
    with pytest.raises(lib.MtnHipError):
        adam.ema_state_dict()
    with pytest.raises(lib.MtnHipError):
        with adam.averaged_weights():
            pass


# ------------------------------------------------------------------------------------------ (d)
def test_checkpoint_round_trip(dev, tmp_path, deterministic_embed, caplog):
    c = _config("cfg1_query")
    dtype, decay = torch.bfloat16, 0.9
    model_a, ts_a = _step(c, dtype, dev, decay, use_graph=False)
    for _ in range(4):
        ts_a()
    model_b, ts_b = _step(c, dtype, dev, decay, use_graph=False)
    for _ in range(2):
        ts_b()
    torch.save(model_b.state_dict(), tmp_path / "m.pth.tar")
    torch.save(ts_b.opt.state_dict(), tmp_path / "m_opt.pth.tar")
    saved = torch.load(tmp_path / "m_opt.pth.tar")
    assert saved["optimizer"]["ema_decay"] == decay and set(saved["optimizer"]["ema"]) == set(saved["optimizer"]["exp_avg"])

    def resumed(opt_state, ema_decay=decay):
        from mtn_amd.train_step import TrainStep
        model = build_model(c, dtype, dev, seed=3).train()                       # other weights: everything must come from the files
        model.load_state_dict(torch.load(tmp_path / "m.pth.tar", map_location=dev), strict=False)
        model.prepare()
        ts = TrainStep(model, dev_batch(raw_batch(c), dev), c["vocab"], pad=fx.PAD, warmup=10, ema_decay=ema_decay, use_graph=False)
        ts.opt.load_state_dict(opt_state)
        return model, ts

    model_c, ts_c = resumed(saved)
    assert _same(ts_c.opt.optimizer.ema, ts_b.opt.optimizer.ema)
    for _ in range(2):
        ts_c()
    torch.cuda.synchronize()
    a, r = ts_a.opt.optimizer, ts_c.opt.optimizer
    assert _same(model_c._flat, model_a._flat) and _same(r.m, a.m) and _same(r.v, a.v) and _same(r.state, a.state)
    assert _same(r.ema, a.ema)
    # a file without "ema" (from before the average existed): the average starts from the loaded masters, and a log line says so
    old = {"step": saved["step"], "optimizer": {k: v for k, v in saved["optimizer"].items() if k not in ("ema", "ema_decay")}}
    import logging
    with caplog.at_level(logging.INFO, logger="mtn_amd"):
        model_d, ts_d = resumed(old)
    assert _same(ts_d.opt.optimizer.ema, model_d._flat) and _same(model_d._flat, model_b._flat)
    assert any("average" in r.getMessage() for r in caplog.records)
    # a file WITH an average loads into an optimiser that keeps none, as any other file
    model_e, ts_e = resumed(saved, ema_decay=0.0)
    assert ts_e.opt.optimizer.ema is None and _same(ts_e.opt.optimizer.m, ts_b.opt.optimizer.m)


# ------------------------------------------------------------------------------------------ (e)
def _rccl_worker(rank, port, out_dir):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", MTN_FORCE_DIST="1",
                      MTN_DIST_BACKEND="nccl", MTN_EMBED_DETERMINISTIC="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    os.environ.pop("MTN_DP_SHARDED", None)
    os.environ.pop("MTN_DP_OVERLAP", None)
    import torch.distributed as dist
    from mtn_amd import dp
    from mtn_amd.train_step import TrainStep
    r, w, _ = dp.init_distributed()
    assert (r, w) == (0, 1) and dist.is_initialized() and dist.get_backend() == "nccl"
    dev = torch.device("cuda:0")
    c = _config("cfg1_query")
    b = dev_batch(raw_batch(c), dev)
    res = {}
    for key, collective in (("rccl", True), ("plain", False)):
        model = _student(c, torch.bfloat16, dev, 0.0)
        sync = dp.GradSync(lambda: model.flat_buffers()[2], n_buckets=3)
        sync.broadcast_(model._flat)
        ts = TrainStep(model, b, c["vocab"], pad=fx.PAD, warmup=10, grad_sync=sync, use_graph=False, ema_decay=0.9)
        sh = ts.sharded
        assert sh is not None and sh.native and sh.collective and ts.overlap
        sh.collective = collective
        start = model._flat.clone()
        snaps = []
        for _ in range(3):
            ts()
            snaps.append(model._flat.clone())
        torch.cuda.synchronize()
        res[key] = dict(ema=ts.opt.optimizer.ema.cpu(), flat=model._flat.detach().cpu().clone(), calls=dict(sh.calls), n_slices=len(ts._slices()),
                        want=torch.from_numpy(R.ema_run([_np(s) for s in snaps], 0.9, start=_np(start))))
    torch.save(res, os.path.join(out_dir, "rccl.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_one_rank_rccl_chain_keeps_the_plain_schedules_average(tmp_path):
    import torch.multiprocessing as mp
    assert torch.cuda.is_available()
    mp.start_processes(_rccl_worker, args=(_free_port(), str(tmp_path)), nprocs=1, join=True, start_method="spawn")
    res = torch.load(tmp_path / "rccl.pt")
    rccl, plain = res["rccl"], res["plain"]
    assert rccl["calls"]["reduce_scatter"] == 3 * rccl["n_slices"] and plain["calls"]["reduce_scatter"] == 0     # the chain did go through RCCL
    assert _same(rccl["flat"], plain["flat"])
    assert _same(rccl["ema"], plain["ema"])
    assert _same(rccl["ema"], rccl["want"]) and not _same(rccl["ema"], rccl["flat"])           # one launch per slice covers every element


def _gloo_worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0",
                      MTN_DP_SHARDED="1", MTN_EMBED_DETERMINISTIC="1")
    import torch.distributed as dist
    from mtn_amd import dp
    from mtn_amd.train_step import TrainStep
    dev = torch.device("cuda:0")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    c = dict(_config("cfg1_query"), B=4)
    raw = raw_batch(c, seed=3)
    s, e = dp.shard_range(c["B"], rank, world)
    shard = {k: (v[s:e] if k != "fts" else [f[s:e] for f in v]) for k, v in raw.items()}
    model = _student(c, torch.bfloat16, dev, 0.0)
    sync = dp.GradSync(lambda: model.flat_buffers()[2], n_buckets=3)
    ts = TrainStep(model, dev_batch(shard, dev), c["vocab"], pad=fx.PAD, warmup=10, grad_sync=sync, use_graph=False, ema_decay=0.9)
    sh = ts.sharded
    assert sh is not None and sh.world == 2 and sh.lp_mode()
    params = {n for n, _ in model.named_parameters()}
    snap = lambda: {k: v.detach().cpu().clone() for k, v in model.state_dict().items() if k in params}      # (collective: gathers the masters)
    start = snap()
    snaps = []
    for _ in range(3):
        ts()
        assert sh.masters_stale                                                 # this rank's copies of the other rank's masters are behind
        snaps.append(snap())
    ema = ts.opt.optimizer.ema_state_dict()                                     # (collective)
    ema = {k: v.cpu() for k, v in ema.items() if k in params}
    torch.cuda.synchronize()
    if rank == 0:
        torch.save(dict(start=start, snaps=snaps, ema=ema, slices=sorted(sh.slices), glue=model._glue_numel), os.path.join(out_dir, "gloo.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_gloo_ranks_gather_the_sharded_average(tmp_path):
    """Two ranks on one GPU with the sharded optimiser and the compute-dtype gather: each rank updates the average of its own shards (and of
    the replicated tails) only; gathered, every element — matrices, vectors, the glue slice — follows the recurrence on the gathered masters."""
    import torch.multiprocessing as mp
    assert torch.cuda.is_available()
    mp.start_processes(_gloo_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True, start_method="spawn")
    r = torch.load(tmp_path / "gloo.pt")
    assert len(r["slices"]) >= 2 and r["glue"] > 0
    dims, moved = set(), 0
    for k, got in r["ema"].items():
        want = R.ema_run([_np(s[k]) for s in r["snaps"]], 0.9, start=_np(r["start"][k]))
        assert np.array_equal(got.numpy().view(np.int32), want.view(np.int32)), k
        moved += int(not torch.equal(got, r["snaps"][-1][k]))
        dims.add(got.dim())
    assert {1, 2} <= dims and len(r["ema"]) > 20 and moved > len(r["ema"]) // 2      # the average is not the masters
