"""Scheduled sampling inside the training step (mtn_amd.train_step.TrainStep(sched=...)) on the smallest golden configuration (2 layers,
d_model 64) at B = 4, with the helpers of tests/test_distill_step_gpu.py:
  (a) with ``start`` beyond the steps run (p = 0 while the first pass still runs) the weights after two captured steps are the plain
      TrainStep's bit for bit, at dropout 0.1: the first pass leaves nothing behind;
  (b) with p = 1, argmax and dropout 0, ``sched_mixed`` is the shifted host arg-max of the model's own eval() logits, and loss and
      gradient buffer equal, bit for bit, a plain TrainStep on a batch whose ``trg`` was replaced by hand;
  (c) graphed and eager steps give the same bytes (losses, weights, mixed tokens, counters);
  (d) two replays differ in their draws once the step has advanced, and each is the definition's at its step;
  (e) with sched=None nothing is allocated and the launch census is the step's without the keyword; with it, the census is the first
      pass followed by exactly the plain step's launches;
  (f) the layer-segmented schedule on a one-rank group gives the monolithic step's mixed tokens and its first loss within 1e-5 relative."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import fixtures as fx
from tests import sched_refs as R
from tests.step_helpers import _census, _student, deterministic_embed  # noqa: F401  (fixture)
from tests.test_distill_step_gpu import _config, _free_port, dev  # noqa: F401  (fixture)
from tests.test_model_gpu import dev_batch, raw_batch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cfg():
    return dict(_config("small_shared"), B=4)


def _bits(t):
    return t.detach().contiguous().view({8: torch.int64, 4: torch.int32, 2: torch.int16}[t.element_size()])


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _step(c, dev, raw, dropout, sched, **kw):
    from mtn_amd.train_step import TrainStep
    model = _student(c, torch.bfloat16, dev, dropout)
    return model, TrainStep(model, dev_batch(raw, dev), c["vocab"], pad=fx.PAD, warmup=10, sched=sched, **kw)


def _eval_logits(model, batch):
    """The model's own eval() generator logits for the gold batch, (B * T, V) float32 numpy; the model is left in train()."""
    model.eval()
    with torch.no_grad():
        o, _ = model.forward(batch)
        z = model.generator.logits(o)
    model.train()
    torch.cuda.synchronize()
    return z.reshape(-1, z.size(-1)).float().cpu().numpy()


# ------------------------------------------------------------------------------------------ (a)
def test_the_first_pass_leaves_nothing_behind(dev, deterministic_embed):
    from mtn_amd.train_step import SchedConfig
    c = _cfg()
    raw = raw_batch(c)
    model_p, plain = _step(c, dev, raw, 0.1, None)
    model_s, sched = _step(c, dev, raw, 0.1, SchedConfig(0.5, start=100, pick="sample"))
    for _ in range(2):
        lp, ls = plain().clone(), sched().clone()
        assert _same(lp, ls)
    torch.cuda.synchronize()
    assert _same(model_p._flat, model_s._flat)
    assert _same(plain.opt.optimizer.m, sched.opt.optimizer.m) and _same(plain.opt.optimizer.v, sched.opt.optimizer.v)
    assert sched.opt.step_count() == 2
    trg = sched.batch.trg
    assert torch.equal(sched.sched_mixed, trg) and sched.sched_mixed.data_ptr() != trg.data_ptr()
    eligible = int((trg[:, 1:] != fx.PAD).sum())
    assert sched.sched_stats.tolist() == [2 * eligible, 0, 0]              # the two steps, not the capture's warm-up passes


# ------------------------------------------------------------------------------------------ (b)
def test_p_one_argmax_is_the_plain_step_on_a_batch_replaced_by_hand(dev, deterministic_embed):
    from mtn_amd.train_step import SchedConfig
    c = _cfg()
    raw = raw_batch(c)
    model, ts = _step(c, dev, raw, 0.0, SchedConfig(1.0, pick="argmax", banned=(fx.SOS,)), use_graph=False, fuse_optimizer=False)
    z = _eval_logits(model, ts.batch)
    loss = ts._fwd_bwd().clone()
    torch.cuda.synchronize()
    mixed = ts.sched_mixed.cpu().numpy()
    trg = raw["trg"]
    B, T = trg.shape
    z[:, [fx.PAD, fx.SOS]] = -np.inf
    am = z.argmax(axis=1).reshape(B, T)                                    # (numpy: the first of equal values)
    want = trg.copy()
    for t in range(1, T):
        want[:, t] = np.where(trg[:, t] != fx.PAD, am[:, t - 1], trg[:, t])
    assert np.array_equal(mixed, want)
    assert (mixed != trg).any() and np.array_equal(ts.batch.trg.cpu().numpy(), trg)          # it did replace; the gold ids survive
    eligible = int((trg[:, 1:] != fx.PAD).sum())
    assert ts.sched_stats.tolist() == [eligible, eligible, int((mixed != trg).sum())]
    # the reference also agrees with the numpy definition over the same logits
    ref = R.mix(_eval_logits(model, ts.batch), trg, ts.sched_keys.cpu().numpy(), 0, pad=fx.PAD, banned=(fx.SOS,), p_max=1.0)
    assert np.array_equal(ref["mixed"], mixed)
    model_b, plain = _step(c, dev, dict(raw, trg=mixed), 0.0, None, use_graph=False, fuse_optimizer=False)
    loss_b = plain._fwd_bwd().clone()
    torch.cuda.synchronize()
    assert _same(loss, loss_b), (float(loss), float(loss_b))
    assert _same(model._flat_grad, model_b._flat_grad) and bool(model._flat_grad.any())
    # ... and it is another step than the one on the gold inputs
    model_g, gold = _step(c, dev, raw, 0.0, None, use_graph=False, fuse_optimizer=False)
    assert float(gold._fwd_bwd()) != float(loss)


# ------------------------------------------------------------------------------------------ (c) (d)
@pytest.mark.parametrize("pick", ["argmax", "sample"])
def test_graphed_equals_eager_and_every_step_draws_anew(dev, deterministic_embed, pick):
    from mtn_amd.train_step import SchedConfig
    c = _cfg()
    raw = raw_batch(c)
    runs = []
    for use_graph in (True, False):
        model, ts = _step(c, dev, raw, 0.0, SchedConfig(0.5, pick=pick, temperature=0.8, seed=5, banned=(fx.SOS,)), use_graph=use_graph)
        steps = []
        for k in range(3):
            z = _eval_logits(model, ts.batch)                             # what this step's first pass will see
            loss = ts().clone()
            torch.cuda.synchronize()
            steps.append((loss, ts.sched_mixed.clone(), z))
        runs.append(dict(steps=steps, flat=model._flat.clone(), stats=ts.sched_stats.tolist(), keys=ts.sched_keys.cpu().numpy()))
    g, e = runs
    for (lg, mg, _), (le, me, _) in zip(g["steps"], e["steps"]):
        assert _same(lg, le) and torch.equal(mg, me)
    assert _same(g["flat"], e["flat"]) and g["stats"] == e["stats"] and g["stats"][0] == 3 * int((raw["trg"][:, 1:] != fx.PAD).sum())
    assert 0 < g["stats"][1] < g["stats"][0] and g["stats"][2] <= g["stats"][1]
    # (d) the coins of step k are the definition's at state[0] = k: other positions are replaced from one replay to the next
    trg = raw["trg"]
    masks = []
    for k, (_, mixed, z) in enumerate(g["steps"]):
        ref = R.mix(z, trg, g["keys"], k, pad=fx.PAD, banned=(fx.SOS,), p_max=0.5, seed=5, pick=R.ARGMAX)
        masks.append(ref["coin"])
        m = mixed.cpu().numpy()
        assert np.array_equal(m[~ref["coin"]], trg[~ref["coin"]])
        assert not np.isin(m[ref["coin"]], (fx.PAD, fx.SOS)).any()
        if pick == "argmax":
            assert np.array_equal(m, ref["mixed"])
    assert not np.array_equal(masks[0], masks[1]) and not np.array_equal(masks[1], masks[2])
    assert list(g["keys"]) == list(range(trg.shape[0]))                    # the fixed batch: rank * B + b


# ------------------------------------------------------------------------------------------ (e)
def test_off_is_the_step_without_the_keyword_and_on_adds_the_first_pass_only(dev, deterministic_embed):
    from mtn_amd.train_step import SchedConfig, TrainStep
    c = _cfg()
    raw = raw_batch(c)
    b = dev_batch(raw, dev)

    def census(**kw):
        model = _student(c, torch.bfloat16, dev, 0.1)
        ts = TrainStep(model, b, c["vocab"], pad=fx.PAD, warmup=10, use_graph=False, **kw)
        ts()                                                              # (lazy set-up outside the census)
        return _census(ts), model, ts

    (without_c, without_f), _, _ = census()
    (off_c, off_f), _, off = census(sched=None)
    assert off_c == without_c and off_f == without_f
    assert off.sched_mixed is None and off.sched_keys is None and off.sched_stats is None and off._fwd_batch is off.batch
    (on_c, on_f), model, on = census(sched=SchedConfig(0.25))

    def first_pass():
        model.eval()
        with torch.no_grad():
            o, _ = model.forward(b)
            model.generator.logits(o)
        model.train()
    pass_c, pass_f = _census(first_pass)
    assert len(pass_c) > 0 and on_c == pass_c + without_c
    assert on_f == tuple(x + y for x, y in zip(pass_f, without_f))
    assert on._fwd_batch is not on.batch and on._fwd_batch.trg is on.sched_mixed and on._fwd_batch.trg_y is on.batch.trg_y \
        and on._fwd_batch.trg_mask is on.batch.trg_mask


def test_argument_checks(dev):
    from mtn_amd.train_step import SchedConfig, ScstConfig, TrainStep
    c = _cfg()
    b = dev_batch(raw_batch(c), dev)
    model = _student(c, torch.bfloat16, dev, 0.0)
    with pytest.raises(ValueError, match="sched"):
        TrainStep(model, b, c["vocab"], pad=fx.PAD, sched=SchedConfig(0.5), teacher=_student(c, torch.bfloat16, dev, 0.0).eval())
    with pytest.raises(ValueError, match="sched"):
        TrainStep(model, b, c["vocab"], pad=fx.PAD, sched=SchedConfig(0.5), scst=ScstConfig())


# ------------------------------------------------------------------------------------------ (f)
def _segmented_worker(rank, port, out_dir):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", MTN_EMBED_DETERMINISTIC="1")
    import torch.distributed as dist
    from mtn_amd import dp
    from mtn_amd.train_step import SchedConfig, TrainStep
    dev = torch.device("cuda:0")
    dist.init_process_group("gloo", rank=0, world_size=1)
    c = _cfg()
    b = dev_batch(raw_batch(c), dev)
    out = {}
    for key in ("segmented", "monolithic"):
        model = _student(c, torch.bfloat16, dev, 0.0)
        sync = dp.GradSync(lambda: model.flat_buffers()[2]) if key == "segmented" else None
        ts = TrainStep(model, b, c["vocab"], pad=fx.PAD, warmup=10, grad_sync=sync, use_graph=True, overlap=True if sync is not None else None,
                       sched=SchedConfig(0.5, pick="sample", seed=3))
        losses, mixed = [], []
        for _ in range(2):
            losses.append(float(ts()))
            mixed.append(ts.sched_mixed.cpu().clone())
        out[key] = dict(losses=losses, mixed=mixed, stats=ts.sched_stats.tolist(), overlap=bool(ts.overlap), keys=ts.sched_keys.tolist())
    torch.cuda.synchronize()
    torch.save(out, os.path.join(out_dir, "sched.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_segmented_schedule_matches_the_monolithic_step(tmp_path):
    import torch.multiprocessing as mp
    assert torch.cuda.is_available()
    mp.start_processes(_segmented_worker, args=(_free_port(), str(tmp_path)), nprocs=1, join=True, start_method="spawn")
    r = torch.load(tmp_path / "sched.pt")
    s, m = r["segmented"], r["monolithic"]
    assert s["overlap"] and not m["overlap"]
    print("segmented", s["losses"], s["stats"], "monolithic", m["losses"], m["stats"])
    assert torch.equal(s["mixed"][0], m["mixed"][0])                       # the same weights, the same first pass, the same draws
    assert abs(s["losses"][0] - m["losses"][0]) <= 1e-5 * abs(m["losses"][0])
    assert s["keys"] == m["keys"] == list(range(4))                        # rank 0: rank * B + b
    assert s["stats"][0] == m["stats"][0] and 0 < s["stats"][1] < s["stats"][0]
    assert not torch.equal(s["mixed"][0], s["mixed"][1])                   # the second step drew anew
