"""Gradient clipping by global norm inside the training step (FusedAdam.enable_clip, TrainStep(clip_grad_norm=...)) on the small
configurations of tests/test_model_gpu.py, with the helpers of tests/test_distill_step_gpu.py and dropout as the other step tests set it
(0.1 where one schedule is compared with itself; 0 where a captured step is compared with an eager one — capture's warm-up passes advance
the dropout stream):
  (1) clip_grad_norm=inf measures and changes nothing: weights and moments after three steps are those of fuse_optimizer=False, bit for
      bit; last_grad_norm is within 1e-12 of the float64 norm of the gradient read back, and that norm is the norm over the parameters'
      own .grad views — the padding between parameters stays zero on the separate-optimiser path;
  (2) C = half of step 1's norm: step 1 clips, its scale is within one ulp of tests/clip_refs.py, and the weights are, bit for bit,
      those of a fuse_optimizer=False step whose grad_scale holds those same scale bits;
  (3) captured equals eager bit for bit over three steps, at that C and at twice the largest norm (where nothing is clipped);
  (4) ema_decay together with clipping: the average follows the clipped masters;
  (5) scst together with clipping through load_rows: captured equals eager;
  and what refuses: a bad max_norm, the fused epilogue, the sharded update, clip_stats() without clipping."""
import math

import numpy as np
import pytest
import torch

from oracle import fixtures as fx
from tests import average_refs as AR
from tests import clip_refs as R
from tests.step_helpers import _student, deterministic_embed  # noqa: F401  (fixture)
from tests.test_distill_step_gpu import _config, dev  # noqa: F401  (fixture)
from tests.test_model_gpu import dev_batch, raw_batch

pytestmark = pytest.mark.gpu
NAMES = ["small_shared", "cfg1_query"]
INF = float("inf")


def _bits(t):
    return t.detach().contiguous().view({8: torch.int64, 4: torch.int32, 2: torch.int16}[t.element_size()])


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _step(c, dev, dropout=0.1, **kw):
    from mtn_amd.train_step import TrainStep
    model = _student(c, torch.bfloat16, dev, dropout)
    return model, TrainStep(model, dev_batch(raw_batch(c), dev), c["vocab"], pad=fx.PAD, warmup=10, **kw)


def _state(model, ts):
    adam = ts.opt.optimizer
    torch.cuda.synchronize()
    return model._flat.clone(), adam.m.clone(), adam.v.clone()


def _grad_norms(model):
    """(float64 norm of the whole flat gradient buffer, the same over the parameters' own .grad views), exactly rounded."""
    whole = R.norm_of(model._flat_grad.cpu().numpy())
    views = []
    for p, o in zip(model._flat_params, model._flat_offsets):
        assert p.grad is not None and p.grad.data_ptr() == model._flat_grad.data_ptr() + 4 * o
        views.append(p.grad.detach().reshape(-1).cpu().numpy())
    return whole, R.norm_of(np.concatenate(views))


@pytest.fixture(scope="module")
def measured(dev):
    """Per configuration, once: the three norms of a clip_grad_norm=inf run (dropout 0.1 and 0), read after each step."""
    import os
    cache = {}

    def get(name, dropout):
        if (name, dropout) not in cache:
            assert os.environ.get("MTN_EMBED_DETERMINISTIC") == "1"
            c = _config(name)
            model, ts = _step(c, dev, dropout, clip_grad_norm=INF, use_graph=False)
            norms = []
            for _ in range(3):
                ts()
                norms.append(float(ts.last_grad_norm))
            cache[(name, dropout)] = norms
        return cache[(name, dropout)]
    return get


# ------------------------------------------------------------------------------------------ (1)
@pytest.mark.parametrize("name", NAMES)
def test_measuring_changes_nothing_and_the_padding_stays_zero(dev, name, deterministic_embed):
    c = _config(name)
    model, ts = _step(c, dev, clip_grad_norm=INF, use_graph=False)
    assert ts.clipping and not ts._fused() and ts.opt.optimizer.clip_max_norm == INF
    for k in range(3):
        ts()
        whole, views = _grad_norms(model)
        got = float(ts.last_grad_norm)
        print("step %d: norm %.17g, of the gradient read back %.17g (relative error %.3g)" % (k + 1, got, whole, abs(got - whole) / whole))
        assert whole > 0 and whole == views                                   # nothing was written between the parameters
        assert abs(got - whole) <= 1e-12 * whole
    on = _state(model, ts)
    assert ts.last_grad_norm.dtype == torch.float64 and ts.last_grad_norm.is_cuda
    st = ts.opt.optimizer.clip_stats()
    assert st["steps"] == 3 and st["clipped"] == 0 and st["nonfinite"] == 0 and st["max"] >= st["mean"] > 0
    assert _same(ts.opt.optimizer.clip_scale, torch.ones(1, device=dev))      # an unclipped step multiplies by exactly one
    model_b, ts_b = _step(c, dev, fuse_optimizer=False, use_graph=False)
    assert not ts_b.clipping and ts_b.last_grad_norm is None
    for _ in range(3):
        ts_b()
    for a, b in zip(on, _state(model_b, ts_b)):
        assert _same(a, b)
    assert ts.opt.optimizer.clip_stats(reset=True)["steps"] == 3 and ts.opt.optimizer.clip_stats()["steps"] == 0
    assert "clip" not in " ".join(ts.opt.optimizer.state_dict())              # no state to resume


# ------------------------------------------------------------------------------------------ (2)
@pytest.mark.parametrize("name", NAMES)
def test_a_clipped_step_is_the_step_with_that_grad_scale(dev, name, deterministic_embed, measured):
    c = _config(name)
    C = float(np.float32(0.5 * measured(name, 0.1)[0]))
    model, ts = _step(c, dev, clip_grad_norm=C, use_graph=False)
    ts()
    adam = ts.opt.optimizer
    clipped = _state(model, ts)
    st = adam.clip_stats()
    assert st["steps"] == 1 and st["clipped"] == 1 and st["nonfinite"] == 0
    whole, _ = _grad_norms(model)
    assert abs(float(ts.last_grad_norm) - measured(name, 0.1)[0]) == 0.0      # the same gradient as the measuring run's
    want = R.scale_of(R.coef_of(whole, C))
    got = np.float32(float(adam.clip_scale))
    print("C %.9g norm %.17g scale %.9g reference %.9g" % (C, whole, got, want))
    assert 0.49 < float(got) < 0.51 and abs(got - want) <= np.spacing(want)
    model_b, ts_b = _step(c, dev, fuse_optimizer=False, use_graph=False)
    ts_b.opt.optimizer.grad_scale = adam.clip_scale.clone()                   # those same bits
    ts_b()
    for a, b in zip(clipped, _state(model_b, ts_b)):
        assert _same(a, b)
    model_c, ts_c = _step(c, dev, fuse_optimizer=False, use_graph=False)      # ... and not the unclipped step
    ts_c()
    assert not _same(clipped[1], _state(model_c, ts_c)[1])


# ------------------------------------------------------------------------------------------ (3)
@pytest.mark.parametrize("factor", [0.5, 2.0], ids=["half-of-step-1", "twice-the-largest"])
@pytest.mark.parametrize("name", NAMES)
def test_captured_equals_eager(dev, name, factor, deterministic_embed, measured):
    c = _config(name)
    norms = measured(name, 0.0)
    C = float(np.float32(0.5 * norms[0] if factor == 0.5 else 2.0 * max(norms)))

    def run(use_graph):
        model, ts = _step(c, dev, 0.0, clip_grad_norm=C, use_graph=use_graph)
        losses, seen = [], []
        for _ in range(3):
            losses.append(ts().clone())
            seen.append(ts.last_grad_norm.clone())
        return losses, seen, _state(model, ts), ts.opt.optimizer.clip_stats()

    cap, eag = run(True), run(False)
    for a, b in zip(cap[0] + cap[1] + list(cap[2]), eag[0] + eag[1] + list(eag[2])):
        assert _same(a, b)
    assert cap[3] == eag[3] and cap[3]["steps"] == 3 and cap[3]["nonfinite"] == 0
    if factor == 2.0:
        assert cap[3]["clipped"] == 0 and [float(v) for v in cap[1]] == norms  # nothing clipped: the measuring run's trajectory
    else:
        assert cap[3]["clipped"] >= 1 and float(cap[1][0]) == norms[0]


# ------------------------------------------------------------------------------------------ (4)
def test_the_average_follows_the_clipped_masters(dev, deterministic_embed, measured):
    name = "cfg1_query"
    c = _config(name)
    C = float(np.float32(0.5 * measured(name, 0.0)[0]))
    snaps_by = {}
    for key, kw in (("clipped", dict(clip_grad_norm=C)), ("plain", dict(fuse_optimizer=False))):
        model, ts = _step(c, dev, 0.0, ema_decay=0.9, use_graph=True, **kw)
        start = model._flat.clone()
        snaps = []
        for _ in range(3):
            ts()
            snaps.append(model._flat.clone())
        torch.cuda.synchronize()
        adam = ts.opt.optimizer
        want = AR.ema_run([s.cpu().numpy() for s in snaps], 0.9, start=start.cpu().numpy())
        got = adam.ema.cpu().numpy()
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), key
        snaps_by[key] = snaps
    assert not _same(snaps_by["clipped"][0], snaps_by["plain"][0])             # the masters it followed were the clipped ones


# ------------------------------------------------------------------------------------------ (5)
def test_scst_rows_with_clipping_captured_equals_eager(dev, deterministic_embed):
    from mtn_amd.train_step import TrainStep
    from tests.test_scst_step_gpu import S, _cfg, _fixed_rows
    c = _config("small_shared")
    raw = raw_batch(c)
    trg, trg_y, w = _fixed_rows(c, c["B"] * S, 23)

    def run(use_graph, C):
        model = _student(c, torch.bfloat16, dev, 0.0)
        ts = TrainStep(model, dev_batch(raw, dev), c["vocab"], pad=fx.PAD, warmup=10, use_graph=use_graph, scst=_cfg(c), clip_grad_norm=C)
        ts.load_rows(trg.to(dev), trg_y.to(dev), w)
        losses, norms = [], []
        for _ in range(2):
            losses.append(ts().clone())
            norms.append(ts.last_grad_norm.clone())
        return losses, norms, _state(model, ts), ts.opt.optimizer.clip_stats()

    C = float(np.float32(0.25 * float(run(False, INF)[1][0])))                 # a quarter of step 1's norm: step 1 clips
    cap, eag = run(True, C), run(False, C)
    for a, b in zip(cap[0] + cap[1] + list(cap[2]), eag[0] + eag[1] + list(eag[2])):
        assert _same(a, b)
    assert cap[3] == eag[3] and cap[3]["steps"] == 2 and cap[3]["clipped"] >= 1 and cap[3]["nonfinite"] == 0


# ------------------------------------------------------------------------------------------ what refuses
def test_refusals(dev):
    from mtn_amd import FusedAdam, lib
    from mtn_amd.train_step import TrainStep
    c = _config("small_shared")
    model = _student(c, torch.bfloat16, dev, 0.0)
    for bad in (0.0, -1.0, float("nan"), -INF):
        with pytest.raises(ValueError):
            FusedAdam(model).enable_clip(bad)
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError):
            TrainStep(model, dev_batch(raw_batch(c), dev), c["vocab"], pad=fx.PAD, clip_grad_norm=bad)
    adam = FusedAdam(model)
    assert adam.clip_max_norm is None
    with pytest.raises(lib.MtnHipError, match="clipping is off"):
        adam.clip_stats()
    fusable = adam.can_fuse()
    adam.enable_clip(1.0)
    assert not adam.can_fuse()
    with pytest.raises(lib.MtnHipError, match="clipping"):
        adam.step_range(0, 8)
    with pytest.raises(lib.MtnHipError, match="clipping"):
        adam.fuse_into_backward()
    ts = TrainStep(model, dev_batch(raw_batch(c), dev), c["vocab"], pad=fx.PAD)            # 0 = off: today's step, fused where it was
    assert not ts.clipping and ts._fused() == fusable and ts.last_grad_norm is None
    assert math.isinf(TrainStep(model, dev_batch(raw_batch(c), dev), c["vocab"], pad=fx.PAD, clip_grad_norm=INF).opt.optimizer.clip_max_norm)
