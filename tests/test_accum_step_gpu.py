"""Gradient accumulation inside the training step (FusedAdam.enable_accumulation, TrainStep(accumulate=True)) on the small configurations
of tests/test_model_gpu.py, with the helpers tests/test_clip_step_gpu.py imports and dropout as the other step tests set it (0.1 where one
schedule is compared with itself; 0 where a captured step is compared with an eager one):
  (1) a window of one is the fuse_optimizer=False step bit for bit: weights and moments after three steps;
  (2) a two-batch window (the same rows, the second with shorter answers: w_1 != w_2) leaves the weights, moments and gradient buffer of
      a reference built by hand: a second model at the same weights, _fwd_bwd() on each batch, G from tests/accum_refs.py copied into
      the gradient buffer, _optim();
  (3) captured equals eager bit for bit over three windows of K = 2;
  (4) the definition is the right one, in fp32 compute with lam = 0 (the auto-encoder weighting, which legitimately differs, stays out):
      a batch's rows split unevenly into two micro-batches whose target-token counts differ at least 2:1 give, per parameter tensor, the
      gradient of the whole batch within 1e-3 relative L2 (the project's fp32 parity bar) — and on the generator weight the unweighted
      mean (g_1 + g_2) / 2 misses that bar, so the test can tell the two definitions apart.  The attention KEY biases are the one
      exception in form, not in strictness: their gradient is zero by softmax's shift invariance, both runs hold rounding residue
      there, and the bar is applied at the scale of the same attention's query-bias gradient;
  (5) with clipping at half of window 1's norm: last_grad_norm is the float64 norm of the gradient buffer within 1e-12, the weights are
      the reference's of (2) with that scale, and no mtn_grad_sumsq launch is issued (the closing launch wrote the partials);
  (6) ema_decay with K = 2: the average follows the masters after each WINDOW;
  (7) what refuses: the fused epilogue, the sharded update, scst."""
import numpy as np
import pytest
import torch

from oracle import fixtures as fx
from tests import accum_refs as R
from tests import average_refs as AR
from tests import clip_refs as CR
from tests.step_helpers import _student, deterministic_embed  # noqa: F401  (fixture)
from tests.test_distill_step_gpu import _config, dev  # noqa: F401  (fixture)
from tests.test_model_gpu import dev_batch, raw_batch

pytestmark = pytest.mark.gpu
NAMES = ["small_shared", "cfg1_query"]


def _bits(t):
    return t.detach().contiguous().view({8: torch.int64, 4: torch.int32, 2: torch.int16}[t.element_size()])


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _shorter(raw, keep=3):
    """The same rows with every answer but the first cut to ``keep`` target positions: another target-token count."""
    out = dict(raw, trg=raw["trg"].copy(), trg_y=raw["trg_y"].copy())
    out["trg"][1:, keep:] = fx.PAD
    out["trg_y"][1:, keep:] = fx.PAD
    return out


def _rows(raw, rows):
    return dict(query=raw["query"][rows], his=raw["his"][rows], cap=raw["cap"][rows], trg=raw["trg"][rows], trg_y=raw["trg_y"][rows],
                fts=[f[rows] for f in raw["fts"]])


def _steps(c, dev, raws, dropout=0.1, dtype=torch.bfloat16, opt_kw=None, **kw):
    """One model and one TrainStep per raw batch over one optimiser (the first step's; ``opt_kw`` are what it enables there)."""
    from mtn_amd.train_step import TrainStep
    model = _student(c, dtype, dev, dropout)
    first = TrainStep(model, dev_batch(raws[0], dev), c["vocab"], pad=fx.PAD, warmup=10, **dict(kw, **(opt_kw or {})))
    rest = [TrainStep(model, dev_batch(r, dev), c["vocab"], pad=fx.PAD, warmup=10, opt=first.opt, **kw) for r in raws[1:]]
    return model, [first] + rest


def _state(model, ts):
    adam = ts.opt.optimizer
    torch.cuda.synchronize()
    return model._flat.clone(), adam.m.clone(), adam.v.clone()


def _reference_window(c, dev, raws, dropout=0.1, grad_scale=None, **kw):
    """(2)'s reference: _fwd_bwd() on each batch, the gradients read back, G built by tests/accum_refs.py, copied into the gradient
    buffer, _optim().  Returns (model, steps, G as numpy, [w_k])."""
    model, steps = _steps(c, dev, raws, dropout, fuse_optimizer=False, use_graph=False, **kw)
    gs, ws = [], []
    for ts in steps:
        ts._fwd_bwd()
        torch.cuda.synchronize()
        gs.append(model._flat_grad.cpu().numpy().copy())
        ws.append(np.float32(float(ts._norms[0])))
    G, total = R.window(gs, ws)
    model._flat_grad.copy_(torch.from_numpy(G))
    if grad_scale is not None:
        steps[-1].opt.optimizer.grad_scale = grad_scale
    steps[-1]._optim()
    return model, steps, G, ws


# ------------------------------------------------------------------------------------------ (1)
@pytest.mark.parametrize("name", NAMES)
def test_a_window_of_one_is_the_unfused_step(dev, name, deterministic_embed):
    c = _config(name)
    raw = raw_batch(c)
    model, (ts,) = _steps(c, dev, [raw], opt_kw=dict(accumulate=True), use_graph=False)
    adam = ts.opt.optimizer
    assert ts.accumulating and not ts._fused() and adam.accum is not None and adam.accum.shape == model._flat_grad.shape
    for _ in range(3):
        ts(True)
    on = _state(model, ts)
    assert adam.accum_windows == adam.accum_micro == 3 and ts.opt.step_count() == 3
    assert not bool(adam.accum.any()) and not bool(adam._accum_total.any())           # nothing was launched
    model_b, (ts_b,) = _steps(c, dev, [raw], fuse_optimizer=False, use_graph=False)
    assert not ts_b.accumulating
    for _ in range(3):
        ts_b()
    for a, b in zip(on, _state(model_b, ts_b)):
        assert _same(a, b)
    assert "accum" not in " ".join(adam.state_dict())                                 # no state to resume


# ------------------------------------------------------------------------------------------ (2)
@pytest.mark.parametrize("name", NAMES)
def test_a_two_batch_window_is_the_reference_built_by_hand(dev, name, deterministic_embed):
    c = _config(name)
    raws = [raw_batch(c), _shorter(raw_batch(c))]
    model_b, steps_b, G, ws = _reference_window(c, dev, raws)
    assert ws[0] != ws[1] and ws[1] >= 1
    model, steps = _steps(c, dev, raws, opt_kw=dict(accumulate=True), use_graph=False)
    start = model._flat.clone()
    loss1 = steps[0](False).clone()
    torch.cuda.synchronize()
    assert _same(model._flat, start) and steps[0].opt.step_count() == 0               # weights do not move inside a window
    loss2 = steps[1](True).clone()
    for a, b in zip(_state(model, steps[1]), _state(model_b, steps_b[1])):
        assert _same(a, b)
    assert R.same_bytes(model._flat_grad.cpu().numpy(), G)
    adam = steps[0].opt.optimizer
    assert float(adam._accum_total[1]) == float(ws[0]) + float(ws[1]) and adam.accum_windows == 1 and adam.accum_micro == 2
    assert steps[0].opt.step_count() == 1 and float(loss1) != float(loss2)            # the step count counts windows; each loss is its micro-step's


# ------------------------------------------------------------------------------------------ (3)
@pytest.mark.parametrize("name", NAMES)
def test_captured_equals_eager(dev, name, deterministic_embed):
    c = _config(name)
    raws = [raw_batch(c), _shorter(raw_batch(c))]

    def run(use_graph):
        model, steps = _steps(c, dev, raws, 0.0, opt_kw=dict(accumulate=True), use_graph=use_graph)
        losses = []
        for _ in range(3):
            losses.append(steps[0](False).clone())
            losses.append(steps[1](True).clone())
        return losses, _state(model, steps[0]), model._flat_grad.clone(), steps[0].opt.step_count()

    cap, eag = run(True), run(False)
    for a, b in zip(cap[0] + list(cap[1]) + [cap[2]], eag[0] + list(eag[1]) + [eag[2]]):
        assert _same(a, b)
    assert cap[3] == eag[3] == 3


# ------------------------------------------------------------------------------------------ (4)
@pytest.mark.parametrize("name", NAMES)
def test_the_window_gradient_is_the_whole_batch_gradient(dev, name, deterministic_embed):
    c = _config(name)
    raw = raw_batch(c)
    B = raw["trg"].shape[0]
    raw["trg"][B - 1, 3:] = fx.PAD                                                     # the last row's answer: three target positions
    raw["trg_y"][B - 1, 3:] = fx.PAD
    parts = [_rows(raw, slice(0, B - 1)), _rows(raw, slice(B - 1, B))]
    kw = dict(dropout=0.0, dtype=torch.float32, lam=0.0, use_graph=False)
    model_w, (whole,) = _steps(c, dev, [raw], fuse_optimizer=False, **kw)
    whole._fwd_bwd()
    model_p, halves = _steps(c, dev, parts, fuse_optimizer=False, **kw)
    gs = []
    for ts in halves:
        ts._fwd_bwd()
        gs.append(model_p._flat_grad.clone())
    model, steps = _steps(c, dev, parts, opt_kw=dict(accumulate=True), **kw)
    steps[0](False)
    steps[1](True)
    torch.cuda.synchronize()
    w = [float(ts._norms[0]) for ts in steps]
    print("target tokens of the micro-batches: %g and %g, of the whole batch %g" % (w[0], w[1], float(whole._norms[0])))
    assert w[0] >= 2 * w[1] > 0 and w[0] + w[1] == float(whole._norms[0])
    want, got, mean = model_w._flat_grad.double(), model._flat_grad.double(), 0.5 * (gs[0].double() + gs[1].double())
    names = {id(p): n for n, p in model.named_parameters()}
    gen = id(model.generator.proj.weight)
    seen_gen = False
    for p, o in zip(model._flat_params, model._flat_offsets):
        sl = slice(o, o + p.numel())
        ref = float(want[sl].norm())
        err = float((got[sl] - want[sl]).norm())
        print("%-60s |whole| %.4g relative L2 %.3g" % (names[id(p)], ref, err / ref if ref else 0.0))
        if ref == 0.0:
            assert err == 0.0, names[id(p)]
            continue
        if names[id(p)].endswith(".linears.1.bias"):
            # An attention's KEY bias has no gradient: it adds the same q . b to every score of a row and softmax does not see it.
            # What the kernels leave there is the rounding residue of dK's column sums (1e-9 here, next to 1e-2 on the query bias),
            # and an error relative to a residue says nothing.  The bar is held at the scale of the same attention's query bias
            # instead: the same shape, the same layer, a gradient that exists.
            q = names[id(p)][:-len("1.bias")] + "0.bias"
            scale = next(float(want[oo:oo + pp.numel()].norm()) for pp, oo in zip(model._flat_params, model._flat_offsets) if names[id(pp)] == q)
            assert ref <= 1e-3 * scale and err <= 1e-3 * scale, names[id(p)]
            continue
        assert err <= 1e-3 * ref, names[id(p)]
        if id(p) == gen:
            miss = float((mean[sl] - want[sl]).norm()) / ref
            print("generator weight: the unweighted mean's relative L2 %.3g" % miss)
            assert miss > 1e-3
            seen_gen = True
    assert seen_gen


# ------------------------------------------------------------------------------------------ (5)
@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "captured"])
@pytest.mark.parametrize("name", NAMES)
def test_clipping_reads_the_closing_launch_partials(dev, name, use_graph, deterministic_embed):
    from mtn_amd import lib as L
    c = _config(name)
    dropout = 0.0 if use_graph else 0.1                                                # (capture's warm-up passes advance the dropout stream)
    raws = [raw_batch(c), _shorter(raw_batch(c))]
    model_m, steps_m = _steps(c, dev, raws, dropout, opt_kw=dict(accumulate=True, clip_grad_norm=float("inf")), use_graph=False)
    steps_m[0](False)
    steps_m[1](True)
    norm1 = float(steps_m[1].last_grad_norm)
    C = float(np.float32(0.5 * norm1))
    h, calls = L.load(), []
    real = h.mtn_grad_sumsq
    model, steps = _steps(c, dev, raws, dropout, opt_kw=dict(accumulate=True, clip_grad_norm=C), use_graph=use_graph)
    adam = steps[0].opt.optimizer
    if use_graph:                  # captured up front: forward/backward, and the optimiser graph of a window of ONE, which holds the norm
        for ts in steps:           # launch and is not replayed below; the graph that reads the partials is captured inside the window
            ts._capture()
    h.mtn_grad_sumsq = lambda *a: (calls.append(a[0]), real(*a))[1]                    # the entry, wrapped: every call is counted
    try:
        steps[0](False)
        steps[1](True)
        torch.cuda.synchronize()
    finally:
        h.mtn_grad_sumsq = real
    assert calls == []                                                                 # the closing launch wrote the partials
    got, whole = float(steps[1].last_grad_norm), CR.norm_of(model._flat_grad.cpu().numpy())
    print("norm %.17g of the gradient read back %.17g (relative error %.3g), measuring run %.17g" % (got, whole, abs(got - whole) / whole, norm1))
    assert abs(got - whole) <= 1e-12 * whole and got == norm1
    st = adam.clip_stats()
    assert st["steps"] == 1 and st["clipped"] == 1 and st["nonfinite"] == 0 and 0.49 < float(adam.clip_scale) < 0.51
    after = _state(model, steps[1])
    if not use_graph:                                                                  # (2)'s reference, with that scale
        model_b, steps_b, G, _ = _reference_window(c, dev, raws, dropout, grad_scale=adam.clip_scale.clone())
        for a, b in zip(after, _state(model_b, steps_b[1])):
            assert _same(a, b)
    else:                                                                              # the eager run of the same window
        model_e, steps_e = _steps(c, dev, raws, dropout, opt_kw=dict(accumulate=True, clip_grad_norm=C), use_graph=False)
        steps_e[0](False)
        steps_e[1](True)
        for a, b in zip(after, _state(model_e, steps_e[1])):
            assert _same(a, b)
        steps[1](True)                                                                 # a window of one on the captured step: the norm launch is back
        torch.cuda.synchronize()
        assert adam.clip_stats()["steps"] == 2


# ------------------------------------------------------------------------------------------ (6)
def test_the_average_follows_the_masters_after_each_window(dev, deterministic_embed):
    c = _config("cfg1_query")
    raws = [raw_batch(c), _shorter(raw_batch(c))]
    model, steps = _steps(c, dev, raws, 0.0, opt_kw=dict(accumulate=True, ema_decay=0.9), use_graph=True)
    start = model._flat.clone()
    snaps = []
    for _ in range(3):
        steps[0](False)
        assert _same(model._flat, start if not snaps else snaps[-1])
        steps[1](True)
        snaps.append(model._flat.clone())
    torch.cuda.synchronize()
    want = AR.ema_run([s.cpu().numpy() for s in snaps], 0.9, start=start.cpu().numpy())
    got = steps[0].opt.optimizer.ema.cpu().numpy()
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    assert not _same(snaps[0], start) and not _same(snaps[1], snaps[0])


# ------------------------------------------------------------------------------------------ (7)
def test_refusals(dev):
    from mtn_amd import FusedAdam, lib
    from mtn_amd.train_step import BucketedTrainer, TrainStep
    from tests.test_scst_step_gpu import _cfg
    c = _config("small_shared")
    model = _student(c, torch.bfloat16, dev, 0.0)
    adam = FusedAdam(model)
    assert adam.accum is None
    with pytest.raises(lib.MtnHipError, match="accumulation is off"):
        adam.accumulate(torch.ones(1, device=dev), True)
    fusable = adam.can_fuse()
    adam.enable_accumulation()
    assert not adam.can_fuse()
    with pytest.raises(lib.MtnHipError, match="accumulation"):
        adam.step_range(0, 8)
    with pytest.raises(lib.MtnHipError, match="accumulation"):
        adam.fuse_into_backward()
    with pytest.raises(ValueError):
        adam.accumulate(1.0, True)                                                     # w is a device float
    with pytest.raises(ValueError, match="accumulation"):
        TrainStep(model, dev_batch(raw_batch(c), dev), c["vocab"], pad=fx.PAD, scst=_cfg(c), accumulate=True)
    with pytest.raises(ValueError, match="accumulation"):
        BucketedTrainer(model, None, c["vocab"], pad=fx.PAD, scst=_cfg(c), accum_steps=2)
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError, match="accum_steps"):
            BucketedTrainer(model, None, c["vocab"], pad=fx.PAD, accum_steps=bad)
    ts = TrainStep(model, dev_batch(raw_batch(c), dev), c["vocab"], pad=fx.PAD)        # off: today's step, fused where it was
    assert not ts.accumulating and ts._fused() == fusable
