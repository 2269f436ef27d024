"""R-Drop inside the training step (mtn_amd.train_step.TrainStep(rdrop=...)) on the small configurations of
tests/test_unlikelihood_step_gpu.py, with its helpers and its bars:
  (a) rdrop = 0 leaves the step what it was, bit for bit and launch for launch, eager and captured;
  (b) a pre-paired batch (rdrop_paired) in float32 with dropout 0: loss, last_rd and every parameter gradient against the CPU oracle plus
      the float64 definition of tests/rdrop_refs.py through autograd;
  (c) under dropout 0.1, replicated from B dialogues: last_rd > 0, fresh masks on every replay, and with the dropout seed pinned the
      R-Drop step's loss is the plain step's on the same doubled batch + rdrop * last_rd;
  (d) with dropout 0.0 the two passes agree and last_rd is under the kernel's floor;
  (e) eager and captured steps give the same loss bits;
  (f) the conflicts raise, naming what conflicts; a paired batch whose halves' targets differ raises naming the row;
  (g) train.py --rdrop-alpha logs the epoch line with a finite value: the fixed synthetic batch, and the synthetic corpus graphed and
      --eager."""
import contextlib
import io
import math
import re

import numpy as np
import pytest
import torch

from oracle import fixtures as fx
from tests import rdrop_refs as rd
from tests.step_helpers import _census, _student, deterministic_embed  # noqa: F401  (fixture)
from tests.test_distill_step_gpu import NAMES, _config, _teacher
from tests.test_model_gpu import dev_batch, raw_batch
from tests.util import TOL, relmax

pytestmark = pytest.mark.gpu
RD_LINE = re.compile(r"^epoch (\d+) mean R-Drop divergence per token: (\S+)$", re.M)
SEED = 4242


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


def _doubled(raw):
    """The raw batch twice: rows b and B + b the same dialogue."""
    return {k: ([np.concatenate([f, f]) for f in v] if k == "fts" else np.concatenate([v, v])) for k, v in raw.items()}


def _paired(c):
    """A raw batch of 2 N dialogues in pair layout: the second half shares the first half's questions, captions and targets and has
    another history and other features (those of the configuration's batch of seed 2)."""
    a, b = raw_batch(c), raw_batch(c, seed=2)
    out = _doubled(a)
    N = a["query"].shape[0]
    out["his"][N:] = b["his"]
    for f, g in zip(out["fts"], b["fts"]):
        f[N:] = g
    return out


# ------------------------------------------------------------------------------------------ (a)
@pytest.mark.parametrize("name", NAMES)
def test_alpha_zero_leaves_the_step_bitwise(dev, name, deterministic_embed):
    from mtn_amd.train_step import TrainStep
    c = _config(name)
    b = dev_batch(raw_batch(c), dev)

    def run(use_graph, **kw):
        model = _student(c, torch.bfloat16, dev, 0.1)
        ts = TrainStep(model, b, c["vocab"], pad=fx.PAD, warmup=10, use_graph=use_graph, **kw)
        losses = [ts().clone() for _ in range(3)]
        torch.cuda.synchronize()
        return losses, model._flat.clone(), ts

    for use_graph in (True, False):
        plain_l, plain_p, _ = run(use_graph)
        zero_l, zero_p, ts = run(use_graph, rdrop=0.0)
        for a, d in zip(plain_l, zero_l):
            assert torch.equal(a.view(torch.int32), d.view(torch.int32)), (float(a), float(d))
        assert torch.equal(plain_p.view(torch.int32), zero_p.view(torch.int32))
        assert plain_l[0].item() != plain_l[2].item()                    # the steps did train
        assert ts.last_rd is None and ts.batch is b and ts._rd_src is None
    rd_l, _, ts = run(True, rdrop=1.0)                                   # and the flag does change the step
    assert float(ts.last_rd) > 0 and ts.batch.trg_y.size(0) == 2 * b.trg_y.size(0) and math.isfinite(float(rd_l[2]))

    def eager(**kw):
        model = _student(c, torch.bfloat16, dev, 0.1)
        ts = TrainStep(model, b, c["vocab"], pad=fx.PAD, warmup=10, use_graph=False, **kw)
        step = ts._step_fused if ts._fused() else ts._fwd_bwd
        step()                                                           # (lazy set-up outside the census)
        return _census(step)

    plain_c, plain_f = eager()
    assert len(plain_c) > 0
    assert eager(rdrop=0.0) == (plain_c, plain_f)


# ------------------------------------------------------------------------------------------ (b)
def _oracle_reference(c, raw, alpha):
    """(loss, {parameter name: gradient}, rd per token) of the R-Drop loss on the CPU oracle: its forward and plain loss, the float64
    definition of tests/rdrop_refs.py on its log-probabilities, autograd through both."""
    ob = fx.oracle_batch(raw)
    student, _ = fx.oracle_from_config(c, seed=0, requires_grad=True)
    out, ae = student.forward(ob)
    logp = student.generator(out)
    norm = ob.ntokens.float()
    rows = rd.rd_rows_of_logp(logp.reshape(-1, logp.size(-1)).double(), ob.trg_y.reshape(-1), fx.PAD).sum()
    total = student.loss(ob, out, ae).double() + alpha * rows / norm.double()
    total.backward()
    return float(total.detach()), {k: v.grad for k, v in student.p.items() if v.grad is not None}, float(rows.detach() / norm)


@pytest.mark.parametrize("name", NAMES)
def test_rdrop_loss_and_gradients_match_the_oracle(dev, name):
    from mtn_amd.train_step import TrainStep
    dtype, alpha = torch.float32, 1.0
    c = _config(name)
    raw = _paired(c)
    ref_loss, ref_grads, ref_rd = _oracle_reference(c, raw, alpha)
    model = _student(c, dtype, dev, 0.0)
    ts = TrainStep(model, dev_batch(raw, dev), c["vocab"], pad=fx.PAD, warmup=10, use_graph=False, fuse_optimizer=False, rdrop=alpha,
                   rdrop_paired=True)
    assert ts._rd_src is None                                           # the batch is used as it is
    out, ae_out = model.forward(ts.batch)                               # the loss is the fused HIP head's, not the composed fallback's
    probe = ts._loss_of(out, ae_out, None)
    assert probe.grad_fn is not None and "GeneratorLossFn" in type(probe.grad_fn).__name__
    del probe, out, ae_out
    loss = ts._fwd_bwd()
    torch.cuda.synchronize()
    tol = TOL[dtype]
    print(f"{name} {dtype}: loss {float(loss):.6f} (oracle {ref_loss:.6f})  rd/token {float(ts.last_rd):.6f} (oracle {ref_rd:.6f})")
    assert ref_rd > 1e-3                                                # the perturbed half does move the distributions
    assert abs(float(loss) - ref_loss) < tol * max(1.0, abs(ref_loss))
    assert abs(float(ts.last_rd) - ref_rd) < tol * max(1.0, abs(ref_rd))
    gtol = 3e-3                                                         # test_model_loss_and_grads_match_reference_golden's float32 bar
    params = dict(model.named_parameters())
    worst, dot, n1, n2, checked = 0.0, 0.0, 0.0, 0.0, 0
    for k, ref in ref_grads.items():
        if k not in params:
            continue
        gr = params[k].grad
        assert gr is not None, k
        n, gn = float(ref.double().norm()), float(gr.double().norm())
        if n < 1e-6:
            assert gn < 1e-5, (k, gn)
            continue
        e = max(relmax(gr, ref), abs(gn - n) / n)
        dot += float((gr.double().cpu() * ref.double()).sum()); n1 += gn * gn; n2 += n * n
        worst = max(worst, e)
        checked += 1
        assert e < gtol, (k, e)
    cos = dot / (n1 ** 0.5 * n2 ** 0.5)
    print(f"worst grad rel err {worst:.2e} over {checked} tensors, cosine {cos:.7f}")
    assert checked > 20
    assert cos > 0.999999, cos


# ------------------------------------------------------------------------------------------ (c)
def test_under_dropout_the_passes_differ_and_every_replay_draws_anew(dev):
    from mtn_amd.train_step import TrainStep
    c = _config("small_shared")
    model = _student(c, torch.bfloat16, dev, 0.1)
    ts = TrainStep(model, dev_batch(raw_batch(c), dev), c["vocab"], pad=fx.PAD, warmup=10, rdrop=1.0)
    vals = []
    for _ in range(2):
        ts()
        vals.append(float(ts.last_rd))
    print("last_rd of two replays:", vals)
    assert all(math.isfinite(v) and v > 0 for v in vals) and vals[0] != vals[1]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_with_the_seed_pinned_the_loss_is_the_plain_loss_plus_alpha_rd(dev, dtype):
    """The plain step on the doubled batch and the R-Drop step replicated from the B dialogues, same weights, same dropout seed: the
    forward passes are the same launches on the same bytes, so the two losses differ by rdrop * last_rd and by float32 rounding alone.
    The bound: a row's scale (KL_ls + rdrop rd) is 3 roundings where the plain row's scale KL_ls is 1 (each 2^-24 of the row's loss);
    the loss is a float32 tree sum over R = 2 B T + auto-encoder rows <= 2^10 (<= log2 R + 1 roundings of partial sums, each 2^-24 of the
    total) on either side, last_rd one more such sum and a division: (4 + 2 * 11 + 13) 2^-24 < 64 * 2^-24 of the R-Drop loss."""
    from mtn_amd.train_step import TrainStep
    c = _config("small_shared")
    raw, alpha = raw_batch(c), 5.0
    out = []
    for kw, r in ((dict(), _doubled(raw)), (dict(rdrop=alpha), raw)):
        model = _student(c, dtype, dev, 0.1)
        ts = TrainStep(model, dev_batch(r, dev), c["vocab"], pad=fx.PAD, warmup=10, use_graph=False, fuse_optimizer=False, **kw)
        model._seed.fill_(SEED)
        loss = ts._fwd_bwd()
        out.append((float(loss), 0.0 if ts.last_rd is None else float(ts.last_rd), ts))
    torch.cuda.synchronize()
    (plain, _, tp), (with_rd, last_rd, tr) = out
    assert tr.batch.trg_y.size(0) == tp.batch.trg_y.size(0) and torch.equal(tr.batch.trg_y, tp.batch.trg_y)
    assert torch.equal(tr._norms, tp._norms)
    tolerance = 64 * 2.0 ** -24 * abs(with_rd)
    print(f"{dtype}: plain {plain:.7f}  R-Drop {with_rd:.7f}  last_rd {last_rd:.7f}  difference {with_rd - plain - alpha * last_rd:.3e} "
          f"(bound {tolerance:.3e})")
    assert last_rd > 0
    assert abs(with_rd - (plain + alpha * last_rd)) <= tolerance


# ------------------------------------------------------------------------------------------ (d)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_without_dropout_there_is_no_divergence(dev, dtype):
    from mtn_amd.train_step import TrainStep
    c = _config("cfg1_query")
    model = _student(c, dtype, dev, 0.0)
    ts = TrainStep(model, dev_batch(raw_batch(c), dev), c["vocab"], pad=fx.PAD, warmup=10, rdrop=1.0)
    for _ in range(2):
        ts()
        print(f"{dtype}: last_rd {float(ts.last_rd):.3e} (floor {rd.RD_FLOOR:.3e})")
        assert 0.0 <= float(ts.last_rd) <= rd.RD_FLOOR


# ------------------------------------------------------------------------------------------ (e)
def test_eager_and_captured_steps_give_the_same_loss_bits(dev, deterministic_embed):
    from mtn_amd.train_step import TrainStep
    c = _config("small_shared")
    b = dev_batch(raw_batch(c), dev)
    runs = []
    for use_graph in (False, True):
        model = _student(c, torch.bfloat16, dev, 0.0)
        ts = TrainStep(model, b, c["vocab"], pad=fx.PAD, warmup=10, use_graph=use_graph, rdrop=1.0)
        runs.append([(ts().clone(), ts.last_rd.clone()) for _ in range(3)])
    torch.cuda.synchronize()
    for (le, re_), (lg, rg) in zip(*runs):
        assert torch.equal(le.view(torch.int32), lg.view(torch.int32)), (float(le), float(lg))
        assert torch.equal(re_.view(torch.int32), rg.view(torch.int32))
    assert float(runs[0][2][0]) != float(runs[0][0][0])


def test_a_source_refilled_in_place_reaches_the_captured_step(dev, deterministic_embed):
    """The refill is part of the captured step: new dialogues written into the source batch's tensors are what the next replay trains
    on, normalisers included (dynamic_norms) — the loss equals a fresh eager step's on that batch, bit for bit."""
    from mtn_amd.train_step import TrainStep
    c = _config("small_shared")
    first, second = dev_batch(raw_batch(c), dev), dev_batch(raw_batch(c, seed=2), dev)

    def fresh(batch, use_graph):
        model = _student(c, torch.bfloat16, dev, 0.0)
        return TrainStep(model, batch, c["vocab"], pad=fx.PAD, warmup=10, use_graph=use_graph, dynamic_norms=True, rdrop=1.0)

    want = fresh(second, False)().clone()
    src = dev_batch(raw_batch(c), dev)
    ts = fresh(src, True)
    ts._capture()
    for name in ("query", "his", "cap", "trg", "trg_y", "query_mask", "his_mask", "cap_mask", "trg_mask"):
        getattr(src, name).copy_(getattr(second, name))
    for f, m, sf, sm in zip(src.fts, src.fts_mask, second.fts, second.fts_mask):
        f.copy_(sf)
        m.copy_(sm)
    got = ts().clone()
    torch.cuda.synchronize()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (float(got), float(want))
    assert not torch.equal(first.trg_y, second.trg_y)


@pytest.mark.parametrize("use_graph", [True, False], ids=["graphs", "eager"])
def test_combines_with_clipping_ema_and_accumulation(dev, use_graph):
    """The switches the step combines with, all at once: a window of two micro-steps on the doubled batch, clipped, with the averaged
    weights kept.  Every figure is finite, the weights moved once per window, and the divergence is there on both micro-steps."""
    from mtn_amd.train_step import TrainStep
    c = _config("small_shared")
    model = _student(c, torch.bfloat16, dev, 0.1)
    before = model._flat.clone()
    ts = TrainStep(model, dev_batch(raw_batch(c), dev), c["vocab"], pad=fx.PAD, warmup=10, use_graph=use_graph, rdrop=1.0,
                   clip_grad_norm=0.5, ema_decay=0.99, accumulate=True)
    assert ts.clipping and ts.accumulating and ts.batch.trg_y.size(0) == 2 * c["B"]
    l0, r0 = float(ts(False)), float(ts.last_rd)
    torch.cuda.synchronize()
    assert torch.equal(model._flat, before)                             # the window is still open
    l1, r1 = float(ts(True)), float(ts.last_rd)
    torch.cuda.synchronize()
    assert not torch.equal(model._flat, before) and bool(torch.isfinite(model._flat).all())
    assert all(math.isfinite(v) and v > 0 for v in (l0, l1, r0, r1, float(ts.last_grad_norm)))
    assert ts.opt.step_count() == 1


# ------------------------------------------------------------------------------------------ (f)
def test_conflicts_raise_and_name_what_conflicts(dev):
    from mtn_amd import ops
    from mtn_amd.train_step import BucketedTrainer, SchedConfig, ScstConfig, TrainStep
    c = _config("cfg1_query")
    b = dev_batch(raw_batch(c), dev)
    model = _student(c, torch.bfloat16, dev, 0.0)
    teacher = _teacher(c, torch.bfloat16, dev, 1)
    scst = ScstConfig.__new__(ScstConfig)                                # (never looked at: the conflict is refused first)
    for cls, args in ((TrainStep, (model, b, c["vocab"])), (BucketedTrainer, (model, None, c["vocab"]))):
        with pytest.raises(ValueError, match="rdrop does not combine with a teacher"):
            cls(*args, pad=fx.PAD, teacher=teacher, rdrop=1.0)
        with pytest.raises(ValueError, match="rdrop does not combine with scst"):
            cls(*args, pad=fx.PAD, scst=scst, rdrop=1.0)
        with pytest.raises(ValueError, match="rdrop does not combine with unlikelihood"):
            cls(*args, pad=fx.PAD, unlikelihood=1.0, rdrop=1.0)
        with pytest.raises(ValueError, match="rdrop does not combine with sched"):
            cls(*args, pad=fx.PAD, sched=SchedConfig(0.25), rdrop=1.0)
        for bad in (-1.0, float("nan"), float("inf")):
            with pytest.raises(ValueError, match="finite"):
                cls(*args, pad=fx.PAD, rdrop=bad)
    # a paired batch whose halves' targets differ: the first such row is named
    raw = _paired(c)
    N = raw["trg_y"].shape[0] // 2
    raw["trg_y"][N + 2, 1] = raw["trg_y"][N + 2, 1] + 1
    raw["trg_y"][N + 3, 0] = raw["trg_y"][N + 3, 0] + 1
    with pytest.raises(ValueError, match=r"row 2 and of its partner, row %d, differ" % (N + 2)):
        TrainStep(model, dev_batch(raw, dev), c["vocab"], pad=fx.PAD, rdrop=1.0, rdrop_paired=True)
    with pytest.raises(ValueError, match="2 N rows"):
        TrainStep(model, dev_batch(raw_batch(dict(c, B=3)), dev), c["vocab"], pad=fx.PAD, rdrop=1.0, rdrop_paired=True)
    # the autograd function itself: a teacher, row weights or unlikelihood next to spec["rdrop"]
    ts = TrainStep(model, b, c["vocab"], pad=fx.PAD, warmup=10, use_graph=False, rdrop=1.0)
    out, ae_out = model.forward(ts.batch)
    rows, V = ts.batch.trg_y.numel(), c["vocab"]
    with pytest.raises(ValueError, match="R-Drop does not combine with teacher"):
        ts.lc._fused_loss(out, ts.batch.trg_y, ts._norms[0], None, None, None, teacher_logp=torch.zeros(rows, V, device=dev), alpha=0.5,
                          rdrop=1.0)
    with pytest.raises(ValueError, match="R-Drop does not combine with row weights"):
        ts.lc._fused_loss(out, ts.batch.trg_y, ts._norms[0], None, None, None, row_weights=torch.ones(rows, device=dev), rdrop=1.0)
    with pytest.raises(ValueError, match="R-Drop does not combine with unlikelihood"):
        ts.lc._fused_loss(out, ts.batch.trg_y, ts._norms[0], None, None, None, unlikelihood=1.0, rdrop=1.0)
    assert "rdrop" in ops.LOSS_HEADS


# ------------------------------------------------------------------------------------------ (g)
SMALL = ["--nb-blocks", "1", "--d-model", "64", "--d-ff", "128", "--att-h", "4", "--vocab-size", "64", "--ft-sizes", "16", "8",
         "--warmup-steps", "20", "--report-interval", "1000", "--dropout", "0.1", "--batch-size", "8"]
CORPUS = SMALL + ["--corpus-videos", "3", "--valid-videos", "1", "--max-length", "12", "--corpus-max-answer", "8", "--corpus-max-question", "8"]


def _run(argv):
    from mtn_amd import train
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        train.main(argv)
    return buf.getvalue()


def _rd_values(out, epochs):
    rows = RD_LINE.findall(out)
    assert [int(r[0]) for r in rows] == list(range(1, epochs + 1)), out
    vals = [float(r[1]) for r in rows]
    assert all(math.isfinite(v) and v > 0.0 for v in vals), vals
    return vals


def test_train_py_logs_the_epoch_line_on_the_fixed_batch(dev):
    out = _run(SMALL + ["--lens", "6", "12", "8", "7", "4", "--rdrop-alpha", "1", "--steps-per-epoch", "3", "--num-epochs", "2"])
    _rd_values(out, 2)
    assert "R-Drop" not in _run(SMALL + ["--lens", "6", "12", "8", "7", "4", "--steps-per-epoch", "3"])


@pytest.mark.parametrize("eager", [False, True], ids=["graphed", "eager"])
def test_train_py_logs_the_epoch_line_on_the_synthetic_corpus(dev, eager):
    out = _run(CORPUS + ["--rdrop-alpha", "1"] + (["--eager"] if eager else []))
    _rd_values(out, 1)
    assert "validation loss" in out                                     # validation stays the plain loss
