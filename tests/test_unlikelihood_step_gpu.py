"""Unlikelihood training inside the training step (mtn_amd.train_step.TrainStep(unlikelihood=...)) on the small configurations of
tests/test_distill_step_gpu.py, with its helpers and its bars:
  (a) unlikelihood = 0 leaves the captured step what it was, bit for bit, and the launch census equal;
  (b) unlikelihood = 1 in float32: loss, last_ul and every parameter gradient against the CPU oracle (oracle forward, the composed loss of
      tests/unlikelihood_refs.py's definition — python sets, torch.clamp — and autograd), at the bars
      test_distilled_loss_and_gradients_match_the_oracle holds its step to;
  (c) eager and captured steps give the same loss bits;
  (d) the conflicts raise, naming what conflicts;
  (e) train.py --unlikelihood-alpha 1 logs the epoch line with a finite value: the fixed synthetic batch, and the synthetic corpus
      graphed and --eager."""
import contextlib
import io
import math
import re

import pytest
import torch

from oracle import fixtures as fx
from tests import unlikelihood_refs as ur
from tests.step_helpers import _census, _student, deterministic_embed  # noqa: F401  (fixture)
from tests.test_distill_step_gpu import NAMES, _config, _teacher
from tests.test_model_gpu import dev_batch, raw_batch
from tests.util import TOL, relmax

pytestmark = pytest.mark.gpu
UL_LINE = re.compile(r"^epoch (\d+) mean unlikelihood per token: (\S+)$", re.M)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------ (a)
@pytest.mark.parametrize("name", NAMES)
def test_alpha_zero_leaves_the_step_bitwise(dev, name, deterministic_embed):
    from mtn_amd.train_step import TrainStep
    c = _config(name)
    b = dev_batch(raw_batch(c), dev)

    def run(**kw):
        model = _student(c, torch.bfloat16, dev, 0.1)
        ts = TrainStep(model, b, c["vocab"], pad=fx.PAD, warmup=10, **kw)
        losses = [ts().clone() for _ in range(3)]
        torch.cuda.synchronize()
        return losses, model._flat.clone(), ts

    plain_l, plain_p, _ = run()
    zero_l, zero_p, ts = run(unlikelihood=0.0)
    for a, d in zip(plain_l, zero_l):
        assert torch.equal(a.view(torch.int32), d.view(torch.int32)), (float(a), float(d))
    assert torch.equal(plain_p.view(torch.int32), zero_p.view(torch.int32))
    assert plain_l[0].item() != plain_l[2].item()                        # the steps did train
    assert ts.last_ul is None
    ul_l, _, ts = run(unlikelihood=1.0)                                  # and the flag does change the step
    assert float(ul_l[0]) > float(plain_l[0]) and float(ts.last_ul) > 0

    def eager(**kw):
        model = _student(c, torch.bfloat16, dev, 0.1)
        ts = TrainStep(model, b, c["vocab"], pad=fx.PAD, warmup=10, use_graph=False, **kw)
        step = ts._step_fused if ts._fused() else ts._fwd_bwd
        step()                                                           # (lazy set-up outside the census)
        return _census(step)

    plain_c, plain_f = eager()
    assert len(plain_c) > 0
    assert eager(unlikelihood=0.0) == (plain_c, plain_f)
    assert eager(unlikelihood=1.0) == (plain_c, plain_f)                 # casts and GEMMs unchanged: only the two row kernels differ


# ------------------------------------------------------------------------------------------ (b)
def _oracle_reference(c, raw, alpha):
    """(loss, {parameter name: gradient}, ul per token) of the unlikelihood loss on the CPU oracle."""
    ob = fx.oracle_batch(raw)
    student, _ = fx.oracle_from_config(c, seed=0, requires_grad=True)
    out, ae = student.forward(ob)
    logp = student.generator(out)
    norm = ob.ntokens.float()
    ul = ur.ul_rows_of_logp(logp.reshape(ob.trg_y.size(0), ob.trg_y.size(1), -1), ob.trg_y, fx.PAD).sum()
    total = student.loss(ob, out, ae) + alpha * ul / norm
    total.backward()
    return float(total.detach()), {k: v.grad for k, v in student.p.items() if v.grad is not None}, float(ul.detach() / norm)


@pytest.mark.parametrize("name", NAMES)
def test_unlikelihood_loss_and_gradients_match_the_oracle(dev, name):
    from mtn_amd.train_step import TrainStep
    dtype, alpha = torch.float32, 1.0
    c = _config(name)
    raw = raw_batch(c)
    ref_loss, ref_grads, ref_ul = _oracle_reference(c, raw, alpha)
    model = _student(c, dtype, dev, 0.0)
    ts = TrainStep(model, dev_batch(raw, dev), c["vocab"], pad=fx.PAD, warmup=10, use_graph=False, fuse_optimizer=False, unlikelihood=alpha)
    out, ae_out = model.forward(ts.batch)                               # the loss is the fused HIP head's, not the composed fallback's
    probe = ts._loss_of(out, ae_out, None)
    assert probe.grad_fn is not None and "GeneratorLossFn" in type(probe.grad_fn).__name__
    del probe, out, ae_out
    loss = ts._fwd_bwd()
    torch.cuda.synchronize()
    tol = TOL[dtype]
    print(f"{name} {dtype}: loss {float(loss):.6f} (oracle {ref_loss:.6f})  ul/token {float(ts.last_ul):.6f} (oracle {ref_ul:.6f})")
    assert abs(float(loss) - ref_loss) < tol * max(1.0, abs(ref_loss))
    assert abs(float(ts.last_ul) - ref_ul) < tol * max(1.0, abs(ref_ul))
    assert ref_ul > 1e-3                                                # the batch does hold earlier targets to be unlikely
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
def test_eager_and_captured_steps_give_the_same_loss_bits(dev, deterministic_embed):
    from mtn_amd.train_step import TrainStep
    c = _config("small_shared")
    b = dev_batch(raw_batch(c), dev)
    runs = []
    for use_graph in (False, True):
        model = _student(c, torch.bfloat16, dev, 0.0)
        ts = TrainStep(model, b, c["vocab"], pad=fx.PAD, warmup=10, use_graph=use_graph, unlikelihood=1.0)
        runs.append([(ts().clone(), ts.last_ul.clone()) for _ in range(3)])
    torch.cuda.synchronize()
    for (le, ue), (lg, ug) in zip(*runs):
        assert torch.equal(le.view(torch.int32), lg.view(torch.int32)), (float(le), float(lg))
        assert torch.equal(ue.view(torch.int32), ug.view(torch.int32))
    assert float(runs[0][0][1]) > 0 and float(runs[0][2][0]) != float(runs[0][0][0])


# ------------------------------------------------------------------------------------------ (d)
def test_conflicts_raise_and_name_what_conflicts(dev):
    from mtn_amd import ops
    from mtn_amd.train_step import BucketedTrainer, ScstConfig, TrainStep
    c = _config("cfg1_query")
    b = dev_batch(raw_batch(c), dev)
    model = _student(c, torch.bfloat16, dev, 0.0)
    teacher = _teacher(c, torch.bfloat16, dev, 1)
    scst = ScstConfig.__new__(ScstConfig)                                # (never looked at: the conflict is refused first)
    for cls, args in ((TrainStep, (model, b, c["vocab"])), (BucketedTrainer, (model, None, c["vocab"]))):
        with pytest.raises(ValueError, match="teacher"):
            cls(*args, pad=fx.PAD, teacher=teacher, unlikelihood=1.0)
        with pytest.raises(ValueError, match="scst"):
            cls(*args, pad=fx.PAD, scst=scst, unlikelihood=1.0)
        for bad in (-1.0, float("nan"), float("inf")):
            with pytest.raises(ValueError, match="finite"):
                cls(*args, pad=fx.PAD, unlikelihood=bad)
    # the autograd function itself: a teacher or row weights next to spec["unlikelihood"]
    ts = TrainStep(model, b, c["vocab"], pad=fx.PAD, warmup=10, use_graph=False, unlikelihood=1.0)
    out, ae_out = model.forward(ts.batch)
    rows, V = ts.batch.trg_y.numel(), c["vocab"]
    with pytest.raises(ValueError, match="unlikelihood does not combine with teacher"):
        ts.lc._fused_loss(out, ts.batch.trg_y, ts._norms[0], None, None, None, teacher_logp=torch.zeros(rows, V, device=dev), alpha=0.5,
                          unlikelihood=1.0)
    with pytest.raises(ValueError, match="unlikelihood does not combine with row weights"):
        ts.lc._fused_loss(out, ts.batch.trg_y, ts._norms[0], None, None, None, row_weights=torch.ones(rows, device=dev), unlikelihood=1.0)
    assert "unlikelihood" in ops.LOSS_HEADS


# ------------------------------------------------------------------------------------------ (e)
SMALL = ["--nb-blocks", "1", "--d-model", "64", "--d-ff", "128", "--att-h", "4", "--vocab-size", "64", "--ft-sizes", "16", "8",
         "--warmup-steps", "20", "--report-interval", "1000", "--dropout", "0.0", "--batch-size", "8"]
CORPUS = SMALL + ["--corpus-videos", "3", "--valid-videos", "1", "--max-length", "12", "--corpus-max-answer", "8", "--corpus-max-question", "8"]


def _run(argv):
    from mtn_amd import train
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        train.main(argv)
    return buf.getvalue()


def _ul_values(out, epochs):
    rows = UL_LINE.findall(out)
    assert [int(r[0]) for r in rows] == list(range(1, epochs + 1)), out
    vals = [float(r[1]) for r in rows]
    assert all(math.isfinite(v) and v > 0.0 for v in vals), vals
    return vals


def test_train_py_logs_the_epoch_line_on_the_fixed_batch(dev):
    out = _run(SMALL + ["--lens", "6", "12", "8", "7", "4", "--unlikelihood-alpha", "1", "--steps-per-epoch", "3", "--num-epochs", "2"])
    _ul_values(out, 2)
    assert "unlikelihood" not in _run(SMALL + ["--lens", "6", "12", "8", "7", "4", "--steps-per-epoch", "3"])


@pytest.mark.parametrize("eager", [False, True], ids=["graphed", "eager"])
def test_train_py_logs_the_epoch_line_on_the_synthetic_corpus(dev, eager):
    out = _run(CORPUS + ["--unlikelihood-alpha", "1"] + (["--eager"] if eager else []))
    _ul_values(out, 1)
    assert "validation loss" in out                                     # validation stays the plain loss
