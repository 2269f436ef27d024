"""Self-critical sequence training inside the training step (mtn_amd.train_step.TrainStep(scst=ScstConfig)) on the small configurations
of tests/test_model_gpu.py, with its helpers and its bars:
  (a) gold targets fed as the "samples" with weight 1 (smoothing 0 everywhere): loss and updated flat weights are those of a plain
      TrainStep(smoothing=0) on the replicated batch, bit for bit;
  (b) fixed rows with signed weights: loss and every parameter gradient against the CPU oracle with autograd on sum w (-log p) / norm, at
      the bars test_model_loss_and_grads_match_reference_golden holds its gradients to;
  (c) eager and captured steps give the same loss bits, two runs from one seed the same weights — with fixed rows and with drawn ones;
  (d) the weighted step's launch census is the plain step's on the replicated batch (a step without scst runs no new code);
  (e) rl_step draws, scores and trains: finite rewards, the gold rows ride along, the greedy baseline is one value per dialogue."""

import numpy as np
import pytest
import torch

from oracle import fixtures as fx
from oracle.mtn_oracle import label_smoothing_kl
from tests.step_helpers import _census, _student, deterministic_embed  # noqa: F401  (fixture)
from tests.test_model_gpu import dev_batch, raw_batch
from tests.util import DTYPES, TOL, relmax

pytestmark = pytest.mark.gpu
NAMES = ["small_shared", "cfg1_query"]
S = 2
SOS, EOS = 2, 3


def _config(name):
    """The golden configuration with its vocabulary rounded up to a multiple of 8, as tests/test_distill_step_gpu.py: what the fused HIP
    loss head takes."""
    c = fx.GOLDEN_CONFIGS[name]
    return dict(c, vocab=-(-c["vocab"] // 8) * 8)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


def _replicated(raw, times):
    """The raw batch with every dialogue ``times`` times in a row (row d * times + s), as the step's static batch holds it."""
    out = dict(raw)
    for k in ("query", "his", "cap", "trg", "trg_y"):
        out[k] = np.repeat(raw[k], times, axis=0)
    out["fts"] = [np.repeat(f, times, axis=0) for f in raw["fts"]]
    return out


def _cfg(c, **kw):
    from mtn_amd.train_step import ScstConfig
    return ScstConfig(samples=S, max_length=c["T"], sos=SOS, eos=EOS, **kw)


# ------------------------------------------------------------------------------------------ (a)
@pytest.mark.parametrize("name", NAMES)
def test_gold_rows_at_weight_one_are_the_plain_step_bitwise(dev, name, deterministic_embed):
    from mtn_amd.train_step import TrainStep
    c = _config(name)
    raw = raw_batch(c)
    rep = dev_batch(_replicated(raw, S), dev)

    def plain():
        model = _student(c, torch.bfloat16, dev, 0.1)
        ts = TrainStep(model, rep, c["vocab"], pad=fx.PAD, warmup=10, smoothing=0.0)
        losses = [ts().clone() for _ in range(3)]
        torch.cuda.synchronize()
        return losses, model._flat.clone()

    def scst():
        model = _student(c, torch.bfloat16, dev, 0.1)
        ts = TrainStep(model, dev_batch(raw, dev), c["vocab"], pad=fx.PAD, warmup=10, smoothing=0.0, scst=_cfg(c))
        ts.load_rows(rep.trg, rep.trg_y, torch.ones(rep.trg.size(0)))
        losses = [ts().clone() for _ in range(3)]
        torch.cuda.synchronize()
        return losses, model._flat.clone(), ts

    plain_l, plain_p = plain()
    scst_l, scst_p, ts = scst()
    assert ts.batch.trg.shape == rep.trg.shape and torch.equal(ts.batch.query, rep.query) and torch.equal(ts.batch.trg_mask, rep.trg_mask)
    for a, b in zip(plain_l, scst_l):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (float(a), float(b))
    assert torch.equal(plain_p.view(torch.int32), scst_p.view(torch.int32))
    assert plain_l[0].item() != plain_l[2].item()                        # the steps did train


# ------------------------------------------------------------------------------------------ (b)
def _fixed_rows(c, n, seed):
    """(trg, trg_y int64 (n, T), weights (n,)): responses of 0..T-1 tokens over the ids >= 4, signed weights with a zero among them."""
    g = torch.Generator().manual_seed(seed)
    T = c["T"]
    trg = torch.full((n, T), fx.PAD, dtype=torch.long)
    trg_y = torch.full((n, T), fx.PAD, dtype=torch.long)
    for r in range(n):
        k = [T - 1, 0, 3, 1][r % 4] if r < 4 else int(torch.randint(0, T, (1,), generator=g))
        k = min(k, T - 1)
        y = torch.randint(4, c["vocab"], (k,), generator=g)
        trg[r, 0], trg[r, 1:k + 1] = SOS, y
        trg_y[r, :k], trg_y[r, k] = y, EOS
    w = torch.randn(n, generator=g)
    w[1 % n] = 0.0
    w[0] = -abs(w[0])
    return trg, trg_y, w


def _oracle_reference(c, raw_rep, trg, trg_y, w):
    """(loss, {parameter name: gradient}) of sum_rows w (-log p(target)) / norm + the plain auto-encoder loss on the CPU oracle."""
    raw = dict(raw_rep, trg=trg.numpy(), trg_y=trg_y.numpy())
    ob = fx.oracle_batch(raw)
    student, _ = fx.oracle_from_config(c, seed=0, requires_grad=True)
    out, ae = student.forward(ob)
    V = c["vocab"]
    logp = student.generator(out).reshape(-1, V)
    y = ob.trg_y.reshape(-1)
    norm = ob.ntokens.float()
    plain = student.loss(ob, out, ae)
    hard = label_smoothing_kl(logp, y, fx.PAD, 0.1) / norm
    nll = -logp.gather(1, y.unsqueeze(1)).squeeze(1)
    wrow = w.to(logp.dtype).unsqueeze(1).expand(-1, trg_y.size(1)).reshape(-1)
    weighted = torch.where(y != fx.PAD, wrow * nll, torch.zeros_like(nll)).sum() / norm
    total = plain - hard + weighted
    total.backward()
    return float(total.detach()), {k: v.grad for k, v in student.p.items() if v.grad is not None}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", NAMES)
def test_signed_rows_match_the_oracle(dev, name, dtype):
    from mtn_amd.train_step import TrainStep
    c = _config(name)
    raw = raw_batch(c)
    n = c["B"] * S
    trg, trg_y, w = _fixed_rows(c, n, 17)
    ref_loss, ref_grads = _oracle_reference(c, _replicated(raw, S), trg, trg_y, w)
    model = _student(c, dtype, dev, 0.0)
    ts = TrainStep(model, dev_batch(raw, dev), c["vocab"], pad=fx.PAD, warmup=10, use_graph=False, fuse_optimizer=False, scst=_cfg(c))
    ts.load_rows(trg.to(dev), trg_y.to(dev), w)
    out, ae_out = model.forward(ts.batch)                               # the loss is the fused HIP head's, not the composed fallback's
    ts._refresh_norms()
    probe = ts._loss_of(out, ae_out, None)
    assert probe.grad_fn is not None and "GeneratorLossFn" in type(probe.grad_fn).__name__
    del probe, out, ae_out
    loss = ts._fwd_bwd()
    torch.cuda.synchronize()
    tol = TOL[dtype]
    print(f"{name} {dtype}: loss {float(loss):.6f} (oracle {ref_loss:.6f})")
    assert abs(float(loss) - ref_loss) < tol * max(1.0, abs(ref_loss))
    gtol = 3e-3 if dtype == torch.float32 else 0.25                     # test_model_loss_and_grads_match_reference_golden's bars
    params = dict(model.named_parameters())
    worst, dot, n1, n2, checked = 0.0, 0.0, 0.0, 0.0, 0
    for k, ref in ref_grads.items():
        if k not in params:
            continue
        gr = params[k].grad
        assert gr is not None, k
        nr, gn = float(ref.double().norm()), float(gr.double().norm())
        if nr < 1e-6:
            assert gn < (1e-5 if dtype == torch.float32 else 1e-3), (k, gn)
            continue
        e = max(relmax(gr, ref), abs(gn - nr) / nr)
        dot += float((gr.double().cpu() * ref.double()).sum()); n1 += gn * gn; n2 += nr * nr
        worst = max(worst, e)
        checked += 1
        assert e < gtol, (k, e)
    cos = dot / (n1 ** 0.5 * n2 ** 0.5)
    print(f"worst grad rel err {worst:.2e} over {checked} tensors, cosine {cos:.7f}")
    assert checked > 20
    assert cos > (0.999999 if dtype == torch.float32 else 0.9995), cos


# ------------------------------------------------------------------------------------------ (c), (e)
def _corpus(c, dev, n_items, seed=3):
    """A reference corpus of n_items items of 1..2 references over the ids >= 4, rows of max_length tokens: (ref, ref_len, n_ref)."""
    rng = np.random.RandomState(seed)
    T = c["T"]
    ref = np.full((n_items, 2, T), fx.PAD, dtype=np.int32)
    ref_len = np.zeros((n_items, 2), dtype=np.int32)
    n_ref = np.zeros(n_items, dtype=np.int32)
    for q in range(n_items):
        n_ref[q] = 1 + q % 2
        for r in range(n_ref[q]):
            k = rng.randint(2, T)
            ref[q, r, :k] = rng.randint(4, 12, k)
            ref_len[q, r] = k
    return tuple(torch.from_numpy(a).to(dev) for a in (ref, ref_len, n_ref))


@pytest.mark.parametrize("name", NAMES)
def test_eager_and_captured_steps_agree_and_runs_repeat(dev, name, deterministic_embed):
    from mtn_amd.train_step import TrainStep
    c = _config(name)
    raw = raw_batch(c)
    n = c["B"] * S
    trg, trg_y, w = _fixed_rows(c, n, 23)
    refs = _corpus(c, dev, 5)
    items = [i % 5 for i in range(c["B"])]

    def run(use_graph, drawn):
        model = _student(c, torch.bfloat16, dev, 0.0)                  # (capture's warm-up passes advance the dropout stream)
        ts = TrainStep(model, dev_batch(raw, dev), c["vocab"], pad=fx.PAD, warmup=10, use_graph=use_graph, scst=_cfg(c, refs=refs, seed=5))
        if drawn:
            losses = [ts.rl_step(items).clone() for _ in range(2)]
        else:
            ts.load_rows(trg.to(dev), trg_y.to(dev), w)
            losses = [ts().clone() for _ in range(2)]
        torch.cuda.synchronize()
        return losses, model._flat.clone(), ts

    for drawn in (False, True):
        cap_l, cap_p, ts = run(True, drawn)
        again_l, again_p, _ = run(True, drawn)
        eager_l, _, _ = run(False, drawn)
        for a, b, e in zip(cap_l, again_l, eager_l):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(a.view(torch.int32), e.view(torch.int32)), (drawn, float(a), float(e))
            assert bool(torch.isfinite(a))
        assert torch.equal(cap_p.view(torch.int32), again_p.view(torch.int32))
        if drawn:
            assert bool(torch.isfinite(ts.last_reward)) and bool(torch.isfinite(ts.last_baseline)) and float(ts.last_reward) >= 0.0
            assert ts.last_reward.dtype == torch.float64 and ts.last_reward.is_cuda
            y = ts.batch.trg_y
            assert bool((y[:, 0] != fx.PAD).all()) and bool(((y == EOS).sum(1) == 1).all())         # every drawn row ends in one <eos>
            assert float(ts._norms[0]) == float((y != fx.PAD).sum())


def test_gold_rows_and_greedy_baseline(dev):
    """xe_weight adds B gold rows of constant weight behind the B * S drawn ones (the normaliser still counts the drawn targets alone);
    the greedy baseline gives every sample of a dialogue the same baseline, so its weights differ from the rewards by a constant."""
    from mtn_amd.train_step import TrainStep
    c = _config("small_shared")
    raw = raw_batch(c)
    B, T = c["B"], c["T"]
    refs = _corpus(c, dev, 4)
    model = _student(c, torch.bfloat16, dev, 0.0)
    src = dev_batch(raw, dev)
    ts = TrainStep(model, src, c["vocab"], pad=fx.PAD, warmup=10, scst=_cfg(c, refs=refs, baseline="greedy", xe_weight=0.5, reward="rouge"))
    p0 = model._flat.clone()
    loss = ts.rl_step([i % 4 for i in range(B)])
    torch.cuda.synchronize()
    n = B * S
    assert ts.batch.trg.shape == (n + B, T) and torch.equal(ts.batch.trg_y[n:, :src.trg_y.size(1)], src.trg_y)
    assert bool((ts._roww[n:] == 0.5).all()) and bool(torch.isfinite(loss)) and not torch.equal(p0, model._flat)
    assert float(ts._norms[0]) == float((ts.batch.trg_y[:n] != fx.PAD).sum())
    w = ts._roww[:n].view(B, S, T)
    assert bool((w == w[:, :, :1]).all())                                                         # one weight per row
    assert 0.0 <= float(ts.last_reward) <= 1.0 and 0.0 <= float(ts.last_baseline) <= 1.0           # ROUGE-L lies in [0, 1]


# ------------------------------------------------------------------------------------------ (d)
@pytest.mark.parametrize("name", NAMES)
def test_weighted_step_has_the_plain_steps_launch_census(dev, name, deterministic_embed):
    from mtn_amd.train_step import TrainStep
    c = _config(name)
    b = dev_batch(raw_batch(c), dev)

    # the weighted step's census is the plain step's on the replicated batch: one row kernel in the place of another, nothing else
    # added to or taken from the step (scst=None is the constructor's default: a TrainStep without it runs the code it ran)
    rep = dev_batch(_replicated(raw_batch(c), S), dev)
    model = _student(c, torch.bfloat16, dev, 0.1)
    ts = TrainStep(model, rep, c["vocab"], pad=fx.PAD, warmup=10, use_graph=False, dynamic_norms=True)
    step = ts._step_fused if ts._fused() else ts._fwd_bwd
    step()
    plain_c = _census(step)
    model = _student(c, torch.bfloat16, dev, 0.1)
    ts = TrainStep(model, b, c["vocab"], pad=fx.PAD, warmup=10, use_graph=False, scst=_cfg(c))
    ts.load_rows(rep.trg, rep.trg_y, torch.ones(rep.trg.size(0)))
    step = ts._step_fused if ts._fused() else ts._fwd_bwd
    step()
    assert _census(step) == plain_c
