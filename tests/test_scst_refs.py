"""tests/scst_refs.py checks itself without a GPU: the weighted loss head reduces to the loss-head reference, its closed-form gradient is
the autograd gradient, the cut rule is sample_decode_many's, equal rewards leave no advantage, and the fixed-corpus rewards are
eval_refs.evaluate's when the hypotheses are the corpus' own items."""
import numpy as np
import pytest
import torch

from tests import eval_refs as er
from tests import row_refs as rr
from tests import scst_refs as sr


@pytest.mark.parametrize("idx", [0, 3, 11, 14, 21, 29, 30])
def test_weights_of_one_reduce_to_the_loss_head_reference(idx):
    c = rr.loss_cases()[idx]
    z, targets = rr.loss_inputs(c, rr.LOSS_SEED + idx)
    ref = rr.composed_loss(z, targets, c)
    n = len(c.segs)
    for weights in ([None] * n, [np.ones(m) for m in c.segs]):
        got = sr.weighted_loss_head(z.numpy(), [t.numpy() for t in targets], weights, [c.smoothing] * n, c.V, c.pad, rr.COEF, rr.NORM, rr.GLOSS)
        assert np.abs(got["lse"] - ref["lse"].numpy()).max() <= 1e-12 * 100
        assert np.abs(got["rowloss"] - ref["rowloss"].numpy()).max() <= 1e-12 * max(1.0, float(ref["rowloss"].abs().max()))
        assert np.abs(got["dlogits"] - ref["dlogits"].numpy()).max() <= 1e-12 * max(1.0, float(ref["dlogits"].abs().max()))
        assert (got["zero"] == ref["zero"].numpy()).all()
        assert abs(got["total"] - ref["total"]) <= 1e-11 * max(1.0, abs(ref["total"]))


@pytest.mark.parametrize("V", [64, 104])
@pytest.mark.parametrize("sm", [(0.0, 0.0, 0.0), (0.1, 0.1, 0.1), (0.0, 0.1, 0.1)])
def test_weighted_gradient_is_autograd_of_the_weighted_sum(V, sm):
    """The closed form against autograd on sum_rows scale w KL_ls built from torch ops in float64; zero weights and zeroed rows hold 0."""
    z, targets, weights = sr.head_inputs(V, 5)
    got = sr.weighted_loss_head(z, targets, weights, sm, V, sr.PAD, sr.COEF, sr.NORM, sr.GLOSS)
    zt = torch.from_numpy(z).double().requires_grad_()
    logp = torch.log_softmax(zt, dim=1)
    total, base = 0.0, 0
    for s, t in enumerate(targets):
        td = torch.from_numpy(sr.smoothed_targets(t, V, sr.PAD, sm[s]))
        kl = (td * (torch.where(td > 0, td, torch.ones_like(td)).log() - logp[base:base + t.size])).sum(1)
        total = total + (torch.from_numpy(weights[s]).double() * kl).sum() * (sr.COEF[s] / sr.NORM[s])
        base += t.size
    (g,) = torch.autograd.grad(total, zt)
    total = float(total.detach())
    assert abs(got["total"] - total) <= 1e-12 * max(1.0, abs(total))
    assert np.abs(got["dlogits"] - sr.GLOSS * g.numpy()).max() <= 1e-13
    assert (got["rowloss"][got["zero"]] == 0).all() and (got["dlogits"][got["zero"]] == 0).all()
    assert got["zero"].tolist() == [False, True, True, False, True, False, False, False, True, True, False, False, False]
    if sm[1] == 0.0:                                      # the quirk row with smoothing 0: an all-zero target row, no loss
        assert got["rowloss"][5] == 0
    else:
        assert got["rowloss"][5] != 0                     # a live quirk row (its td sums to less than 1: the sign is the logits')
    assert got["rowloss"][0] < 0 < got["rowloss"][3]


def test_smoothing_zero_is_minus_log_p_of_the_target():
    V = 64
    z, targets, weights = sr.head_inputs(V, 6)
    got = sr.weighted_loss_head(z, targets, weights, (0.0, 0.0, 0.0), V, sr.PAD, sr.COEF, sr.NORM, sr.GLOSS)
    logp = torch.log_softmax(torch.from_numpy(z).double(), dim=1).numpy()
    t = np.concatenate(targets)
    live = t != sr.PAD
    assert np.abs(got["kl"][live] + logp[np.arange(t.size), t][live]).max() <= 1e-13


def test_cut_rule_on_every_case():
    eos, L = 2, 5
    log = sr.assemble_log(eos, L)
    assert [sr.cut_length(log[:, r], eos) for r in range(6)] == [0, L - 1, L - 1, 2, 1, 1]
    trg, trg_y, hyp, hyp_len = sr.assemble(log, sos=0, eos=eos, pad=1, T=7)
    assert hyp_len.tolist() == [0, 4, 4, 2, 1, 1]
    assert trg[0].tolist() == [0, 1, 1, 1, 1, 1, 1] and trg_y[0].tolist() == [2, 1, 1, 1, 1, 1, 1]          # <eos> at position 0
    assert trg[1].tolist() == [0, 4, 5, 6, 7, 1, 1] and trg_y[1].tolist() == [4, 5, 6, 7, 2, 1, 1]          # <eos> at position L - 1
    assert trg[2].tolist() == [0, 4, 5, 6, 7, 1, 1] and trg_y[2].tolist() == [4, 5, 6, 7, 2, 1, 1]          # none: L - 1 tokens kept
    assert trg[4].tolist() == [0, 3, 1, 1, 1, 1, 1] and trg_y[4].tolist() == [3, 2, 1, 1, 1, 1, 1]          # the first <eos> counts
    assert hyp[3].tolist() == [9, 8, 1, 1, 1] and hyp[0].tolist() == [1] * 5
    # the same rule as decode.sample_decode_many states it
    for r in range(6):
        col = [int(t) for t in log[:, r]]
        n = col.index(eos) if eos in col else len(col) - 1
        assert hyp_len[r] == n and hyp[r, :n].tolist() == col[:n]
    a, b, _, _ = sr.assemble(log, 0, eos, 1)                                                                # T = L still holds every row
    assert a.shape == (6, L) and (a == trg[:, :L]).all() and (b == trg_y[:, :L]).all()


@pytest.mark.parametrize("S", [2, 3, 4, 5])
def test_equal_rewards_leave_no_advantage(S):
    reward = np.array([[0.75] * S, [1.25, 0.5, 2.0, 0.125, 1.0][:S], [0.0] * S])
    out = sr.advantage(reward, T=3)
    assert (out["adv"][0] == 0).all() and (out["adv"][2] == 0).all() and (out["roww"][:S] == 0).all()
    assert out["roww"].shape == (3 * S, 3) and out["roww"].dtype == np.float32
    assert abs(out["adv"][1].sum()) <= 1e-15                         # leave-one-out advantages of a dialogue sum to 0
    assert abs(out["mean_baseline"] - out["mean_reward"]) <= 1e-15   # and the mean baseline is the mean reward
    if S == 2:
        assert out["base"][1].tolist() == [0.5, 1.25]
    given = sr.advantage(reward, T=2, baseline=[0.75, 1.0, -1.0])
    assert (given["adv"][0] == 0).all() and given["adv"][2].tolist() == [1.0] * S and (given["roww"][-1] == -1.0).all()
    assert given["mean_baseline"] == pytest.approx(0.25)


def test_rewards_of_the_corpus_own_items_are_evaluate():
    hyps, ref_sets = er.random_corpus(4, 9, 1, 10, 5, refs=(1, 3))
    ev = er.evaluate(hyps, ref_sets)
    got = sr.rewards(hyps, list(range(9)), ref_sets)
    assert (got["stats"] == ev["stats"]).all() and (got["rouge"] == ev["rouge"]).all() and (got["cider"] == ev["cider"]).all()
    perm = [4, 4, 0, 8, 2]
    sub = sr.rewards([hyps[i] for i in perm], perm, ref_sets)
    assert (sub["cider"] == ev["cider"][perm]).all() and (sub["stats"] == ev["stats"][perm]).all()


def test_reward_corpus_covers_the_stated_lengths():
    ref_sets, hyps, items = sr.reward_corpus()
    assert len(ref_sets) == 7 and all(1 <= len(r) <= 3 for r in ref_sets) and max(len(s) for r in ref_sets for s in r) == 12
    assert len(hyps) == 10 and {0, 1, 3, 12} <= {len(h) for h in hyps}
    assert len(set(items)) < len(items) and items != sorted(items)
    ref, ref_len, n_ref = sr.pack_corpus(ref_sets, 3, 12)
    assert ref.shape == (7, 3, 12) and int(n_ref.max()) == 3 and int(ref_len.max()) == 12


def test_composed_fallback_of_simple_loss_compute_matches_the_definition():
    """SimpleLossCompute.loss(..., row_weights=, smoothing=) on CPU tensors (the composed PyTorch form) is the numpy definition on the
    generator's logits, value and gradient; without either it is the plain loss, and with weights of one at the criterion's smoothing too."""
    from mtn_amd.data_utils import LabelSmoothing, SimpleLossCompute
    from mtn_amd.mtn import Generator
    torch.manual_seed(5)
    V, d, n = 104, 16, 9
    gen = Generator(d, V).double()
    x = torch.randn(n, d, dtype=torch.float64, requires_grad=True)
    y = torch.randint(2, V, (n,))
    y[4] = y[8] = 1
    w = torch.tensor([-1.5, 0.0, 1.0, 0.25, -2.0, 1.0, -0.3, 2.5, 1.0])
    norm = torch.tensor(7.0)
    lc = SimpleLossCompute(gen, None, LabelSmoothing(V, 1, 0.1), opt=None, sync=False)
    z = gen.proj(x).detach().numpy()
    for sm in (0.0, 0.1):
        loss = lc.loss(x, y, norm, row_weights=w, smoothing=sm)
        (gx,) = torch.autograd.grad(loss, x)
        ref = sr.weighted_loss_head(z, [y.numpy()], [w.numpy()], [sm], V, 1, [1.0], [7.0], 1.0)
        assert abs(float(loss.detach()) - ref["total"]) <= 1e-12 * max(1.0, abs(ref["total"]))
        assert float((torch.from_numpy(ref["dlogits"]) @ gen.proj.weight.detach() - gx).abs().max()) <= 1e-12 * float(gx.abs().max())
    plain = float(lc.loss(x, y, norm).detach())
    assert abs(float(lc.loss(x, y, norm, row_weights=torch.ones(n)).detach()) - plain) <= 1e-12 * abs(plain)
    assert abs(float(lc.loss(x, y, norm, smoothing=0.1).detach()) - plain) <= 1e-12 * abs(plain)
    with pytest.raises(ValueError):
        lc.loss(x, y, norm, row_weights=w, teacher_logp=torch.randn(n, V))
    with pytest.raises(ValueError):
        lc.loss(x, y, norm, row_weights=w[:3])
    with pytest.raises(ValueError):
        lc.loss(x, y, norm, smoothing=1.5)
