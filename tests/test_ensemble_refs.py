"""The float64 reference of tests/test_ensemble_kernel_gpu.py (tests/ensemble_refs.py) checked without a GPU against the definitions computed
another way: prob against log(sum_m w_m softmax(x_m)), logprob rows against logsumexp = 0 and against the directly renormalised weighted sum,
M = 1 and identical members against log_softmax, invariance under a permutation of the members, the exact -inf pattern, what the case list
holds, and the recorded float32 yardstick the GPU bound is a multiple of."""
import numpy as np
import pytest
import torch

from tests import ensemble_refs as er

CASES = er.ens_cases()
IDS = [er.ens_case_id(c) for c in CASES]


def _log_softmax64(x):
    return torch.log_softmax(torch.from_numpy(np.ascontiguousarray(x)), dim=-1).numpy()


def _close(a, b, tol=1e-9):
    fin = np.isfinite(b)
    assert np.array_equal(np.isneginf(a), np.isneginf(b)) and not np.isnan(a).any() and not np.isnan(b).any()
    assert not fin.any() or float(np.abs(a[fin] - b[fin]).max()) <= tol * max(1.0, float(np.abs(b[fin]).max()))


def test_case_list_covers_what_the_issue_names():
    assert {c.rows for c in CASES} == {1, 5, 16}
    assert {c.M for c in CASES} == {1, 2, 3, 8}
    assert {c.V for c in CASES} == {1, 3, 255, 257, 1000, 4099}
    assert any(c.V == 1000 and 1003 in c.lds for c in CASES)                       # rows that are not 16-byte aligned
    assert any(len(set(c.lds)) > 1 for c in CASES)                                 # members with different row strides
    assert {c.weights for c in CASES} == {"uniform", "skewed", "zero"}
    assert {c.inputs for c in CASES} == {"logits", "logp", "identical", "neginf", "zero_inf"}
    assert all(len(c.lds) == c.M and min(c.lds) >= c.V for c in CASES)
    for c in CASES:
        w = er.ens_weights(c)
        assert abs(w.sum() - 1.0) < 1e-15 and (w >= 0).all()
        if c.weights == "zero":
            assert w[1] == 0.0 and c.M >= 2
        if c.weights == "skewed" and c.M == 2:
            assert np.allclose(w, [0.9, 0.1])


@pytest.mark.parametrize("idx", range(len(CASES)), ids=IDS)
def test_reference_matches_the_definitions(idx):
    c = CASES[idx]
    bufs, xs, w = er.case_views(c, er.ENS_SEED + idx)
    for b in bufs:
        assert bool(torch.isnan(b[:, c.V:]).all()) and not bool(torch.isnan(b[:, :c.V]).any())
    keep = [m for m in range(c.M) if w[m] > 0]
    for m in keep:
        assert np.isfinite(xs[m]).any(axis=1).all()                                 # the precondition
    prob, logprob = er.ensemble_ref64(xs, w, "prob"), er.ensemble_ref64(xs, w, "logprob")
    # prob = log of the weighted mean of the softmaxes
    with np.errstate(divide="ignore"):
        mean = sum(w[m] * np.exp(_log_softmax64(xs[m])) for m in keep)
        direct = np.log(mean)
    tiny = mean < 1e-290                                                            # (exp underflows there; the stable form does not)
    _close(np.where(tiny, 0.0, prob), np.where(tiny, 0.0, direct))
    assert abs(np.exp(prob).sum(1) - 1.0).max() < 1e-12                             # already normalised
    # logprob = the weighted sum of log_softmax rows, renormalised: its rows have logsumexp 0
    s = sum(w[m] * _log_softmax64(xs[m]) for m in keep)
    _close(logprob, _log_softmax64(s))
    assert abs(torch.logsumexp(torch.from_numpy(logprob), 1).numpy()).max() < 1e-12
    # the -inf pattern, exactly
    ninf = np.stack([np.isneginf(xs[m]) for m in keep])
    assert np.array_equal(np.isneginf(prob), ninf.all(0)) and np.array_equal(np.isneginf(logprob), ninf.any(0))
    if c.inputs == "neginf" and c.V >= 3:
        assert np.isneginf(prob).any() and (np.isneginf(logprob).sum() > np.isneginf(prob).sum() or c.M == 1)
    if c.inputs == "zero_inf":
        assert np.isneginf(xs[1]).any() and not np.isneginf(prob).any() and not np.isneginf(logprob).any()
    # M = 1, or members that are all the same rows: log_softmax of that row
    if len(keep) == 1 or all(np.array_equal(xs[m], xs[keep[0]]) for m in keep):
        _close(prob, _log_softmax64(xs[keep[0]]))
        _close(logprob, _log_softmax64(xs[keep[0]]))
    # members permuted together with their weights: nothing changes
    perm = list(reversed(range(c.M)))
    for mode, ref in (("prob", prob), ("logprob", logprob)):
        _close(er.ensemble_ref64([xs[m] for m in perm], w[perm], mode), ref, 1e-12)


def test_identical_members_give_log_softmax():
    g = torch.Generator().manual_seed(1)
    x = (torch.rand(4, 300, generator=g) * 80 - 40).double().numpy()
    for w in ([0.5, 0.5], [0.9, 0.1], [0.2, 0.3, 0.5]):
        for mode in er.MODES:
            _close(er.ensemble_ref64([x] * len(w), w, mode), _log_softmax64(x))


def test_zero_weight_member_is_never_looked_at():
    g = torch.Generator().manual_seed(2)
    x = (torch.rand(3, 50, generator=g) * 80 - 40).double().numpy()
    junk = np.full_like(x, -np.inf)                                                 # not even one finite entry
    for mode in er.MODES:
        _close(er.ensemble_ref64([x, junk], [1.0, 0.0], mode), _log_softmax64(x))
        assert np.array_equal(er.closed_form_f32([x, junk], [1.0, 0.0], mode).numpy(), er.closed_form_f32([x], [1.0], mode).numpy())


def test_float32_yardstick_is_what_the_cpu_measures():
    """The constant the GPU bound is 4x of: the float32 CPU evaluation of the closed form against float64, re-measured."""
    worst = 0.0
    for i, c in enumerate(CASES):
        bufs, xs, w = er.case_views(c, er.ENS_SEED + i)
        for mode in er.MODES:
            ref = er.ensemble_ref64(xs, w, mode)
            got = er.closed_form_f32([b[:, :c.V] for b in bufs], w, mode).numpy()
            assert np.array_equal(np.isneginf(got), np.isneginf(ref)) and not np.isnan(got).any()
            worst = max(worst, er.worst_abs_error(got, ref))
    assert er.CPU_F32_ENSEMBLE_ABS / 2 <= worst <= er.CPU_F32_ENSEMBLE_ABS * 2, worst
