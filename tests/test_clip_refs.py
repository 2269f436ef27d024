"""tests/clip_refs.py held against torch.nn.utils.clip_grad_norm_ on CPU tensors in float64 (so that the comparison is about the
definition, not about fp32 summation), and each GPU case's own condition: no case's norm sits on the clip threshold.  No GPU needed."""
import math

import numpy as np
import pytest
import torch

from tests import clip_refs as R


def _torch_clip(parts, max_norm):
    """(total norm, the gradients after clipping) as clip_grad_norm_ computes them, error_if_nonfinite=False."""
    ps = [torch.nn.Parameter(torch.zeros(p.shape, dtype=torch.float64)) for p in parts]
    for p, g in zip(ps, parts):
        p.grad = torch.from_numpy(g.astype(np.float64))
    total = torch.nn.utils.clip_grad_norm_(ps, max_norm, norm_type=2.0, error_if_nonfinite=False)
    return float(total), [p.grad.numpy() for p in ps]


@pytest.mark.parametrize("max_norm", [0.5, 1.0, 7.0, 1e3, R.INF])
@pytest.mark.parametrize("scale", [1.0, 1e-3, 40.0])
def test_the_definition_is_clip_grad_norm(max_norm, scale):
    rng = np.random.default_rng(5)
    parts = [(rng.standard_normal(s) * scale).astype(np.float32) for s in ((7, 3), (11,), (2, 5, 4), (1,))]
    flat = np.concatenate([p.reshape(-1) for p in parts])
    norm, coef, scale32 = R.clip(flat, max_norm)
    t_norm, t_grads = _torch_clip(parts, max_norm)
    assert abs(norm - t_norm) <= 1e-14 * t_norm
    got = np.concatenate([p.reshape(-1) for p in parts]).astype(np.float64) * coef
    want = np.concatenate([g.reshape(-1) for g in t_grads])
    assert np.abs(got - want).max() <= 1e-14 * np.abs(want).max()
    assert (coef == 1.0) == (t_norm + 1e-6 <= max_norm)
    assert scale32.dtype == np.float32 and abs(float(scale32) - coef) <= 2.0 ** -24 * coef      # rounded once
    if coef == 1.0:
        assert scale32.view(np.int32) == np.float32(1.0).view(np.int32)


def test_a_base_scale_scales_the_norm_and_the_result():
    x = np.random.default_rng(2).standard_normal(100).astype(np.float32)
    n1, _, _ = R.clip(x, 1.0)
    for base in (0.125, -3.0):
        norm, coef, s = R.clip(x, 1.0, base)
        assert norm == n1 * abs(base)
        t_norm, _ = _torch_clip([x.astype(np.float64) * base], 1.0)
        assert abs(norm - t_norm) <= 1e-14 * t_norm
        assert coef < 1.0 and float(s) == float(np.float32(np.float64(np.float32(base)) * coef)) and (float(s) < 0) == (base < 0)
    norm, coef, s = R.clip(x, 1e6, -3.0)
    assert coef == 1.0 and s.view(np.int32) == np.float32(-3.0).view(np.int32)


def test_non_finite_norms_and_the_stats_block():
    x = np.ones(8, dtype=np.float32)
    st = [0.0] * 5
    seq = [(x, 1.0), (x * 0, 1.0), (np.where(np.arange(8) == 3, np.nan, x).astype(np.float32), 1.0),
           (np.where(np.arange(8) == 7, np.inf, x).astype(np.float32), R.INF), (x * 3, R.INF), (x * 3, 0.5)]
    for v, c in seq:
        norm, coef, s = R.clip(v, c)
        R.stats_update(st, norm, coef)
        if not math.isfinite(norm):
            assert math.isnan(coef) and math.isnan(float(s))
    assert st[2] == 6 and st[3] == 2 and st[4] == 2
    assert st[1] == math.sqrt(72.0) and abs(st[0] - (math.sqrt(8.0) + 0.0 + 2 * math.sqrt(72.0))) < 1e-12
    assert R.clip(x * 0, 1.0)[1] == 1.0                      # a zero gradient is not clipped: 1 / 1e-6 > 1
    assert R.clip(x, R.INF)[1] == 1.0


def test_partials_are_the_grid_of_the_kernel():
    assert [R.partials(n) for n in (0, 1, 1024, 1027, 1028, 2048, 2052)] == [0, 1, 1, 1, 2, 2, 3]
    assert R.partials(R.CAP_ELEMS) == R.GRID_CAP == R.partials(R.CAP_ELEMS + 5) == R.partials(1 << 40)
    assert R.partials(R.CAP_ELEMS - 1) == R.GRID_CAP                                # ... the last workgroup one thread short


def test_the_cases_cover_what_the_issue_names():
    ids = [c["id"] for c in R.CASES]
    assert len(set(ids)) == len(ids)
    for n in R.SIZES:
        assert {c["scale"] for c in R.CASES if c["n"] == n and c["kind"] == "randn"} >= {1.0, 1e-25, 1e25}
    assert {c["kind"] for c in R.CASES} == {"randn", "zeros", "nan", "inf"}
    assert R.SIZES[-1] * 4 < 14e6                                                     # the largest buffer is 13 MB


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c["id"])
def test_no_case_sits_on_the_threshold(case):
    """The side of the clip is never a rounding accident: |norm - C| > 1e-9 C, and the same for the quantity the coefficient really
    compares, norm + 1e-6."""
    norm, coef, scale = R.expected(case["id"])
    C = case["max_norm"]
    if case["kind"] in ("nan", "inf"):
        assert not math.isfinite(norm) and math.isnan(coef) and math.isnan(float(scale))
        return
    assert math.isfinite(norm) and (norm > 0) == (case["kind"] != "zeros")
    if math.isfinite(C):
        assert abs(norm - C) > 1e-9 * C
        assert abs(norm + 1e-6 - C) > 1e-9 * C
    assert (coef < 1.0) == (norm + 1e-6 > C)
    assert math.isfinite(float(scale))


def test_both_sides_of_the_clip_occur():
    sides = {R.expected(c["id"])[1] < 1.0 for c in R.CASES if c["kind"] in ("randn", "zeros")}
    assert sides == {True, False}
    big = [c for c in R.CASES if c["scale"] == 1e25 and c["kind"] == "randn"]
    assert all(R.expected(c["id"])[0] > 1e25 for c in big if c["n"] >= 4)            # the squares left fp32's range; the norm did not
