"""tests/accum_refs.py against the definition, without a GPU.
  * For K in 1..5 and integer weights in 1..2000 a window's float32 result lies within (K + 3) * 2^-24 * sum_k |w_k g_k| / sum_k w_k of
    the float64 value of G = (sum_k w_k g_k) / (sum_k w_k).  Derived, with u = 2^-24 and S = sum_k |w_k g_k|: the K products err by u S
    in all, each of the K - 1 additions by at most u S (1 + O(u)), the total of integer weights below 2^24 is exact, the reciprocal
    (rounded once from double) and the final product by u each: (K + 2) u S / sum w, and one more u for the second-order terms.
  * FIRST followed by LAST with equal w and equal g returns g within 4 * 2^-24 relative (w g exact or rounded, the sum 2 w g exact, the
    reciprocal, the product).
  * the GPU cases are what their docstring says, and NaN / inf propagate as IEEE arithmetic says."""
import numpy as np
import pytest

from tests import accum_refs as R

U = 2.0 ** -24


@pytest.mark.parametrize("K", [1, 2, 3, 4, 5])
def test_a_window_lies_within_the_derived_bound_of_the_definition(K):
    worst = 0.0
    for seed in range(20):
        rng = np.random.default_rng(100 * K + seed)
        n = 4099
        gs = [rng.standard_normal(n).astype(np.float32) * np.float32(10.0 ** rng.integers(-3, 4)) for _ in range(K)]
        ws = [np.float32(w) for w in rng.integers(1, 2001, size=K)]
        got, total = R.window(gs, ws)
        want, mag = R.exact(gs, ws)
        assert got.dtype == np.float32 and float(total) == float(sum(np.float64(w) for w in ws))
        err = np.abs(got.astype(np.float64) - want)
        assert (err <= (K + 3) * U * mag).all()
        worst = max(worst, float((err / (U * mag)).max()))
    print("K = %d: largest error %.3f of 2^-24 * sum |w g| / sum w (bound %d)" % (K, worst, K + 3))
    if K == 1:
        assert worst == 0.0                                  # a window of one is g itself


def test_first_then_last_with_equal_terms_returns_g():
    rng = np.random.default_rng(7)
    g = rng.standard_normal(10007).astype(np.float32)
    for w in (1.0, 3.0, 777.0, 2000.0):
        acc, total = R.first(g, w)
        got, t = R.last(acc, g, w, total)
        assert float(t) == 2.0 * w
        rel = np.abs(got.astype(np.float64) - g.astype(np.float64)) / np.abs(g.astype(np.float64))
        assert (rel <= 4 * U).all()


def test_the_modes_are_separately_rounded_operations():
    """Against scalar float32 arithmetic spelt out, on values where an fma would differ."""
    rng = np.random.default_rng(11)
    g, a = rng.standard_normal(257).astype(np.float32), rng.standard_normal(257).astype(np.float32) * np.float32(1000.0)
    w, tot = np.float32(1999.0), np.float32(4001.0)
    acc, t = R.add(a, g, w, tot)
    out, t2 = R.last(a, g, w, tot)
    inv = np.float32(1.0 / np.float64(np.float32(6000.0)))
    fused = 0
    for i in range(g.size):
        p = np.float32(w * g[i])
        s = np.float32(a[i] + p)
        assert acc[i] == s and out[i] == np.float32(s * inv)
        fused += int(np.float32(np.float64(a[i]) + np.float64(w) * np.float64(g[i])) != s)
    assert float(t) == float(t2) == 6000.0 and fused > 0      # the once-rounded sum differs somewhere: the data can tell the two apart


def test_the_gpu_cases():
    assert R.SIZES[:6] == [1, 3, 4, 5, 1023, 1024] and R.SIZES[6] == 256 * 1024 + 7 and R.SIZES[7] == 2048 * 1024 * 2 + 5
    assert {c["K"] for c in R.CASES} == {2, 3} and len(R.CASES) == 2 * len(R.SIZES)
    for case in R.CASES:
        if case["n"] > 1024:
            continue
        gs, ws = R.data(case)
        n, K = case["n"], case["K"]
        assert len(gs) == K and all(g.dtype == np.float32 and g.shape == (n,) for g in gs) and all(1 <= float(w) <= 2000 for w in ws)
        mags = np.abs(np.concatenate(gs))
        if n >= 1023:
            fin = mags[np.isfinite(mags)]
            assert (fin > 1e29).any() and ((fin < 1e-29) & (fin > 0)).any()
        G, total = R.window(gs, ws)
        assert np.isnan(G[n // 2]) and (np.isnan(G[n - 1]) if n // 2 == n - 1 else np.isposinf(G[n - 1]))
        ok = np.ones(n, dtype=bool)
        ok[[n // 2, n - 1]] = False
        assert np.isfinite(G[ok]).all() and float(total) == sum(float(w) for w in ws)
        assert R.same_bytes(G, G.copy()) and (n < 4 or not R.same_bytes(G, np.roll(G, 1)))
