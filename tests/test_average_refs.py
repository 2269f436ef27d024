"""tests/average_refs.py (the numpy float32 definition of csrc/average.hip) against float64."""
import numpy as np
import pytest

from tests import average_refs as R

F = np.float32


def _values(rs, n):
    """normal floats with magnitudes from 1e-6 to 1e3 and both signs, plus exact zeros"""
    x = (10.0 ** rs.uniform(-6, 3, n) * rs.choice([-1.0, 1.0], n)).astype(F)
    x[rs.rand(n) < 0.05] = 0.0
    return x


def test_ema_coef_warm_up():
    assert R.ema_coef(0.9, 1) == F(9.0) / F(11.0)
    assert R.ema_coef(0.9999, 1) == F(9.0) / F(11.0)
    for t in (80, 81, 100, 10000):
        assert R.ema_coef(0.9, t) == F(1.0) - F(0.9)
    assert R.ema_coef(0.9, 79) > F(1.0) - F(0.9)
    assert R.ema_coef(0.0, 5) == F(1.0)
    assert isinstance(R.ema_coef(0.9, 3), np.float32)
    # 1 - min(decay, (1 + t) / (10 + t)), the usual form of the warm-up, up to rounding
    for t in (1, 7, 79, 500):
        assert abs(float(R.ema_coef(0.999, t)) - (1.0 - min(0.999, (1.0 + t) / (10.0 + t)))) < 1e-6


def test_lerp_is_three_fp32_operations():
    rs = np.random.RandomState(0)
    a, x = _values(rs, 4096), _values(rs, 4096)
    for c in (0.0, 1.0 / 3.0, 0.5, 1.0):
        got = R.lerp(a, x, c)
        assert got.dtype == F
        want = (a.astype(np.float64) + float(F(c)) * (x.astype(np.float64) - a.astype(np.float64)))
        # three roundings, each at most 2^-24 of a magnitude no larger than 2 max(|a|, |x|)
        assert np.all(np.abs(got - want) <= 6 * 2.0 ** -24 * np.maximum(np.abs(a), np.abs(x)))
    assert np.array_equal(R.lerp(a, x, 0.0), a)
    assert np.array_equal(R.lerp(a, a, 1.0 / 3.0).view(np.int32), (a + F(0)).view(np.int32))


@pytest.mark.parametrize("decay", [0.9, 0.999])
def test_ema_run_against_float64(decay):
    rs = np.random.RandomState(1)
    start = _values(rs, 2048)
    snaps = [_values(rs, 2048) for _ in range(12)]
    got = R.ema_run(snaps, decay, start=start)
    ref = start.astype(np.float64)
    for i, p in enumerate(snaps):
        c = max(1.0 - decay, 9.0 / (10.0 + (1 + i)))
        ref = ref + c * (p.astype(np.float64) - ref)
    big = max(np.abs(start).max(), max(np.abs(p).max() for p in snaps))
    # per step: three roundings (8 * 2^-24 * max|x| with the margin of running_mean's bound) and the fp32 coefficient (2^-24 relative)
    assert np.all(np.abs(got - ref) <= 8 * len(snaps) * 2.0 ** -24 * big)
    # the default start is the first snapshot: the first step then changes nothing
    assert np.array_equal(R.ema_run(snaps[:1], decay), snaps[0])


@pytest.mark.parametrize("weights", [None, [1, 1, 2], [0, 3, 1, 0, 2], [0.5, 0.25, 0.25]])
def test_running_mean_against_float64(weights):
    rs = np.random.RandomState(2)
    K = 3 if weights is None else len(weights)
    xs = [_values(rs, 4099) for _ in range(K)]
    got = R.running_mean(xs, weights)
    w = np.ones(K) if weights is None else np.asarray(weights, dtype=np.float64)
    ref = sum(wk * x.astype(np.float64) for wk, x in zip(w, xs)) / w.sum()
    big = np.max(np.abs(np.stack(xs)), axis=0)
    assert got.dtype == F
    assert np.all(np.abs(got - ref) <= 8 * K * 2.0 ** -24 * big)


def test_running_mean_of_identical_inputs_is_the_input():
    rs = np.random.RandomState(3)
    x = _values(rs, 1000)
    x = np.where(x == 0, F(0), x)             # (no negative zeros: -0 + 0 = +0)
    assert np.array_equal(R.running_mean([x, x, x]).view(np.int32), x.view(np.int32))
    assert np.array_equal(R.running_mean([x, x, x], [1, 1, 2]).view(np.int32), x.view(np.int32))
