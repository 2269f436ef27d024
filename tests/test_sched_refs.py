"""CPU checks of tests/sched_refs.py, the numpy definition the GPU tests of mtn_sched_mix compare with: the error bound E_c holds against a
numpy-float32 emulation of the kernel's operations, the coin falls at its rate, the float64 Gumbel picks are distributed as
softmax(z / temperature), and the GPU SAMPLE cases have gaps between the best and the second score wide enough that the GPU check
(s64[pick] >= max s64 - 2 E) forces the float64 arg-max: a condition on the inputs, so that check cannot be vacuous."""
import numpy as np
import pytest

from tests import sched_refs as R


def test_schedule_is_float32_and_matches_the_config():
    from mtn_amd.train_step import SchedConfig
    assert R.prob(0, 0.25, 0, 0) == np.float32(0.25) and R.prob(4, 0.25, 5, 0) == 0.0 and R.prob(5, 0.25, 5, 0) == np.float32(0.25)
    assert R.prob(3, 0.6, 1, 4) == np.float32(np.float32(0.6) * np.float32(0.5))
    assert R.prob(1, 0.6, 1, 4) == 0.0 and R.prob(5, 0.6, 1, 4) == np.float32(0.6) and R.prob(900, 0.6, 1, 4) == np.float32(0.6)
    assert R.prob(2, 1.0, 1, 3) == np.float32(np.float32(1.0) / np.float32(3.0))
    for start, ramp in ((0, 0), (5, 0), (1, 4), (2, 7), (0, 1000)):
        cfg = SchedConfig(0.3, start=start, ramp=ramp)
        for step in (0, 1, 2, 3, 5, 8, 9, 500, 1000, 5000):
            assert np.float32(cfg.prob_at(step)) == R.prob(step, 0.3, start, ramp)


def test_gumbel_is_finite_over_the_whole_range_of_the_hash():
    k = np.array([0, 1, 2, (1 << 23) - 1, 1 << 23, (1 << 23) + 1, (1 << 24) - 2, (1 << 24) - 1])
    g64, g32 = R.gumbel64(k), R.gumbel32(k)
    assert np.isfinite(g64).all() and np.isfinite(g32).all()
    assert (np.diff(g64) > 0).all()                                       # monotone in u, across the switch at one half too
    assert abs(g64[0] + np.log(-np.log(0.5 / 16777216.0))) < 1e-12 and abs(g64[-1] + np.log(-np.log1p(-0.5 / 16777216.0))) < 1e-12


@pytest.mark.parametrize("inv_t", [1.0, 1.0 / 0.7, 0.5, 4.0])
def test_bound_holds_against_a_float32_emulation(inv_t):
    rs = np.random.RandomState(7)
    n = 400000
    k = rs.randint(0, 1 << 24, size=n)
    edge = np.array([0, 1, 2, 3, (1 << 23) - 2, (1 << 23) - 1, 1 << 23, (1 << 23) + 1, (1 << 24) - 3, (1 << 24) - 2, (1 << 24) - 1])
    k[:edge.size * 4] = np.repeat(edge, 4)
    # u with -log(u) near 1 (g near 0), where the outer logarithm's argument sits next to its zero
    near = np.round(np.exp(-1.0) * 16777216.0).astype(np.int64) + np.arange(-200, 200)
    k[100:100 + near.size] = near
    z = (rs.randn(n) * np.where(rs.rand(n) < 0.1, 100.0, 3.0)).astype(np.float32)
    z[:8] = [0.0, -0.0, np.inf, -np.inf, 1e-30, -1e30, 3.0e38, -3.0e38]
    s64, E = R.scores64(z, np.float32(inv_t), k)
    s32 = R.scores32(z, np.float32(inv_t), k).astype(np.float64)
    fin = np.isfinite(s64)
    with np.errstate(invalid="ignore"):
        assert (np.abs(s32[fin] - s64[fin]) <= E[fin]).all()
    assert (s32[~fin] == s64[~fin]).all()                                 # (an infinite logit gives the same infinity in both)
    # the bound is not slack by orders of magnitude: the emulation uses a good part of it somewhere
    fin &= np.isfinite(E)
    assert (np.abs(s32[fin] - s64[fin]) / E[fin]).max() > 0.05


def test_coin_rate_lies_in_its_binomial_interval():
    B, T = 64, 4000
    key = (np.arange(B, dtype=np.int64) * 7919 + 13)
    for seed, step, p in ((0, 0, 0.25), (5, 17, 0.25), (1 << 40, 3, 0.9), (0, 1, 0.01)):
        u = R.coin(seed, step, key, T)
        assert u.dtype == np.float32 and (u >= 0).all() and (u < 1).all()
        n = B * T
        hits = int((u < np.float32(p)).sum())
        assert abs(hits - n * p) <= 5.0 * np.sqrt(n * p * (1 - p)), (seed, step, p, hits)
    # another step, another stream; the same step, the same bytes
    a, b, c = R.coin(0, 0, key, T), R.coin(0, 1, key, T), R.coin(0, 0, key, T)
    assert (a == c).all() and (a != b).mean() > 0.99
    # the position shares the key word with key << 12: positions below 4096 of different keys never collide
    assert R._words(0, 0, np.array([1, 2]), 4095)[1][0, -1] != R._words(0, 0, np.array([1, 2]), 4095)[1][1, 0]


@pytest.mark.parametrize("temperature", [1.0, 0.6, 2.0])
def test_float64_gumbel_picks_are_distributed_as_the_softmax(temperature):
    V, n = 6, 60000
    z = np.array([0.3, -1.2, 2.0, 0.0, 1.1, -0.4], dtype=np.float32)
    inv_t = np.float32(1.0 / temperature)
    key = np.arange(n, dtype=np.int64) * 2654435761 % (1 << 50)
    kb = R.column_bits(11, 4, key, 2, V)[:, 1]                            # position t = 1 of n sequences
    s, _ = R.scores64(np.broadcast_to(z, (n, V)), inv_t, kb)
    counts = np.bincount(np.argmax(s, axis=1), minlength=V).astype(np.float64)
    e = np.exp((z.astype(np.float64) * float(inv_t)))
    expect = n * e / e.sum()
    chi2 = ((counts - expect) ** 2 / expect).sum()
    assert chi2 < 35.9                                                   # chi-square, 5 degrees of freedom, upper quantile 1 - 1e-6


SAMPLE_CASES = [c for c in R.CASES if c.pick == R.SAMPLE]


@pytest.mark.parametrize("case", SAMPLE_CASES, ids=lambda c: c.name)
def test_gpu_sample_cases_have_decisive_gaps(case):
    """best - runner-up > 2 (E_best + E_runner-up) in at least 99 % of the replaced rows: there the fp32 arg-max cannot differ from the
    float64 one, and the GPU check leaves exactly one admissible column."""
    z, trg, key = case.data()
    o = R.mix(z, trg, key, case.step, **case.kw())
    ok = R.admitted(case.V, case.pad, case.banned)
    rows = np.argwhere(o["replaced"])
    assert len(rows) >= 3                                                 # the case replaces something
    decisive = 0
    for b, t in rows:
        s, E = o["s"][b, t][ok], o["E"][b, t][ok]
        order = np.argsort(-s, kind="stable")
        if s.size == 1:
            decisive += 1
            continue
        best, second = order[0], order[1]
        decisive += bool(s[best] - s[second] > 2.0 * (E[best] + E[second]))
    assert decisive >= 0.99 * len(rows)


def test_cases_cover_the_shapes_and_the_planted_rows():
    assert {c.V for c in R.CASES if c.pick == R.ARGMAX} == {1, 3, 255, 257, 1030, 4099} == {c.V for c in SAMPLE_CASES}
    assert all(c.B <= 4 and c.T <= 8 for c in R.CASES)
    assert any(c.offset % 4 for c in R.CASES if c.pick == R.ARGMAX) and any(c.offset % 4 for c in SAMPLE_CASES)
    assert any(c.ldx > c.V for c in R.CASES)
    seen = set()
    for c in R.CASES:
        z, trg, key = c.data()
        o = R.mix(z, trg, key, c.step, **c.kw())
        assert (o["mixed"][trg == c.pad] == c.pad).all() and (o["mixed"][:, 0] == trg[:, 0]).all()
        assert not np.isin(o["mixed"][o["replaced"]], (c.pad,) + c.banned).any()
        assert o["stats"][2] <= o["stats"][1] <= o["stats"][0]
        if o["coin"].sum() > o["replaced"].sum():
            seen.add("kept_gold")
        seen.update(c.plant)
    assert {"ties", "neginf", "banned", "nan", "posinf", "kept_gold"} <= seen
    assert trg[0, 0] == c.pad                                             # <pad> at t = 0
