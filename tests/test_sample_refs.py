"""The numpy side of the sampling decode's tests (tests/sample_refs.py): the counter hash is uniform and its streams do not collide,
and the float64 filter does what include/mtn_hip.h (mtn_sample_rows) defines — on hand-built rows."""
import math

import numpy as np

from tests import sample_refs as R


def _chi2_pvalue(stat, dof):
    """Upper tail of the chi-square distribution (Wilson-Hilferty; exact enough at the 1e-6 level for dof >= 30)."""
    z = ((stat / dof) ** (1.0 / 3.0) - (1.0 - 2.0 / (9.0 * dof))) / math.sqrt(2.0 / (9.0 * dof))
    return 0.5 * math.erfc(z / math.sqrt(2.0))


def test_hash_is_uniform_over_2_to_20_counters():
    """2^15 keys x 32 positions under one seed: 256 bins of u, chi-square p-value >= 1e-6 (a fixed seed: deterministic)."""
    keys = np.arange(1 << 15, dtype=np.int64)[:, None]
    pos = np.arange(32)[None, :]
    u = R.uniform24(20260117, keys, pos).ravel()
    assert u.size == 1 << 20 and u.min() >= 0.0 and u.max() < 1.0
    counts = np.bincount((u * 256).astype(np.int64), minlength=256)
    expect = u.size / 256.0
    stat = float(((counts - expect) ** 2 / expect).sum())
    p = _chi2_pvalue(stat, 255)
    print(f"chi-square {stat:.1f} over 255 degrees of freedom, p = {p:.3g}")
    assert p >= 1e-6
    assert abs(u.mean() - 0.5) < 5 * math.sqrt(1.0 / 12.0 / u.size)


def test_hash_streams_do_not_collide():
    """By construction key -> hash is a bijection at a fixed position and position -> hash at a fixed key; the streams of different
    keys differ, (key, position) is not symmetric, and seeds that differ in either word give different streams."""
    keys = np.arange(1 << 16, dtype=np.int64)
    for pos in (0, 1, 29):
        assert np.unique(R.sample_hash(7, keys, pos)).size == keys.size
    for key in (0, 5, (3 << 32) + 1):
        assert np.unique(R.sample_hash(7, key, np.arange(1024))).size == 1024
    streams = R.sample_hash(7, keys[:4096, None], np.arange(30)[None, :])
    assert np.unique(streams, axis=0).shape[0] == 4096
    grid = R.sample_hash(7, np.arange(64, dtype=np.int64)[:, None], np.arange(64)[None, :])
    off = ~np.eye(64, dtype=bool)
    assert (grid != grid.T)[off].mean() > 0.99
    a = R.sample_hash(1, keys[:256], 3)
    assert (a != R.sample_hash(2, keys[:256], 3)).mean() > 0.99 and (a != R.sample_hash(1 + (1 << 32), keys[:256], 3)).mean() > 0.99
    assert (a != R.sample_hash(1, keys[:256] + (1 << 32), 3)).mean() > 0.99          # the key's high word counts
    assert int(R.sample_hash(-1, -1, 0)) == int(R.sample_hash(2 ** 64 - 1, 2 ** 64 - 1, 0))


def test_top_k_keeps_ties_at_the_threshold():
    x = np.log(np.array([0.05, 0.2, 0.2, 0.3, 0.2, 0.05]))
    p = R.filtered(x, R.Params(top_k=2))
    assert set(np.nonzero(p)[0]) == {1, 2, 3, 4}                     # the 2nd largest is 0.2: all three of them stay
    assert np.allclose(p[[1, 2, 3, 4]], np.array([0.2, 0.2, 0.3, 0.2]) / 0.9)
    assert set(np.nonzero(R.filtered(x, R.Params(top_k=1)))[0]) == {3}
    assert np.count_nonzero(R.filtered(x, R.Params(top_k=6))) == 6 and np.count_nonzero(R.filtered(x, R.Params(top_k=0))) == 6


def test_top_p_keeps_ties_and_the_smallest_sufficient_set():
    x = np.log(np.array([0.1, 0.4, 0.25, 0.25]))
    assert set(np.nonzero(R.filtered(x, R.Params(top_p=0.3)))[0]) == {1}
    assert set(np.nonzero(R.filtered(x, R.Params(top_p=0.4)))[0]) == {1}              # mass 0.4 >= 0.4
    assert set(np.nonzero(R.filtered(x, R.Params(top_p=0.5)))[0]) == {1, 2, 3}        # 0.4 < 0.5: the next value, both of its tokens
    assert set(np.nonzero(R.filtered(x, R.Params(top_p=0.95)))[0]) == {0, 1, 2, 3}
    assert abs(R.filtered(x, R.Params(top_p=0.5)).sum() - 1.0) < 1e-12


def test_top_k_runs_before_top_p():
    x = np.log(np.array([0.4, 0.3, 0.2, 0.1]))
    # top-k = 2 leaves {0.4, 0.3}, renormalised 4/7 | 3/7: top_p = 0.6 then needs both; on the unfiltered row it would need two as well,
    # but top_p = 0.5 separates the orders: after top-k 4/7 >= 0.5 keeps one token; top-p first would keep {0.4, 0.3} (0.4 < 0.5)
    assert set(np.nonzero(R.filtered(x, R.Params(top_k=2, top_p=0.6)))[0]) == {0, 1}
    assert set(np.nonzero(R.filtered(x, R.Params(top_k=2, top_p=0.5)))[0]) == {0}
    assert set(np.nonzero(R.filtered(x, R.Params(top_p=0.5)))[0]) == {0, 1}


def test_temperature_sharpens_and_flattens():
    x = np.log(np.array([0.5, 0.25, 0.25]))
    assert np.allclose(R.filtered(x, R.Params(temperature=1.0)), [0.5, 0.25, 0.25])
    assert np.allclose(R.filtered(x, R.Params(temperature=0.5)), np.array([4.0, 1.0, 1.0]) / 6.0)
    assert R.filtered(x, R.Params(temperature=2.0))[0] < 0.5


def test_argmax_survives_bans_and_min_len():
    x = np.log(np.array([0.5, 0.3, 0.15, 0.05]))
    prm = R.Params(top_k=1, banned=(0,), eos=1, min_len=2)
    assert set(np.nonzero(R.filtered(x, prm, position=0))[0]) == {2}                  # 0 banned, <eos> = 1 banned below min_len
    assert set(np.nonzero(R.filtered(x, prm, position=2))[0]) == {1}                  # <eos> allowed from min_len on
    prm = R.Params(top_p=0.01, banned=(0, 1))
    assert set(np.nonzero(R.filtered(x, prm))[0]) == {2}
    for u in (0.0, 0.5, 1.0 - 2.0 ** -24):
        assert R.admissible(x, u, prm, 0.0) == {2}


def test_draw_walks_the_vocabulary_order():
    p = np.array([0.0, 0.25, 0.0, 0.5, 0.25])
    assert [R.draw(p, u) for u in (0.0, 0.2499, 0.25, 0.7499, 0.75, 1.0 - 2.0 ** -24)] == [1, 1, 3, 3, 4, 4]


def test_admissible_is_one_token_without_tolerance_and_widens_with_it():
    rs = np.random.RandomState(3)
    x = np.log(rs.dirichlet(np.ones(50) * 0.3))
    for prm in (R.Params(), R.Params(temperature=0.7, top_k=5), R.Params(top_p=0.9), R.Params(top_k=40, top_p=0.3, banned=(1, 2))):
        p = R.filtered(x, prm)
        for u in rs.randint(0, 1 << 24, size=200) / 16777216.0:
            one = R.admissible(x, u, prm, 0.0)
            assert len(one) == 1 and one == {R.draw(p, u)}
            wide = R.admissible(x, u, prm, 1e-3)
            assert one <= wide
    # u right at a boundary: both neighbours with a tolerance, one without
    p = np.array([0.5, 0.5])
    assert R.admissible(np.log(p), 0.5, R.Params(), 0.0) == {1} and R.admissible(np.log(p), 0.5, R.Params(), 1e-6) == {0, 1}
    # a token within eps of the top-k threshold is optional
    x = np.log(np.array([0.2, 0.2 * (1 - 1e-7), 0.6]))
    assert R.admissible(x, 0.3, R.Params(top_k=2), 0.0) == {2}
    assert R.admissible(x, 0.3, R.Params(top_k=2), 1e-5) == {1, 2}
    # ... and without such a token the top-k set is exact whatever the tolerance
    x = np.log(np.array([0.2, 0.1, 0.7]))
    assert R.admissible(x, 0.3, R.Params(top_k=1), 1e-3) == {2} and R.admissible(x, 0.1, R.Params(top_k=2), 1e-3) == {0}
