"""Properties of the minimum-Bayes-risk definition (tests/mbr_refs.py, the numpy form of include/mtn_hip.h mtn_mbr_select) without a GPU:
what the header promises about U, a second formulation of the clipped match count, tie order, and that the seeded sets the kernel tests
draw from do move the answer away from index 0."""
import random

import numpy as np
import pytest

from tests import mbr_refs as R


def _sets():
    rng = random.Random(11)
    return [R.random_set(rng, 6, 14, nv) for nv in (2, 3, 5, 12, 1000) for _ in range(4)]


@pytest.mark.parametrize("N", [1, 2, 3, 4])
def test_utility_properties(N):
    for hyps in _sets():
        hyps = hyps + [[]]
        for h in hyps:
            assert R.utility(h, h, N) == min(len(h), N) / N
            assert R.utility(h, [], N) == 0.0 and R.utility([], h, N) == 0.0
            for r in hyps:
                u = R.utility(h, r, N)
                assert u == R.utility(r, h, N) and 0.0 <= u <= 1.0
    assert R.utility([], [], N) == 0.0


def test_known_values():
    assert R.utility([1, 2, 3], [1, 2, 3], 4) == 3 / 4                       # no 4-gram on either side: F_4 = 0
    assert R.utility([1, 1, 1], [1], 1) == 2 * 1 / 4                          # clipped: one of the three 1s counts
    assert R.utility([1, 2, 1, 2], [1, 2], 2) == (2 * 2 / 6 + 2 * 1 / 4) / 2
    assert R.utility([7], [8], 3) == 0.0


@pytest.mark.parametrize("N", [1, 2, 3, 4])
def test_occurrence_clipping_is_the_same_number(N):
    for hyps in _sets():
        for h in hyps:
            for r in hyps:
                assert R.utility(h, r, N) == R.utility_by_occurrence(h, r, N)
    a, b = R.select(_sets()[3], N), R.select(_sets()[3], N, util_fn=R.utility_by_occurrence)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2] and np.array_equal(a[3], b[3])


def test_duplicates_tie_and_resolve_by_index():
    h, g = [4, 5, 6, 4, 5], [9, 9, 4]
    util, e, best, order = R.select([g, h, [1], h, g, h], 3)
    assert e[1] == e[3] == e[5] and e[0] == e[4] and e[1] > e[0] > e[2]
    assert best == 1 and order.tolist() == [1, 3, 5, 0, 4, 2]
    # padding: invalid entries follow by ascending index, expected -1, util 0
    util, e, best, order = R.select([h, h], 2, K=4)
    assert order.tolist() == [0, 1, 2, 3] and best == 0 and e.tolist()[2:] == [-1.0, -1.0] and not util[2:].any() and not util[:, 2:].any()
    assert R.select([], 2, K=3)[2] == -1 and R.select([], 2, K=3)[3].tolist() == [0, 1, 2]


def test_weights_and_expected_value():
    hyps = [[1, 2, 3], [1, 2], [3]]
    util, e, best, order = R.select(hyps, 2, w=[0.5, 0.25, 0.25])
    for i in range(3):
        acc = 0.0
        for j, w in enumerate([0.5, 0.25, 0.25]):
            acc = acc + w * util[i, j]
        assert e[i] == acc
    w = R.score_weights([-1.0, -3.0, -2.0], 2.0)
    assert abs(sum(w) - 1.0) < 1e-15 and w[0] > w[2] > w[1] and w[0] / w[1] == pytest.approx(np.exp(1.0))
    assert R.score_weights([5.0], 0.5) == [1.0]


def test_cut_log():
    eos = 3
    tok = np.array([[3, 5, 5], [4, 6, 5], [4, 3, 5], [4, 3, 5]], dtype=np.int32)
    assert R.cut_log(tok, eos) == [[], [5, 6], [5, 5, 5]]


def test_seeded_sets_move_the_answer():
    """Over 200 seeded sets (ids from 12 values, K = 16, lengths 0..30, N = 4, sorted random weights) the answer is not index 0 in at
    least 40 %: a kernel that always answers 0 cannot pass the kernel tests that draw from these sets."""
    sets = R.seeded_sets(2024, 200, 16, 30, 12)
    moved = sum(1 for hyps, w in sets if R.select(hyps, 4, w)[2] != 0)
    print("best != 0 in %d of 200 sets" % moved)
    assert moved >= 80
