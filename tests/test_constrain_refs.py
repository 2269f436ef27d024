"""tests/constrain_refs.py against hand-worked cases (CPU): the numpy definitions the constraint kernel is compared with."""
import numpy as np

from tests.constrain_refs import constrain_row, has_repeated_ngram, history_from_log


def _row(V=12):
    return (-np.arange(1, V + 1, dtype=np.float32) / np.float32(3.0)).astype(np.float32)


def _banned(out):
    return sorted(int(c) for c in np.flatnonzero(np.isneginf(out)))


def test_bigram_blocking_bans_what_followed_the_last_token():
    x = _row()
    out = constrain_row(x, [7, 3, 7], 2, 1.0)
    assert _banned(out) == [3]                               # 7 was followed by 3 once: "7 3" must not occur again
    keep = np.ones(x.size, bool)
    keep[3] = False
    assert out[keep].tobytes() == x[keep].tobytes() and x[3] == np.float32(-4.0 / 3.0)     # the input is not modified


def test_unigram_blocking_bans_every_token_of_the_history():
    assert _banned(constrain_row(_row(), [7, 3, 7, 0], 1, 1.0)) == [0, 3, 7]
    assert _banned(constrain_row(_row(), [], 1, 1.0)) == []


def test_trigram_blocking_and_every_earlier_occurrence_counts():
    # history a b c a b: the suffix "a b" occurred at 0 -> c banned; N = 3
    assert _banned(constrain_row(_row(), [4, 5, 6, 4, 5], 3, 1.0)) == [6]
    # two earlier occurrences with different continuations: both banned
    assert _banned(constrain_row(_row(), [4, 5, 6, 4, 5, 8, 4, 5], 3, 1.0)) == [6, 8]
    # overlapping: 2 2 2 with N = 2 -> "2 2" occurred: 2 banned
    assert _banned(constrain_row(_row(), [2, 2], 2, 1.0)) == [2]
    assert _banned(constrain_row(_row(), [2], 2, 1.0)) == []  # "2 ?" has not occurred yet


def test_history_shorter_than_n_minus_one_bans_nothing():
    x = _row()
    for N, h in [(3, [5]), (4, [5, 5]), (8, [1, 2, 3, 1, 2, 3]), (4, [])]:
        assert constrain_row(x, h, N, 1.0).tobytes() == x.tobytes(), (N, h)
    # exactly N - 1 tokens: a complete suffix, but no earlier occurrence can exist
    assert constrain_row(x, [5, 5], 3, 1.0).tobytes() == x.tobytes()


def test_penalty_is_one_float32_multiply_applied_once_per_distinct_token():
    x = _row()
    out = constrain_row(x, [7, 3, 7], 0, 1.3)
    th = np.float32(1.3)
    assert out[7] == np.float32(x[7]) * th and out[3] == np.float32(x[3]) * th
    assert out[7] != np.float32(x[7]) * th * th              # 7 occurs twice: still one multiply
    assert out[7] < x[7] and out[3] < x[3]                   # log-probabilities are <= 0: the penalty lowers them
    keep = np.ones(x.size, bool)
    keep[[3, 7]] = False
    assert out[keep].tobytes() == x[keep].tobytes() and out.dtype == np.float32
    assert constrain_row(x, [7, 3, 7], 0, 1.0).tobytes() == x.tobytes()


def test_ban_overrides_penalty_and_out_of_range_tokens_name_no_column():
    x = _row()
    out = constrain_row(x, [7, 3, 7], 2, 1.3)
    assert _banned(out) == [3] and out[7] == np.float32(x[7]) * np.float32(1.3)
    out = constrain_row(x, [99, 3, 99, -1], 1, 1.5)          # V = 12
    assert _banned(out) == [3]
    keep = np.ones(x.size, bool)
    keep[3] = False
    assert out[keep].tobytes() == x[keep].tobytes()
    assert _banned(constrain_row(x, [99, 3, 99], 2, 1.0)) == [3]      # ... but they do take part in the comparisons


def test_history_from_log_follows_the_parents():
    # one dialogue of width 3, three steps.  step 0: rows 0..2 extend row 0 with 10, 11, 12; step 1: row 0 extends old row 2 with 20,
    # row 1 extends old row 0 with 21; step 2: row 0 extends old row 1 with 30
    tok = np.array([[10, 11, 12], [20, 21, 77], [30, 78, 79]], dtype=np.int32)
    par = np.array([[0, 0, 0], [2, 0, 9], [1, -4, 1]], dtype=np.int32)
    assert history_from_log(tok, par, 3, 0, 3) == [10, 21, 30]
    assert history_from_log(tok, par, 2, 0, 3) == [12, 20]
    assert history_from_log(tok, par, 2, 1, 3) == [10, 21]
    assert history_from_log(tok, par, 0, 2, 3) == []
    assert history_from_log(tok, par, 99, 0, 3) == [10, 21, 30]       # step clamped to L
    assert history_from_log(tok, par, 2, 2, 3) == [12, 77]            # a dead row: parent 9 clamped to 2
    assert history_from_log(tok, par, 3, 1, 3) == [12, 20, 78]        # parent -4 clamped to 0
    # second dialogue of two: rows 3..5 index their own group
    tok2 = np.concatenate([tok, tok + 100], 1)
    par2 = np.concatenate([par, par], 1)
    assert history_from_log(tok2, par2, 3, 3, 3) == [110, 121, 130]
    # no parents: a row's own column
    assert history_from_log(tok, None, 3, 1, 1) == [11, 21, 78]


def test_has_repeated_ngram():
    assert has_repeated_ngram([7, 3, 7, 3], 2) and not has_repeated_ngram([7, 3, 7], 2)
    assert has_repeated_ngram([7, 3, 7], 1) and not has_repeated_ngram([7, 3, 5], 1)
    assert has_repeated_ngram([2, 2, 2], 2) and not has_repeated_ngram([2, 2], 2)
    assert not has_repeated_ngram([], 3) and not has_repeated_ngram([1, 2], 3)
    assert has_repeated_ngram([1, 2, 3, 9, 1, 2, 3], 3) and not has_repeated_ngram([1, 2, 3, 9, 1, 2, 4], 3)


def test_blocking_makes_a_repeat_impossible():
    """Whatever a selection picks among the unbanned columns of the constrained row, the extended history holds no repeated N-gram."""
    rs = np.random.RandomState(0)
    for N in (1, 2, 3, 4):
        h = []
        for _ in range(40):
            out = constrain_row(_row(64), h, N, 1.0)
            free = np.flatnonzero(~np.isneginf(out))
            # a small alphabet makes repeats likely: prefer the lowest free columns
            h.append(int(free[rs.randint(0, min(3, free.size))]))
            assert not has_repeated_ngram(h, N), (N, h)
