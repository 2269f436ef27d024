"""The Python definition of the corpus metrics (tests/eval_refs.py; include/mtn_hip.h mtn_eval_metrics) against values worked by hand."""
import math

import numpy as np
import pytest

from tests import eval_refs as R

# words as small integers: the=1 cat=2 is=3 on=4 mat=5 a=6 dog=7 sat=8 there=9
THE, CAT, IS, ON, MAT, A, DOG, SAT, THERE = range(1, 10)


def test_hypothesis_equal_to_its_single_reference():
    # item 0 is scored; item 1 holds other words, so no n-gram of item 0 is in every item: idf = ln 2 for all of them
    h = [THE, CAT, IS, ON, THE, MAT]
    ev = R.evaluate([h, [A, DOG]], [[h], [[A, DOG]]])
    assert ev["stats"][0].tolist() == [6, 5, 4, 3, 6, 5, 4, 3, 6, 6]
    assert ev["rouge"][0] == 1.0 and abs(ev["cider"][0] - 10.0) < 1e-12
    # both items equal their references: every Bleu_n is 1 up to the 1e-9 / 1e-15 constants of the definition
    assert np.all(np.abs(ev["corpus"][:4] - 1.0) < 1e-9) and ev["corpus"][4] == 1.0
    assert ev["corpus"][6] == 8 and ev["corpus"][7] == 8


def test_clipped_unigrams():
    ev = R.evaluate([[THE] * 7], [[[THE, CAT, IS, ON, THE, MAT]]])
    assert ev["stats"][0].tolist() == [7, 6, 5, 4, 2, 0, 0, 0, 7, 6]          # match_1 = min(7, 2)
    # the max over references comes before the clip: 2 from the first reference, 3 from the second, never 5
    assert R.bleu_stats([THE] * 7, [[THE, CAT, THE], [THE, THE, THE, MAT]])[4] == 3


def test_brevity_penalty_at_a_stated_ratio():
    # 3 hypothesis tokens against a reference of 6: ratio 0.5, penalty exp(1 - 2); all three unigrams match
    ev = R.evaluate([[THE, CAT, IS]], [[[THE, CAT, IS, ON, THE, MAT]]])
    assert ev["corpus"][6] == 3 and ev["corpus"][7] == 6
    assert abs(ev["corpus"][0] - math.exp(-1.0)) < 1e-9
    assert abs(ev["corpus"][1] - math.exp(-1.0)) < 1e-9                        # 2 of 2 bigrams as well
    # a hypothesis longer than its reference is not penalised
    ev = R.evaluate([[THE, CAT, IS, ON, THE, MAT]], [[[THE, CAT, IS]]])
    assert abs(ev["corpus"][0] - 0.5) < 1e-9


def test_closest_length_tie_goes_to_the_shorter():
    h = [THE] * 5
    assert R.bleu_stats(h, [[CAT] * 7, [CAT] * 3])[9] == 3
    assert R.bleu_stats(h, [[CAT] * 3, [CAT] * 7])[9] == 3
    assert R.bleu_stats(h, [[CAT] * 7, [CAT] * 4, [CAT] * 6])[9] == 4
    assert R.bleu_stats(h, [[CAT] * 9, [CAT] * 6])[9] == 6


def test_lcs_and_rouge_by_inspection():
    assert R.lcs([1, 2, 3, 4, 5], [2, 4, 5, 9]) == 3                          # 2 4 5
    assert R.lcs([1, 2, 1, 2], [2, 1, 2, 1]) == 3
    assert R.lcs([1, 2, 3], [4, 5]) == 0 and R.lcs([], [1]) == 0
    # P = 3/5, R = 3/4, beta = 1.2
    want = (1 + 1.44) * 0.6 * 0.75 / (0.75 + 1.44 * 0.6)
    assert abs(R.rouge_l([1, 2, 3, 4, 5], [[2, 4, 5, 9]]) - want) < 1e-15
    # P and R are each maximised over the references
    want = (1 + 1.44) * 0.6 * 1.0 / (1.0 + 1.44 * 0.6)
    assert abs(R.rouge_l([1, 2, 3, 4, 5], [[2, 4, 5, 9], [1]]) - want) < 1e-15
    assert R.rouge_l([1, 2], [[3, 4]]) == 0.0


def test_document_frequency_counts_items_not_references():
    refs = [[[THE, CAT], [THE, CAT], [THE, DOG]], [[THE, MAT]], [[A, DOG]]]
    df = R.document_frequency(refs)
    assert df[0][(THE,)] == 2 and df[0][(CAT,)] == 1 and df[0][(DOG,)] == 2 and df[1][(THE, CAT)] == 1
    d = R.df_of_ref(refs, df, 3, 2)
    assert d[0, 0, 0].tolist() == [2, 1, 0, 0] and d[0, 0, 1].tolist() == [1, 0, 0, 0] and d[1, 1].tolist() == [[0] * 4] * 2
    # idf of an n-gram no reference holds: df 0 counts as 1
    ev = R.evaluate([[SAT], [THE], [THE]], refs)
    assert ev["cider"][0] == 0.0


def test_all_shared_corpus_gives_cider_zero():
    s = [THE, CAT, IS, ON, THE, MAT]
    ev = R.evaluate([s] * 3, [[s]] * 3)
    assert ev["cider"].tolist() == [0.0] * 3 and ev["corpus"][5] == 0.0
    assert R.evaluate([s], [[s]])["corpus"][5] == 0.0                          # Q = 1
    assert ev["rouge"].tolist() == [1.0] * 3


def test_empty_hypothesis_and_empty_reference():
    ev = R.evaluate([[], [THE, CAT]], [[[THE, CAT]], [[]]])
    assert ev["stats"].tolist() == [[0, 0, 0, 0, 0, 0, 0, 0, 0, 2], [2, 1, 0, 0, 0, 0, 0, 0, 2, 0]]
    assert ev["rouge"].tolist() == [0.0, 0.0] and ev["cider"].tolist() == [0.0, 0.0]
    assert np.all(np.isfinite(ev["corpus"]))
    ev = R.evaluate([[]], [[[]]])
    assert np.all(np.isfinite(ev["corpus"])) and ev["corpus"][4] == 0.0


def test_cider_by_hand():
    # Q = 2; item 0: h = [the cat], r = [the dog]; item 1 references [a].  df(the) = df(cat)... only unigrams and one bigram matter.
    ev = R.evaluate([[THE, CAT], [A]], [[[THE, DOG]], [[A]]])
    l2 = math.log(2.0)
    # order 1: v_h = {the: l2, cat: l2 (df 0 -> 1)}, v_r = {the: l2, dog: l2}; sim = l2^2 / (2 l2^2) = 1/2; orders 2: no shared bigram; 3, 4: none
    assert abs(ev["cider"][0] - 10.0 * 0.5 / 4.0) < 1e-12
    assert abs(ev["cider"][1] - 10.0 * 1.0 / 4.0) < 1e-12                     # [a] == [a]: order 1 alone exists
