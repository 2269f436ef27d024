"""The definition of minimum-Bayes-risk selection (include/mtn_hip.h mtn_mbr_select), written the slow obvious way: no torch, Python
floats (IEEE doubles; a Python `a + w * u` is one multiply then one add, never an fma) and collections.Counter.  The kernel must agree
with this bit for bit.  Also: the host cut of a sample log, the `score` weights of decode.mbr_rerank, and seeded generators of sets."""
import math
import random
from collections import Counter

import numpy as np


def grams(h, n):
    return Counter(tuple(h[p:p + n]) for p in range(len(h) - n + 1))


def utility(h, r, N):
    """U(h, r) = (F_1 + .. + F_N) / N with F_n = 2 m_n / (c_n(h) + c_n(r)), 0.0 where that denominator is 0."""
    u = 0.0
    for n in range(1, N + 1):
        gh, gr = grams(h, n), grams(r, n)
        m = sum(min(c, gr[g]) for g, c in gh.items())
        den = max(len(h) - n + 1, 0) + max(len(r) - n + 1, 0)
        u = u + (float(2 * m) / float(den) if den else 0.0)
    return u / float(N)


def utility_by_occurrence(h, r, N):
    """The same number another way: occurrence number k (by position) of a gram in h counts iff r holds more than k of it."""
    u = 0.0
    for n in range(1, N + 1):
        m = 0
        for p in range(len(h) - n + 1):
            g = h[p:p + n]
            k = sum(1 for q in range(p) if h[q:q + n] == g)
            m += k < sum(1 for q in range(len(r) - n + 1) if r[q:q + n] == g)
        den = max(len(h) - n + 1, 0) + max(len(r) - n + 1, 0)
        u = u + (float(2 * m) / float(den) if den else 0.0)
    return u / float(N)


def select(hyps, N, w=None, K=None, util_fn=utility):
    """(util [K][K], expected [K], best, order [K]) of one set as numpy arrays; K >= len(hyps) pads as the kernel does (expected -1.0, order
    by ascending index behind the valid ones, util 0.0).  w None: uniform, 1.0 / n."""
    hyps = [[int(t) for t in h] for h in hyps]
    n = len(hyps)
    K = n if K is None else K
    assert n <= K
    w = ([1.0 / float(n)] * n if n else []) if w is None else [float(v) for v in w[:n]]
    util = np.zeros((K, K), dtype=np.float64)
    for i in range(n):
        for j in range(n):
            util[i, j] = util_fn(hyps[i], hyps[j], N)
    expected = np.full(K, -1.0, dtype=np.float64)
    for i in range(n):
        e = 0.0
        for j in range(n):
            e = e + w[j] * float(util[i, j])
        expected[i] = e
    order = np.arange(K, dtype=np.int32)
    for i in range(n):
        rank = sum(1 for j in range(n) if expected[j] > expected[i] or (expected[j] == expected[i] and j < i))
        order[rank] = i
    return util, expected, (int(order[0]) if n else -1), order


def cut_log(tok, eos):
    """The hypotheses of a sample log tok (L, columns), as decode.sample_decode_many cuts them: a column's tokens before its first <eos>,
    its first L - 1 tokens without one."""
    out = []
    for r in range(tok.shape[1]):
        col = [int(t) for t in tok[:, r]]
        out.append(col[:col.index(eos)] if eos in col else col[:len(col) - 1])
    return out


def score_weights(scores, temperature=1.0):
    """w_j = exp((s_j - max s) / temperature) / sum, in float64, the sum in ascending j."""
    top = max(scores)
    e = [math.exp((float(s) - float(top)) / float(temperature)) for s in scores]
    z = 0.0
    for v in e:
        z = z + v
    return [v / z for v in e]


def random_set(rng, K, max_len, n_values, min_len=0, base=0):
    """K hypotheses of lengths min_len..max_len over n_values token ids (few values: repeated n-grams, so clipping matters)."""
    return [[base + rng.randrange(n_values) for _ in range(rng.randint(min_len, max_len))] for _ in range(K)]


def sorted_weights(rng, K):
    """Random weights that sum to 1, largest first — an n-best list's shape: the model's favourite is index 0."""
    w = sorted((rng.random() for _ in range(K)), reverse=True)
    z = sum(w)
    return [v / z for v in w]


def seeded_sets(seed, count, K, max_len, n_values, min_len=0):
    rng = random.Random(seed)
    return [(random_set(rng, K, max_len, n_values, min_len), sorted_weights(rng, K)) for _ in range(count)]
