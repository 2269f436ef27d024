"""The definition of the corpus metrics (include/mtn_hip.h mtn_eval_metrics), written the slow obvious way: no torch, Python ints and
floats (IEEE doubles), collections.Counter and a textbook LCS table.  BLEU-1..4, ROUGE-L and CIDEr (the clipped, length-penalised form
coco-caption prints as "CIDEr") of Q items, each one hypothesis against its references, all of them lists of token ids.  The kernel's
integers must equal these; its doubles are held within 1e-9.  Also: seeded generators of corpora."""
import math
import random
from collections import Counter

import numpy as np

MAX_REF, MAX_LEN = 8, 128


def grams(s, n):
    return Counter(tuple(s[p:p + n]) for p in range(len(s) - n + 1))


def bleu_stats(h, refs):
    """[guess_1..4, match_1..4, len(h), closest]: the item's ten integers."""
    guess, match = [], []
    for n in range(1, 5):
        gh = grams(h, n)
        best = Counter()
        for r in refs:                                           # the max over the references, then the clip
            for g, c in grams(r, n).items():
                best[g] = max(best[g], c)
        guess.append(max(len(h) - n + 1, 0))
        match.append(sum(min(c, best[g]) for g, c in gh.items()))
    closest = min((abs(len(r) - len(h)), len(r)) for r in refs)[1]
    return guess + match + [len(h), closest]


def bleu_corpus(stats):
    """([Bleu_1..4], T, C) from the items' integers."""
    tot = [sum(int(s[k]) for s in stats) for k in range(10)]
    T, C = tot[8], tot[9]
    ratio = (T + 1e-15) / (C + 1e-9)
    out, p = [], 1.0
    for n in range(1, 5):
        p = p * ((tot[3 + n] + 1e-15) / (tot[n - 1] + 1e-9))
        b = p ** (1.0 / n)
        out.append(b * math.exp(1.0 - 1.0 / ratio) if ratio < 1 else b)
    return out, T, C


def lcs(a, b):
    t = [[0] * (len(b) + 1) for _ in range(len(a) + 1)]
    for i in range(1, len(a) + 1):
        for j in range(1, len(b) + 1):
            t[i][j] = t[i - 1][j - 1] + 1 if a[i - 1] == b[j - 1] else max(t[i - 1][j], t[i][j - 1])
    return t[len(a)][len(b)]


def rouge_l(h, refs, beta=1.2):
    if not h:
        return 0.0
    ls = [lcs(h, r) for r in refs]
    p = max(l / float(len(h)) for l in ls)
    rc = max((l / float(len(r)) if r else 0.0) for l, r in zip(ls, refs))
    if p == 0 or rc == 0:
        return 0.0
    return (1 + beta ** 2) * p * rc / (rc + beta ** 2 * p)


def document_frequency(ref_sets):
    """df[n-1][g]: the number of ITEMS whose reference set holds the n-gram g at least once."""
    df = [Counter() for _ in range(4)]
    for refs in ref_sets:
        for n in range(1, 5):
            seen = set()
            for r in refs:
                seen.update(grams(r, n))
            df[n - 1].update(seen)
    return df


def cider(h, refs, df, Q):
    def vec(s, n):
        return {g: c * (math.log(Q) - math.log(max(1, df[n - 1][g]))) for g, c in grams(s, n).items()}

    total = 0.0
    for n in range(1, 5):
        vh = vec(h, n)
        nh = math.sqrt(sum(v * v for v in vh.values()))
        acc = 0.0
        for r in refs:
            vr = vec(r, n)
            nr = math.sqrt(sum(v * v for v in vr.values()))
            sim = sum(min(v, vr.get(g, 0.0)) * vr.get(g, 0.0) for g, v in vh.items())
            if nh != 0 and nr != 0:
                sim = sim / (nh * nr)
            d = float(len(h) - len(r))
            acc += sim * math.exp(-(d * d) / (2 * 6.0 ** 2))
        total += acc / len(refs)
    return 10.0 * (total / 4.0)


def df_of_ref(ref_sets, df, R, L):
    """[Q][R][L][4]: the df of the n-gram that starts at each reference position, 0 where there is none."""
    out = np.zeros((len(ref_sets), R, L, 4), dtype=np.int32)
    for q, refs in enumerate(ref_sets):
        for r, s in enumerate(refs):
            for n in range(1, 5):
                for p in range(len(s) - n + 1):
                    out[q, r, p, n - 1] = df[n - 1][tuple(s[p:p + n])]
    return out


def evaluate(hyps, ref_sets):
    """dict(stats int32 [Q][10], rouge [Q], cider [Q], corpus [8] = Bleu_1..4, ROUGE_L, CIDEr, T, C, df = the tables) of a corpus:
    hyps[q] a token list, ref_sets[q] its 1..8 reference token lists."""
    hyps = [[int(t) for t in h] for h in hyps]
    ref_sets = [[[int(t) for t in r] for r in refs] for refs in ref_sets]
    assert len(hyps) == len(ref_sets) >= 1 and all(1 <= len(refs) <= MAX_REF for refs in ref_sets)
    Q = len(hyps)
    df = document_frequency(ref_sets)
    stats = np.asarray([bleu_stats(h, refs) for h, refs in zip(hyps, ref_sets)], dtype=np.int32)
    rouge = np.asarray([rouge_l(h, refs) for h, refs in zip(hyps, ref_sets)], dtype=np.float64)
    cid = np.asarray([cider(h, refs, df, Q) for h, refs in zip(hyps, ref_sets)], dtype=np.float64)
    bleu, T, C = bleu_corpus(stats)
    corpus = np.asarray(bleu + [math.fsum(rouge) / Q, math.fsum(cid) / Q, float(T), float(C)], dtype=np.float64)
    return dict(stats=stats, rouge=rouge, cider=cid, corpus=corpus, df=df)


NAMES = ["Bleu_1", "Bleu_2", "Bleu_3", "Bleu_4", "ROUGE_L", "CIDEr"]


def as_result(ev):
    """The dict decode.evaluate_responses returns, from evaluate()'s."""
    out = {k: float(v) for k, v in zip(NAMES, ev["corpus"][:6])}
    out.update(hyp_len=int(ev["corpus"][6]), ref_len=int(ev["corpus"][7]), stats=ev["stats"], rouge=ev["rouge"], cider=ev["cider"])
    return out


def random_sentence(rng, lo, hi, n_values, base=0):
    return [base + rng.randrange(n_values) for _ in range(rng.randint(lo, hi))]


def random_corpus(seed, Q, lo, hi, n_values, refs=(1, 1), noise=0.3):
    """Q items: references of lo..hi tokens over n_values ids, the hypothesis a noisy copy of one of them (so that n-grams match)."""
    rng = random.Random(seed)
    hyps, ref_sets = [], []
    for _ in range(Q):
        rs = [random_sentence(rng, lo, hi, n_values) for _ in range(rng.randint(*refs))]
        src = list(rs[rng.randrange(len(rs))])
        h = [t if rng.random() >= noise else rng.randrange(n_values) for t in src]
        if h and rng.random() < 0.5:
            del h[rng.randrange(len(h))]
        hyps.append(h)
        ref_sets.append(rs)
    return hyps, ref_sets
