"""The definitions behind self-critical sequence training (csrc/scst.hip; include/mtn_hip.h mtn_wlosshead_args, mtn_eval_rows_args,
mtn_scst_assemble_args, mtn_scst_advantage_args), written the slow obvious way in numpy float64 and Python; validated without a GPU by
tests/test_scst_refs.py and used on the device by tests/test_scst_kernel_gpu.py.  Plain helpers, no fixtures.

weighted_loss_head   the label-smoothed KL of a row (the smoothed target row td built explicitly, the lone-<pad> quirk of
                     label_smoothing.py:29 included) times coef / norm times the row's weight; the gradient is the closed form
                     gloss scale w (softmax sum(td) - td).  With weights of 1 it is row_refs.composed_loss (autograd through the oracle).
assemble             the cut rule of decode.sample_decode_many on a (L, rows) sample log, exact.
advantage            -(r - b): b a given baseline or the leave-one-out mean of the other rewards, summed in ascending s.
rewards              tests/eval_refs.py's per-item definitions with the document frequency of a FIXED corpus and Q = its size.
"""
import numpy as np

from tests import eval_refs as er


# ------------------------------------------------------------------------------------------ weighted loss head
def zeroed_rows(target, pad):
    """Rows label_smoothing.py:29 zeroes: <pad> rows, if the sum of their row indices is positive."""
    target = np.asarray(target)
    is_pad = target == pad
    return is_pad & (int((np.arange(target.size) * is_pad).sum()) > 0)


def smoothed_targets(target, V, pad, smoothing):
    target = np.asarray(target)
    td = np.full((target.size, V), smoothing / (V - 2), dtype=np.float64)
    td[np.arange(target.size), target] = 1.0 - smoothing
    td[:, pad] = 0.0
    td[zeroed_rows(target, pad)] = 0.0
    return td


def weighted_loss_head(logits, targets, weights, smoothings, V, pad, coef, norm, gloss):
    """float64.  logits [rows, V]; per segment: targets[s] int [n_s], weights[s] float [n_s] or None (ones), smoothings[s], coef[s],
    norm[s].  dict(lse [rows], rowloss [rows], total, dlogits [rows, V] = gloss * d total / d logits, zero [rows]: the rows that hold
    +0.0 everywhere (zeroed <pad> rows and zero weights), kl [rows]: the unweighted KL_ls)."""
    z = np.asarray(logits, dtype=np.float64)
    mx = z.max(1, keepdims=True)
    lse = (mx + np.log(np.exp(z - mx).sum(1, keepdims=True)))[:, 0]
    logp = z - lse[:, None]
    rowloss, dz, zero, kls, base = [], [], [], [], 0
    for s, t in enumerate(targets):
        t = np.asarray(t)
        n = t.size
        td = smoothed_targets(t, V, pad, smoothings[s])
        w = np.ones(n) if weights[s] is None else np.asarray(weights[s], dtype=np.float64)
        lp = logp[base:base + n]
        kl = (td * (np.log(np.where(td > 0, td, 1.0)) - lp)).sum(1)
        scale = float(coef[s]) / float(norm[s])
        rowloss.append(scale * w * kl)
        dz.append(gloss * scale * w[:, None] * (np.exp(lp) * td.sum(1, keepdims=True) - td))
        zero.append(zeroed_rows(t, pad) | (w == 0))
        kls.append(kl)
        base += n
    rowloss = np.concatenate(rowloss)
    return dict(lse=lse, rowloss=rowloss, total=float(rowloss.sum()), dlogits=np.concatenate(dz), zero=np.concatenate(zero),
                kl=np.concatenate(kls))


# ------------------------------------------------------------------------------------------ sample log -> targets
def cut_length(col, eos):
    """Tokens a sampled row keeps: those before its first <eos>; L - 1 of them without one (decode.sample_decode_many)."""
    col = [int(t) for t in col]
    return col.index(eos) if eos in col else len(col) - 1


def assemble(log_tok, sos, eos, pad, T=None):
    """log_tok int [L][rows] -> (trg int64 [rows][T], trg_y int64 [rows][T], hyp int32 [rows][L], hyp_len int32 [rows])."""
    log_tok = np.asarray(log_tok)
    L, rows = log_tok.shape
    T = L if T is None else T
    assert T >= L
    trg = np.full((rows, T), pad, dtype=np.int64)
    trg_y = np.full((rows, T), pad, dtype=np.int64)
    hyp = np.full((rows, L), pad, dtype=np.int32)
    hyp_len = np.zeros(rows, dtype=np.int32)
    for r in range(rows):
        n = cut_length(log_tok[:, r], eos)
        y = log_tok[:n, r]
        trg[r, 0] = sos
        trg[r, 1:n + 1] = y
        trg_y[r, :n] = y
        trg_y[r, n] = eos
        hyp[r, :n] = y
        hyp_len[r] = n
    return trg, trg_y, hyp, hyp_len


# ------------------------------------------------------------------------------------------ rewards -> row weights
def advantage(reward, T, baseline=None):
    """reward float64 [D][S] -> dict(adv [D][S] = r - b, base [D][S] = b, roww float32 [D * S][T] = -(r - b) on every target row,
    mean_reward, mean_baseline).  b: baseline[d], or the mean of the other S - 1 rewards of the dialogue summed in ascending s."""
    reward = np.asarray(reward, dtype=np.float64)
    D, S = reward.shape
    base = np.zeros((D, S), dtype=np.float64)
    for d in range(D):
        for s in range(S):
            if baseline is not None:
                base[d, s] = float(baseline[d])
            else:
                acc = 0.0
                for k in range(S):
                    if k != s:
                        acc += float(reward[d, k])
                base[d, s] = acc / float(S - 1)
    adv = reward - base
    roww = np.repeat((-adv).astype(np.float32).reshape(D * S, 1), T, axis=1)

    def mean(x):
        tot = 0.0
        for d in range(D):
            row = 0.0
            for s in range(S):
                row += float(x[d, s])
            tot += row
        return tot / float(D * S)

    return dict(adv=adv, base=base, roww=roww, mean_reward=mean(reward), mean_baseline=mean(base))


# ------------------------------------------------------------------------------------------ rewards against a fixed corpus
def rewards(hyps, items, ref_sets):
    """Hypothesis n (a token list) against corpus item items[n], df and Q from the whole corpus ``ref_sets``:
    dict(stats int32 [N][10], rouge [N], cider [N])."""
    ref_sets = [[[int(t) for t in r] for r in refs] for refs in ref_sets]
    df, Qc = er.document_frequency(ref_sets), len(ref_sets)
    hyps = [[int(t) for t in h] for h in hyps]
    stats = np.asarray([er.bleu_stats(h, ref_sets[i]) for h, i in zip(hyps, items)], dtype=np.int32)
    rouge = np.asarray([er.rouge_l(h, ref_sets[i]) for h, i in zip(hyps, items)], dtype=np.float64)
    cider = np.asarray([er.cider(h, ref_sets[i], df, Qc) for h, i in zip(hyps, items)], dtype=np.float64)
    return dict(stats=stats, rouge=rouge, cider=cider)


def pack_corpus(ref_sets, R, L, fill=-7):
    """(ref int32 [Q][R][L], ref_len int32 [Q][R], n_ref int32 [Q]) — what lies past a length or past n_ref holds ``fill``."""
    Q = len(ref_sets)
    ref = np.full((Q, R, L), fill, dtype=np.int32)
    ref_len = np.zeros((Q, R), dtype=np.int32)
    n_ref = np.zeros(Q, dtype=np.int32)
    for q, refs in enumerate(ref_sets):
        n_ref[q] = len(refs)
        for r, s in enumerate(refs):
            ref[q, r, :len(s)] = s
            ref_len[q, r] = len(s)
    return ref, ref_len, n_ref


def pack_rows(hyps, L, fill=-7):
    hyp = np.full((len(hyps), L), fill, dtype=np.int32)
    for n, h in enumerate(hyps):
        hyp[n, :len(h)] = h
    return hyp, np.asarray([len(h) for h in hyps], dtype=np.int32)


# ------------------------------------------------------------------------------------------ the kernel tests' cases
SEGS = (5, 1, 7)
COEF = (1.0, 0.7, 0.3)
NORM = (7.0, 13.0, 3.0)
GLOSS = 0.37
PAD = 1


def head_inputs(V, seed):
    """(logits float32 [13, V], targets per segment, weights per segment).  Segment 0: <pad> rows at 2 and 4 (zeroed), weights negative,
    zero, one, fractional.  Segment 1: ONE row whose target is <pad> — the quirk row (not zeroed), weight negative.  Segment 2: a <pad>
    row in the middle, the edge columns as targets, a zero weight on a live row and a negative one on the <pad> row."""
    rng = np.random.RandomState(seed)
    z = rng.randn(sum(SEGS), V).astype(np.float32) * 2.0
    t0 = np.array([5, V - 1, PAD, 0, PAD], dtype=np.int64)
    t1 = np.array([PAD], dtype=np.int64)
    t2 = np.array([7, 0, V - 1, PAD, 3, 2, V // 2], dtype=np.int64)
    w0 = np.array([-1.5, 0.0, 1.0, 0.25, -2.0], dtype=np.float32)
    w1 = np.array([-0.75], dtype=np.float32)
    w2 = np.array([1.0, -0.3, 0.0, -1.0, 2.5, 1.0, -0.0625], dtype=np.float32)
    return z, [t0, t1, t2], [w0, w1, w2]


def reward_corpus(seed=11, Qc=7, L=12):
    """(ref_sets, hyps, items): 7 items of 1..3 references of 2..L tokens over six ids; N = 10 hypotheses naming repeated and permuted
    items, of lengths 0, 1, 3 and L among them, noisy copies of a reference of their item so that n-grams match."""
    import random
    rng = random.Random(seed)
    _, ref_sets = er.random_corpus(seed, Qc, 2, L, 6, refs=(1, 3))
    ref_sets[0][0] = [rng.randrange(6) for _ in range(L)]            # a reference of full length
    items = [3, 0, 6, 3, 1, 0, 5, 2, 3, 4]
    lens = [0, 1, 3, L, 5, L, 3, 7, 1, 4]
    hyps = []
    for i, n in zip(items, lens):
        src = ref_sets[i][rng.randrange(len(ref_sets[i]))]
        h = [(src[k % len(src)] if rng.random() > 0.25 else rng.randrange(6)) for k in range(n)]
        hyps.append(h)
    return ref_sets, hyps, items


def assemble_log(eos=2, L=5):
    """A (L, 6) sample log that covers every cut case: <eos> at position 0, at L - 1, none, in the middle, twice (the first counts),
    and at position 1."""
    cols = [[eos, 9, 8, 7, 6], [4, 5, 6, 7, eos], [4, 5, 6, 7, 8], [9, 8, eos, 7, 6], [3, eos, 5, eos, 4], [7, eos, eos, eos, eos]]
    assert all(len(c) == L for c in cols)
    return np.asarray(cols, dtype=np.int32).T.copy()
