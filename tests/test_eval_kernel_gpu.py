"""mtn_eval_metrics (csrc/eval.hip) against its definition (tests/eval_refs.py) on the GPU.  Integers — the ten BLEU statistics per item,
the document frequency at every reference position, the corpus lengths T and C — are compared exactly.  Doubles are held within 1e-9
absolute: the values lie in [0, 10] and are sums of at most a few hundred double terms through log, sqrt and exp, so the expected error
is of order 1e-13, and the bar is six orders below the three decimals that are printed.  The cases are the smallest shapes at which each
part of the kernels can go wrong."""
import functools
import random

import numpy as np
import pytest
import torch

from tests import eval_refs as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-9


def _case(name):
    """(hyps, ref_sets, R, L, ldl): R and L are the launch's bounds, ldl its row stride."""
    rng = random.Random(sum(map(ord, name)))
    if name == "minimal":
        return [[7]], [[[7]]], 1, 1, 1
    if name == "lengths-below-n":                                # 0..3 tokens with n up to 4
        hyps = [[], [1], [1, 2], [1, 2, 3], [2, 3], [3], [1, 2, 3], []]
        refs = [[[1, 2]], [[]], [[1, 2, 3]], [[1, 2, 3], [2]], [[1, 2, 3], []], [[3], [3, 3]], [[], [1, 2, 3], [1]], [[]]]
        return hyps, refs, 3, 3, 3
    if name == "heavy-clipping":                                 # alphabet of 3: the max over the references comes before the clip
        hyps = [R.random_sentence(rng, 5, 12, 3) for _ in range(12)]
        refs = [[R.random_sentence(rng, 5, 12, 3) for _ in range(1 + q % 4)] for q in range(12)]
        return hyps, refs, 4, 12, 12
    if name == "closest-ties":                                   # reference lengths on both sides of the hypothesis at equal distance
        hyps = [R.random_sentence(rng, 6, 6, 8) for _ in range(6)]
        lens = [(8, 4), (4, 8), (9, 3, 7, 5), (5, 7, 6), (10, 2), (7, 7, 5)]
        refs = [[R.random_sentence(rng, l, l, 8) for l in ls] for ls in lens]
        return hyps, refs, 4, 10, 10
    if name == "largest":                                        # the worst case for the LCS, for LDS and for duplicate keys in one item
        hyps = [R.random_sentence(rng, 128, 128, 5) for _ in range(4)]
        refs = [[R.random_sentence(rng, 128, 128, 5) for _ in range(8)] for _ in range(4)]
        hyps[1], refs[1][3], refs[2][7] = [1, 2] * 64, [2, 1] * 64, [1, 2] * 64
        return hyps, refs, 8, 128, 128
    if name == "shared-table":                                   # most n-grams are contended by many workgroups
        hyps, refs = R.random_corpus(11, 300, 10, 30, 40, refs=(1, 2))
        return hyps, refs, 2, 30, 30
    if name == "table-load":                                     # 64 x 128 distinct tokens: the table at its densest
        refs = [[[q * 128 + p for p in range(128)]] for q in range(64)]
        hyps = [list(r[0]) for r in refs]
        for q in range(0, 64, 2):
            hyps[q] = hyps[q][::2] + refs[(q + 1) % 64][0][:20]
        return hyps, refs, 1, 128, 128
    if name == "wide-ids":                                       # compared as int32, nothing is an index
        vals = [2 ** 30 - 1, 2 ** 30, 2 ** 30 + 1, -2 ** 30, -2 ** 30 - 1, -2 ** 30 + 1, 2 ** 31 - 1, -2 ** 31, 0, -1]
        pick = lambda: [vals[rng.randrange(len(vals))] for _ in range(rng.randint(0, 12))]
        return [pick() for _ in range(10)], [[pick() for _ in range(rng.randint(1, 3))] for _ in range(10)], 3, 12, 12
    if name == "varying-n-ref":                                  # garbage past n_ref and past every length, ldl > L
        hyps = [R.random_sentence(rng, 0, 20, 6) for _ in range(16)]
        refs = [[R.random_sentence(rng, 0, 20, 6) for _ in range(1 + q % 8)] for q in range(16)]
        return hyps, refs, 8, 20, 27
    if name == "all-shared":
        s = R.random_sentence(rng, 17, 17, 6)
        return [list(s) for _ in range(5)], [[list(s)] for _ in range(5)], 1, 17, 17
    raise KeyError(name)


CASES = ["minimal", "lengths-below-n", "heavy-clipping", "closest-ties", "largest", "shared-table", "table-load", "wide-ids", "varying-n-ref",
         "all-shared"]


@functools.lru_cache(maxsize=None)
def _reference(name):
    hyps, refs, Rm, L, ldl = _case(name)
    ev = R.evaluate(hyps, refs)
    ev["df_of_ref"] = R.df_of_ref(refs, ev["df"], Rm, L)
    return hyps, refs, Rm, L, ldl, ev


def _pack(hyps, refs, Rm, L, ldl, garbage_seed=5):
    """Device tensors of a launch; every token past a length, every row past n_ref and every column past L holds garbage that occurs in
    the corpus (it would match if it were read)."""
    rng = np.random.RandomState(garbage_seed)
    Q = len(hyps)
    pool = np.asarray(sorted({t for h in hyps for t in h} | {t for rs in refs for r in rs for t in r} | {0}), dtype=np.int64)
    h = pool[rng.randint(0, len(pool), size=(Q, ldl))]
    r = pool[rng.randint(0, len(pool), size=(Q, Rm, ldl))]
    hl, rl = np.zeros(Q, dtype=np.int32), rng.randint(0, L + 1, size=(Q, Rm)).astype(np.int32)
    for q in range(Q):
        h[q, :len(hyps[q])] = hyps[q]
        hl[q] = len(hyps[q])
        for k, s in enumerate(refs[q]):
            r[q, k, :len(s)] = s
            rl[q, k] = len(s)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    n_ref = up(np.asarray([len(rs) for rs in refs], dtype=np.int32))
    return up(h.astype(np.int32))[:, :L], up(hl), up(r.astype(np.int32))[:, :, :L], up(rl), n_ref


def _launch(name, **kw):
    from mtn_amd import ops
    hyps, refs, Rm, L, ldl, _ = _reference(name)
    out = ops.eval_metrics(*_pack(hyps, refs, Rm, L, ldl), df_of_ref=True, **kw)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def _check(got, ev, n_ref=None):
    stats, rouge, cider, corpus, df = got
    assert np.array_equal(stats, ev["stats"])
    assert np.array_equal(df, ev["df_of_ref"])
    assert corpus[6] == ev["corpus"][6] and corpus[7] == ev["corpus"][7]
    errs = dict(rouge=np.abs(rouge - ev["rouge"]).max(), cider=np.abs(cider - ev["cider"]).max(), corpus=np.abs(corpus[:6] - ev["corpus"][:6]).max())
    print("largest absolute errors:", errs)
    assert all(np.isfinite(v) and v <= TOL for v in errs.values()), errs


@pytest.mark.parametrize("name", CASES)
def test_kernel_equals_the_definition(name):
    ev = _reference(name)[5]
    got = _launch(name)
    _check(got, ev)
    if name == "all-shared":
        assert got[2].tobytes() == np.zeros(len(got[2])).tobytes() and got[3][5].tobytes() == np.float64(0.0).tobytes()
    if name == "minimal":
        assert got[3][5] == 0.0 and got[1][0] == 1.0 and got[0][0].tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1, 1]


def test_two_launches_give_the_same_bytes():
    a, b = _launch("shared-table"), _launch("shared-table")
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_a_dirty_and_larger_workspace_changes_nothing():
    from mtn_amd import ops
    _, _, Rm, L, _, _ = _reference("shared-table")
    ws = torch.full((ops.eval_workspace_bytes(300, Rm, L) + 4096,), 0xA5, dtype=torch.uint8, device=DEV)
    a, b = _launch("shared-table"), _launch("shared-table", workspace=ws)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_an_items_stats_and_rouge_do_not_depend_on_its_company():
    from mtn_amd import ops
    hyps, refs, Rm, L, ldl, ev = _reference("shared-table")
    full = _launch("shared-table")
    keep = [3, 17, 120, 299]
    out = ops.eval_metrics(*_pack([hyps[q] for q in keep], [refs[q] for q in keep], Rm, L, ldl))
    stats, rouge = out[0].cpu().numpy(), out[1].cpu().numpy()
    assert np.array_equal(stats, full[0][keep]) and rouge.tobytes() == full[1][keep].tobytes()


def test_evaluate_responses_equals_the_direct_call():
    from mtn_amd import decode as D
    hyps, refs, _, _, _, ev = _reference("shared-table")
    direct = _launch("shared-table")
    res = D.evaluate_responses(hyps, refs)
    assert np.array_equal(res["stats"], direct[0]) and res["rouge"].tobytes() == direct[1].tobytes() and res["cider"].tobytes() == direct[2].tobytes()
    assert [res[k] for k in D.EVAL_NAMES] == direct[3][:6].tolist() and (res["hyp_len"], res["ref_len"]) == (int(direct[3][6]), int(direct[3][7]))
    assert np.array_equal(res["stats"], ev["stats"])
