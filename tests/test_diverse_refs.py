"""The numpy definition of diverse beam search (tests/diverse_refs.py) held to what it extends and to itself: one group is decode._Beam
step by step, a hand-worked two-group step, head path = full-row path where nothing ties, the tie input is reported, and every seeded input
of tests/test_diverse_kernel_gpu.py is tie-free — the condition that keeps that test from passing through a fallback."""
import numpy as np
import pytest

from tests import diverse_refs as R

F32 = np.float32


def _run(V, D, B, G, lam, steps=R.KERNEL_STEPS, full=False, rows_of=None):
    st = R.State(D, B, G, R.KERNEL_L, R.START, R.PAD)
    k_top, k = B + 3, B // G + 2
    for l in range(steps):
        rows = rows_of(l) if rows_of else R.seeded_rows(V, D, B, G, l)
        if full:
            R.advance(st, k_top, k, R.UNK, R.EOS, R.PENALTY, R.MIN_LEN, lam, rows=rows)
        else:
            R.advance(st, k_top, k, R.UNK, R.EOS, R.PENALTY, R.MIN_LEN, lam, heads=R.heads_of(rows, k_top, R.EOS))
    return st


def _same(a, b):
    for name in ("tokens", "anc", "n_live", "step", "log_parent", "log_tok", "log_n_old", "log_n_new"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name
    for name in ("lp", "log_score", "log_done"):
        assert getattr(a, name).tobytes() == getattr(b, name).tobytes(), name
    assert a.pos == b.pos


@pytest.mark.parametrize("beam", [1, 3, 5])
def test_one_group_is_the_plain_beam(beam):
    from mtn_amd.decode import _Beam
    V, L = 300, R.KERNEL_L
    st = R.State(1, beam, 1, L, R.START, R.PAD)
    bm = _Beam(R.START, R.UNK, R.EOS, beam, R.PENALTY, R.MIN_LEN)
    k = beam + 2
    for l in range(6):
        rows = R.seeded_rows(V, 1, beam, 1, l, seed=5)
        heads = R.heads_of(rows, k + 1, R.EOS).astype("float64")
        n = len(bm.hyps)
        bm.advance(None, l, top=(heads[:n, :k], heads[:n, k + 1:2 * k + 1].astype("int64"), heads[:n, 2 * k + 2]))
        R.advance(st, k + 1, k, R.UNK, R.EOS, R.PENALTY, R.MIN_LEN, 0.0, heads=heads.astype(F32))
        assert st.flag == 0
        assert [h[0][-1] for h in bm.hyps] == st.tokens[:len(bm.hyps)].tolist()
        assert [h[1] for h in bm.hyps] == st.lp[:len(bm.hyps)].tolist()
        assert bm.parents == st.log_parent[l, :len(bm.hyps)].tolist()
    # the finished scores, in append order
    done = [float(st.log_done[l, h]) for l in range(R.MIN_LEN, 6) for h in range(int(st.log_n_old[l, 0]))]
    assert done == [s for _, s in bm.done]


def test_hand_worked_two_groups():
    """V = 8, B = 2, G = 2 (one hypothesis per group), lambda = 1, <unk> = 0, <eos> = 3.  Both groups read the same row at step 0:
    token 5 (-0.25) then 6 (-0.5) then 7 (-2).  Group 0 takes 5.  Group 1 sees 5 at -1.25, so it takes 6 with the unpenalised -0.5.  At
    step 1 group 0's row favours 6 (-0.125), group 1's row favours 6 as well (-0.25) over 4 (-1): penalised, 6 is at -1.25, so group 1 takes
    4 with -0.5 + -1 = -1.5."""
    row0 = np.array([-9, -9, -9, -4, -9, -0.25, -0.5, -2], dtype=F32)
    st = R.State(1, 2, 2, 4, 2, 1)
    R.advance(st, 5, 3, 0, 3, 1.0, 1, 1.0, heads=R.heads_of(np.stack([row0, row0]), 5, 3))
    assert st.tokens.tolist() == [5, 6] and st.lp.tolist() == [-0.25, -0.5]
    r0 = np.array([-9, -9, -9, -3, -8, -7, -0.125, -6], dtype=F32)
    r1 = np.array([-9, -9, -9, -5, -1, -7, -0.25, -6], dtype=F32)
    R.advance(st, 5, 3, 0, 3, 1.0, 1, 1.0, heads=R.heads_of(np.stack([r0, r1]), 5, 3))
    assert st.tokens.tolist() == [6, 4] and st.lp.tolist() == [-0.375, -1.5]
    assert st.log_parent[1].tolist() == [0, 0] and st.n_live.tolist() == [1, 1] and st.step.tolist() == [2, 2] and st.pos == 2
    # finished at step 1 (min_len 1): r[eos] + lp + penalty * 2, with the UNPENALISED <eos> value
    assert st.log_done[1].tolist() == [-3 - 0.25 + 2, -5 - 0.5 + 2]
    assert st.anc.tolist() == [[0, 0, 0, 0], [1, 1, 1, 1]]
    assert st.flag == 0                   # (no two equal values inside a head of 5, before or after the penalty)


@pytest.mark.parametrize("D,B,G", R.KERNEL_SHAPES)
@pytest.mark.parametrize("lam", R.KERNEL_LAMBDAS)
def test_head_path_equals_full_row_path_and_inputs_are_tie_free(D, B, G, lam):
    for V in R.KERNEL_V:
        heads = _run(V, D, B, G, lam)
        assert heads.flag == 0, "a seeded input of the kernel test holds a tie"
        _same(heads, _run(V, D, B, G, lam, full=True))
        if lam > 0:                       # the penalty is felt: otherwise these inputs would test nothing
            plain = _run(V, D, B, G, 0.0)
            assert not np.array_equal(plain.log_tok, heads.log_tok)


def test_large_penalty_keeps_groups_apart():
    st = _run(300, 2, 4, 4, 64.0)
    for l in range(R.KERNEL_STEPS):
        for d in range(2):
            toks = st.log_tok[l, d * 4:d * 4 + 4].tolist()
            assert len(set(toks)) == 4, toks


def test_multiples_of_half_report_a_tie():
    D, B, G = 1, 4, 2
    rows = R.tie_rows(300, D * B)
    assert _run(300, D, B, G, 0.5, steps=1, rows_of=lambda l: rows).flag == 1
    assert _run(300, D, B, G, 0.0, steps=1, rows_of=lambda l: rows).flag == 0          # the rows themselves hold none


def test_whole_search_pools_groups():
    """search() on rows that depend on the prefix only through its last token: the groups' finished hypotheses are pooled, identical token
    lists once, sorted by score; with one group and no penalty it is decode._Beam's search."""
    from mtn_amd.decode import _Beam
    V = 40
    table = R.seeded_rows(V, 1, V, 1, 0, seed=9)                              # row per last token

    def rows(prefix_lists):
        return [table[[p[-1] for p in pl]] for pl in prefix_lists]

    trace = []
    res = R.search(rows, 2, 4, 2, 0.5, 6, R.START, R.UNK, R.EOS, 1.0, 2, 4, trace=trace)
    assert len(res) == 2 and res[0] == res[1]
    nbest, best = res[0]
    assert len(nbest) == 4 and best == nbest[0][1] and [s for _, s in nbest] == sorted((s for _, s in nbest), reverse=True)
    assert len({tuple(t) for t, _ in nbest}) == 4
    assert [t[:3] for t in trace[:4]] == [(0, 0, 0), (0, 0, 1), (0, 1, 0), (0, 1, 1)]
    one = R.search(rows, 1, 3, 1, 0.0, 6, R.START, R.UNK, R.EOS, 1.0, 2, 3)[0]
    bm = _Beam(R.START, R.UNK, R.EOS, 3, 1.0, 2)
    for l in range(6):
        bm.advance(rows([bm.prefixes()])[0].astype("float64"), l)
    assert one == bm.result(3)
    assert R.pool([([1], -2.0), ([2], -1.0), ([1], -1.5), ([1], -1.5)], 5) == ([([2], -1.0), ([1], -1.5)], -1.0)
