"""Ensemble decoding (decode.Ensemble) on the GPU: three small models (d_model 128, V 300; two of one block with different seeds, one of two
blocks), each with its generator bias shifted toward another token pair, decoded together for D = 2 dialogues with beam 4, max_len 16, in
bf16 (every member on the persistent step: the search is ONE captured graph with csrc/ensemble.hip inside) and fp32 (launch-per-sublayer
pass).  Non-vacuity (asserted by the fixture): the ensemble's best hypothesis of every dialogue differs from each member's own.

Bars, the project's own for the same pairs of paths (tests/test_decode_gpu.py, tests/test_constrain_decode_gpu.py): the captured search
against the same session stepped from the host — equal; against use_graph=False and (fp32) kv_cache=True — identical n-best tokens, scores
within 1e-3; the bf16 persistent step against MTN_DECODE_MEGA=0 — best score within 1e-2 x max(1, |score|).  The combination itself, in
prob mode: every returned hypothesis' score against the float64 combination of the MEMBERS' own token log-probabilities
(score_candidates(member)), fp32 within 1e-3, bf16 within 1e-2 x max(1, |score|)."""
import copy

import numpy as np
import pytest
import torch

from tests.constrain_refs import has_repeated_ngram

pytestmark = pytest.mark.gpu
V, SOS, UNK, EOS, PAD = 300, 2, 0, 3, 1
D_, BEAM, MAXLEN, MINLEN, PENALTY = 2, 4, 16, 4, 1.0
# (seed, blocks, the token pair its generator bias is shifted toward)
MEMBERS = [(4, 1, (11, 29)), (5, 1, (37, 53)), (6, 2, (71, 97))]
SHIFT = 6.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


def _model(dev, dtype, seed, blocks, pair, shift=SHIFT, vocab=V):
    from mtn_amd import make_model
    torch.manual_seed(seed)
    m = make_model(vocab, vocab, N=blocks, d_model=128, d_ff=256, h=4, dropout=0.1, ft_sizes=[64, 32], diff_encoder=True, auto_encoder_ft="query",
                   compute_dtype=dtype)
    with torch.no_grad():
        m.generator.proj.bias[list(pair)] += shift
    return m.to(dev).eval()


def _batch(dev, seed=50, n=D_):
    from mtn_amd.synthetic import synthetic_batch
    return synthetic_batch(V, n, 9, 30, 14, 8, [11, 7], [64, 32], device=dev, seed=seed, ragged=True)


def _one(b, d):
    """Dialogue d of a batch as a batch of its own (same padding, same masks)."""
    o, s = copy.copy(b), slice(d, d + 1)
    for name in ("query", "query_mask", "his", "his_mask", "cap", "cap_mask"):
        setattr(o, name, getattr(b, name)[s].clone())
    o.fts, o.fts_mask = [f[s].clone() for f in b.fts], [m[s].clone() for m in b.fts_mask]
    return o


def _beam(model, b, **kw):
    from mtn_amd import decode as D
    return D.beam_search_decode_many(model, b, MAXLEN, SOS, UNK, EOS, PAD, beam=BEAM, penalty=PENALTY, nbest=4, min_len=MINLEN, **kw)


def _tol(dtype, score):
    return 1e-3 if dtype == torch.float32 else 1e-2 * max(1.0, abs(score))


@pytest.fixture(scope="module", params=[torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def setup(request, dev):
    from mtn_amd import decode as D
    D._SESSIONS.clear()
    dtype = request.param
    members = [_model(dev, dtype, *m) for m in MEMBERS]
    b = _batch(dev)
    ens = D.Ensemble(members)
    own = [_beam(m, b) for m in members]
    res = _beam(ens, b)
    # non-vacuity — a condition of every test below: the ensemble's best hypothesis of EVERY dialogue is none of its members' own
    for d in range(D_):
        best = res[d][0][0][0]
        assert len(best) >= MINLEN - 1
        for k, o in enumerate(own):
            assert best != o[d][0][0][0], (d, k, best)
    assert [t for t, _ in own[0][0][0]] != [t for t, _ in own[1][0][0]]      # members 0 and 1 disagree with each other (the (1, 0) identity)
    yield ens, members, b, dtype, res, own
    D._SESSIONS.clear()


def _member_token_logps(members, b, hyps_per_dialogue):
    """Per member, per dialogue, per hypothesis: token_logp ([c..., <eos>]) from score_candidates on the member ALONE."""
    from mtn_amd import decode as D
    return [D.score_candidates(m, b, hyps_per_dialogue, SOS, EOS, PAD, max_len=MAXLEN) for m in members]


def _prob_reference(per_member, weights, d, i, n=None):
    """float64: sum over the first n positions of log sum_m w_m exp(token_logp_m)."""
    lp = np.array([pm[d][i]["token_logp"] for pm in per_member], dtype=np.float64)        # (M, len + 1)
    w = np.asarray(weights, dtype=np.float64).reshape(-1, 1)
    tok = np.log((w * np.exp(lp)).sum(0))
    return tok[:n].sum() if n is not None else tok.sum(), tok


def test_paths_agree(setup, monkeypatch):
    from mtn_amd import decode as D
    ens, members, b, dtype, res, _ = setup
    assert len(res) == D_ and _beam(ens, b) == res
    for nbest, best in res:
        assert len(nbest) == 4 and best == nbest[0][1]
        for toks, score in nbest:
            assert UNK not in toks and EOS not in toks and score == score and len(toks) >= MINLEN - 1
    if dtype == torch.bfloat16:
        mega = [s[0] for s in D._SESSIONS.values() if isinstance(s[0], D.EnsembleMegaSession) and s[0].width == BEAM]
        assert mega and getattr(mega[0], "_search_key", None) is not None, "the ensemble search did not run as the captured graph"
        assert len(mega[0].members) == len(members) and not mega[0].timed_out() and not any(s.timed_out() for s in mega[0].members)
        blk = mega[0]._devblk.data_ptr()
        assert all(s._args.tokens == blk for s in mega[0].members), "the members do not read one [tokens | pos | anc] block"
        fallbacks = D.MegaDecodeSession.FALLBACKS
        # the same session stepped from the host: the per-step kernels are the same, so everything is EQUAL
        with monkeypatch.context() as mp:
            mp.setattr(D.MegaDecodeSession, "search", lambda self, *a, **k: None)
            assert _beam(ens, b) == res
        assert D.MegaDecodeSession.FALLBACKS == fallbacks
    else:
        assert any(isinstance(s[0], D.EnsembleSession) for s in D._SESSIONS.values())
        assert not any(isinstance(s[0], D.MegaDecodeSession) for s in D._SESSIONS.values())
    assert _beam(ens, b) == res                                              # the cached session, loaded again
    eager = _beam(ens, b, use_graph=False)
    for (n1, b1), (n0, b0) in zip(res, eager):
        assert [t for t, _ in n1] == [t for t, _ in n0]
        assert max(abs(x[1] - y[1]) for x, y in zip(n1, n0)) < 1e-3 and abs(b1 - b0) < 1e-3
    if dtype == torch.float32:
        cached = _beam(ens, b, kv_cache=True)
        for (n1, b1), (n0, b0) in zip(res, cached):
            assert [t for t, _ in n1] == [t for t, _ in n0]
            assert max(abs(x[1] - y[1]) for x, y in zip(n1, n0)) < 1e-3 and abs(b1 - b0) < 1e-3


def test_bf16_persistent_step_and_launch_path_agree(dev, monkeypatch):
    from mtn_amd import decode as D
    D._SESSIONS.clear()
    ens, b = D.Ensemble([_model(dev, torch.bfloat16, *m) for m in MEMBERS]), _batch(dev)
    res = _beam(ens, b)
    assert any(isinstance(s[0], D.EnsembleMegaSession) for s in D._SESSIONS.values()), "the persistent step was not taken"
    with monkeypatch.context() as mp:
        mp.setenv("MTN_DECODE_MEGA", "0")
        D._SESSIONS.clear()
        launch = _beam(ens, b)
        assert not any(isinstance(s[0], D.MegaDecodeSession) for s in D._SESSIONS.values())
        assert any(isinstance(s[0], D.EnsembleSession) for s in D._SESSIONS.values())
    D._SESSIONS.clear()
    for (n1, b1), (n0, b0) in zip(res, launch):
        assert len(n1) == len(n0)
        assert abs(b1 - b0) < 1e-2 * max(1.0, abs(b0))


def test_scores_are_the_prob_combination_of_the_members(setup, monkeypatch):
    from mtn_amd import decode as D
    ens, members, b, dtype, res, _ = setup
    w = ens.weights
    # beam search: every hypothesis of every n-best list
    hyps = [[t for t, _ in nbest] for nbest, _ in res]
    per_member = _member_token_logps(members, b, hyps)
    combined = D.score_candidates(ens, b, hyps, SOS, EOS, PAD, penalty=PENALTY, max_len=MAXLEN)
    worst = 0.0
    for d, (nbest, _) in enumerate(res):
        for i, (toks, score) in enumerate(nbest):
            ref, tok = _prob_reference(per_member, w, d, i)
            ref += PENALTY * (len(toks) + 1)
            worst = max(worst, abs(score - ref) / (_tol(dtype, ref)))
            assert abs(score - ref) <= _tol(dtype, ref), (d, i, score, ref)
            c = combined[d][i]
            assert c["n_tokens"] == len(toks) + 1 and abs(c["score"] - ref) <= _tol(dtype, ref)
            assert max(abs(x - y) for x, y in zip(c["token_logp"], tok)) <= _tol(dtype, 1.0), (d, i)
    print(f"beam: worst |score - reference| / bar = {worst:.3g}")
    # greedy: the ensemble's arg-max at every step (rank 0 under the ensemble's own scoring), token log-probabilities = the combination
    ys = D.greedy_decode_many(ens, b, MAXLEN, SOS, PAD).tolist()
    assert all(y[0] == SOS and len(y) == MAXLEN for y in ys)
    g_hyps = [[y[1:]] for y in ys]
    g_members = _member_token_logps(members, b, g_hyps)
    g_comb = D.score_candidates(ens, b, g_hyps, SOS, EOS, PAD, max_len=MAXLEN)
    for d in range(D_):
        _, tok = _prob_reference(g_members, w, d, 0)
        c = g_comb[d][0]
        assert max(abs(x - y) for x, y in zip(c["token_logp"], tok)) <= _tol(dtype, 1.0)
        ranks = c["token_rank"][:MAXLEN - 1]                                   # (the last position is the <eos> the scoring appends)
        if dtype == torch.float32:
            assert ranks == [0] * (MAXLEN - 1), ranks
    if dtype == torch.bfloat16:
        # bf16: that greedy ran on the persistent step, the scoring runs on the launch-per-sublayer pass.  On ONE path the rank is 0
        # everywhere: greedy again with the persistent step off, scored by the same pass
        with monkeypatch.context() as mp:
            mp.setenv("MTN_DECODE_MEGA", "0")
            ys0 = D.greedy_decode_many(ens, b, MAXLEN, SOS, PAD).tolist()
        c0 = D.score_candidates(ens, b, [[y[1:]] for y in ys0], SOS, EOS, PAD, max_len=MAXLEN)
        for d in range(D_):
            assert c0[d][0]["token_rank"][:MAXLEN - 1] == [0] * (MAXLEN - 1), (d, c0[d][0]["token_rank"])
        # ... and across the two paths a rank other than 0 is a near-tie: the launch pass' own row at that position (the ensemble's
        # session stepped from the host on the persistent step's prefix) has its maximum within the bf16 bar of the chosen token
        sess = D.EnsembleSession(ens, b, MAXLEN, 1, pad=PAD, use_graph=False)
        swapped = 0
        for j in range(MAXLEN - 1):
            if all(g_comb[d][0]["token_rank"][j] == 0 for d in range(D_)):
                continue
            rows = sess.step_many([[ys[d][:j + 1]] for d in range(D_)])
            for d in range(D_):
                if g_comb[d][0]["token_rank"][j] != 0:
                    row = rows[d][0].double().cpu()
                    top, chosen = float(row.max()), float(row[ys[d][j + 1]])
                    assert top - chosen <= 1e-2 * max(1.0, abs(top)), (d, j, top, chosen)
                    swapped += 1
        print(f"bf16 greedy: {swapped} of {D_ * (MAXLEN - 1)} positions rank != 0 across the two paths")
    # samples: S = 3 per dialogue; score = the drawn tokens' combined log-probabilities (<eos> included where drawn)
    trace = []
    skw = dict(samples=3, temperature=1.0, seed=7, banned=(UNK, PAD, SOS), min_len=2)
    drawn = D.sample_decode_many(ens, b, MAXLEN, SOS, EOS, PAD, trace=trace, **skw)
    assert len(drawn) == D_ and all(len(h) == 3 for h in drawn)
    s_hyps = [[t for t, _ in h] for h in drawn]
    s_members = _member_token_logps(members, b, s_hyps)
    for d, h in enumerate(drawn):
        for i, (toks, score) in enumerate(h):
            ended = len(toks) < MAXLEN - 1                                      # (a row without <eos> keeps max_len - 1 tokens)
            ref, _ = _prob_reference(s_members, w, d, i, n=None if ended else len(toks))
            assert abs(score - ref) <= _tol(dtype, ref), (d, i, score, ref)


def test_identities(setup, dev):
    from mtn_amd import decode as D
    ens, members, b, dtype, res, own = setup
    m0, m1 = members[0], members[1]
    for mode in ("prob", "logprob"):
        twin = _beam(D.Ensemble([m0, copy.deepcopy(m0)], mode=mode), b)
        for (n1, _), (n0, _) in zip(twin, own[0]):
            assert [t for t, _ in n1] == [t for t, _ in n0], mode
            assert max(abs(x[1] - y[1]) for x, y in zip(n1, n0)) < 1e-3
    solo = _beam(D.Ensemble([m0, m1], weights=[1, 0]), b)
    for (n1, _), (n0, _) in zip(solo, own[0]):
        assert [t for t, _ in n1] == [t for t, _ in n0]
        assert max(abs(x[1] - y[1]) for x, y in zip(n1, n0)) < 1e-3
    other = _beam(D.Ensemble([m0, m1], weights=[0, 2.5]), b)
    for (n1, _), (n0, _) in zip(other, own[1]):
        assert [t for t, _ in n1] == [t for t, _ in n0]
    lg = _beam(D.Ensemble(members, mode="logprob"), b)                          # the other mode: a search of its own, valid n-best lists
    assert all(len(nb) == 4 and sc == sc and UNK not in t and EOS not in t for nb, _ in lg for t, sc in nb)


def test_constraints_compose_and_sampling_keys(setup):
    from mtn_amd import decode as D
    ens, members, b, dtype, res, _ = setup
    con = _beam(ens, b, no_repeat_ngram=2)
    for nbest, _ in con:
        for toks, _ in nbest:
            assert not has_repeated_ngram(toks, 2), toks
    ys = D.greedy_decode_many(ens, b, MAXLEN, SOS, PAD, no_repeat_ngram=2).tolist()
    assert all(not has_repeated_ngram(y[1:], 2) for y in ys)
    assert any(has_repeated_ngram(y[1:], 2) for y in D.greedy_decode_many(ens, b, MAXLEN, SOS, PAD).tolist())       # non-vacuity
    # sampling: a dialogue's stream is a function of (seed, key, position) — the same draws alone (D = 1) and in the batch (D = 2)
    skw = dict(samples=3, temperature=1.0, seed=11, banned=(UNK, PAD, SOS), min_len=2)
    t2 = []
    both = D.sample_decode_many(ens, b, MAXLEN, SOS, EOS, PAD, trace=t2, **skw)
    assert D.sample_decode_many(ens, b, MAXLEN, SOS, EOS, PAD, **skw) == both
    S = skw["samples"]
    for d in range(D_):
        t1 = []
        alone = D.sample_decode_many(ens, _one(b, d), MAXLEN, SOS, EOS, PAD, keys=[d], trace=t1, **skw)[0]
        assert t1[0][0] == t2[0][0][d * S:d * S + S]                                          # the rows' keys
        assert np.array_equal(t1[0][3].view(np.int32), t2[0][3][:, d * S:d * S + S].view(np.int32))     # the uniforms drawn: bitwise
        if dtype == torch.float32:         # (where a row's arithmetic does not depend on the rows beside it: the same tokens, too)
            assert [t for t, _ in alone] == [t for t, _ in both[d]], d
            assert max(abs(x[1] - y[1]) for x, y in zip(alone, both[d])) < 1e-3
        else:
            # bf16 (persistent step at 3 and at 6 rows): every sample drawn alone scores what the members alone give its tokens, and a
            # sample whose tokens came out the same in the batch has the same score, both within the bf16 bar
            one = _one(b, d)
            per_member = _member_token_logps(members, one, [[t for t, _ in alone]])
            for i, (toks, score) in enumerate(alone):
                ended = len(toks) < MAXLEN - 1
                ref, _ = _prob_reference(per_member, ens.weights, 0, i, n=None if ended else len(toks))
                assert abs(score - ref) <= _tol(dtype, ref), (d, i, score, ref)
                for toks2, score2 in both[d]:
                    if toks2 == toks:
                        assert abs(score - score2) <= _tol(dtype, score2)


def test_misuse_is_refused(setup, dev):
    from mtn_amd import decode as D
    ens, members, b, dtype, _, _ = setup
    m0 = members[0]
    with pytest.raises(ValueError):
        D.Ensemble([m0, m0])
    with pytest.raises(ValueError):
        D.Ensemble([])
    with pytest.raises(ValueError):
        D.Ensemble([m0] + [copy.copy(m0) for _ in range(8)])                    # 9 members
    with pytest.raises(ValueError):
        D.Ensemble([m0, _model(dev, dtype, 9, 1, (5, 6), vocab=V + 4)])         # another vocabulary size
    for bad in ([1.0], [1.0, -1.0], [0.0, 0.0], [float("nan"), 1.0]):
        with pytest.raises(ValueError):
            D.Ensemble(members[:2], weights=bad)
    with pytest.raises(ValueError):
        D.Ensemble(members[:2], mode="mean")


def test_session_cache_holds_an_ensemble_as_one_entry(setup):
    from mtn_amd import decode as D
    ens, members, b, dtype, res, _ = setup
    D._SESSIONS.clear()
    assert _beam(ens, b) == res
    assert len(D._SESSIONS) == 1                                                # the members' sessions live inside it
    sess = next(iter(D._SESSIONS.values()))[0]
    assert _beam(D.Ensemble(members), b) == res and next(iter(D._SESSIONS.values()))[0] is sess     # the same members and weights: reused
    _beam(D.Ensemble(members, weights=[2, 1, 1]), b)
    assert len(D._SESSIONS) == 2                                                # other weights are frozen into another graph
    # a member's weights replaced (prepare() sees the parameters' versions move): the entry is stale and built again
    n = len(D._SESSIONS)
    with torch.no_grad():
        members[2].generator.proj.bias[5] += 1.0
    try:
        _beam(ens, b)
        assert len(D._SESSIONS) == n
        fresh = [s[0] for s in D._SESSIONS.values() if s[0].model.weights == ens.weights]
        assert len(fresh) == 1 and fresh[0] is not sess
    finally:
        with torch.no_grad():
            members[2].generator.proj.bias[5] -= 1.0
        D._SESSIONS.clear()
