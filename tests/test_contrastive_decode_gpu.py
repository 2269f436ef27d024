"""Contrastive search (--decode-style contrastive; decode.contrastive_decode_many) end to end on the GPU, on the checkpoint and the mini
test set of tests/test_generate_gpu.py, fp32 and bf16: k = 1 is greedy, alpha = 0 follows the row maxima, a traced eager search is held
step by step to the float64 definition (tests/contrastive_refs.py) on the very inputs the kernel read, the captured search gives the eager
search's logs byte for byte, the result JSON and the log are what the CLI promises, and a reused session equals a fresh one."""
import json
import logging

import numpy as np
import pytest
import torch

from tests import contrastive_refs as R
from tests.test_generate_gpu import MAXLEN, _argv, _logged_hyps, _reference_side, run  # noqa: F401  (run: the module-scoped fixture)

pytestmark = pytest.mark.gpu
K, ALPHA = 5, 0.6
BAR = {"fp32": 1e-3, "bf16": 1e-2}                       # the project's parity bar on log-probabilities


def _main(run, style, dtype, out, extra, caplog):
    from mtn_amd import decode as D
    from mtn_amd import generate as G
    D._SESSIONS.clear()
    caplog.clear()
    caplog.set_level(logging.INFO)
    result = G.main(_argv(run, style, dtype, 0, str(run["tmp"] / out)) + extra)
    assert json.load(open(str(run["tmp"] / out))) == result
    return result, _logged_hyps(caplog.records)


def _turns(result):
    return [t for d in result["dialogs"] for t in d["dialog"]]


def _batch_of(data, corpus, vocab, ids):
    """QAs ``ids`` side by side at their common padded shape."""
    from mtn_amd import data_handler as dh
    idx, _ = dh.make_batch_indices(data, 1, separate_caption=True)
    lens = [idx[i] for i in ids]
    ix = ([data["dialogs"][i][0] for i in ids], list(ids), [max(l[2][f] for l in lens) for f in range(len(lens[0][2]))],
          max(l[3] for l in lens), max(l[4] for l in lens), max(l[5] for l in lens), max(l[6] for l in lens), len(ids))
    return dh.make_batch(corpus, ix, vocab, separate_caption=True)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_k_one_reproduces_greedy(run, dtype, caplog, monkeypatch):
    """One candidate per position is the arg-max for every alpha: the answers of the result JSON are greedy's, both searches on the
    launch-per-sublayer pass at one dialogue per search.  (--min-length 0: greedy may end a response at once.)"""
    monkeypatch.setenv("MTN_DECODE_MEGA", "0")
    from mtn_amd import decode as D
    greedy, g_log = _main(run, "greedy", dtype, "cs_greedy_%s.json" % dtype, ["--dialogues-per-search", "1"], caplog)
    assert not any(isinstance(s[0], D.MegaDecodeSession) for s in D._SESSIONS.values())
    cs, c_log = _main(run, "contrastive", dtype, "cs_k1_%s.json" % dtype,
                      ["--dialogues-per-search", "1", "--contrastive-k", "1", "--contrastive-alpha", "0.6", "--min-length", "0"], caplog)
    assert [t["answer"] for t in _turns(cs)] == [t["answer"] for t in _turns(greedy)]
    assert c_log == g_log and all(isinstance(h, str) for h in c_log)          # greedy's HYP: line
    assert all("contrastive" not in t for t in _turns(greedy))               # without the style the JSON is what it was
    assert all(set(t["contrastive"]) == {"score", "logp", "penalty", "rank"} and set(t["contrastive"]["rank"]) <= {0} for t in _turns(cs))


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_alpha_zero_follows_the_row_maxima(run, dtype, caplog, monkeypatch):
    """--contrastive-alpha 0 --contrastive-k 5: every chosen token's log-probability is within the parity bar of the largest admitted one
    of the row a single-QA, unpadded DecodeSession.step gives for its own prefix."""
    monkeypatch.setenv("MTN_DECODE_MEGA", "0")
    from mtn_amd import data_handler as dh
    from mtn_amd import decode as D
    cs, _ = _main(run, "contrastive", dtype, "cs_a0_%s.json" % dtype, ["--contrastive-k", "5", "--contrastive-alpha", "0"], caplog)
    vocab, _, data, corpus, model, _ = _reference_side(run, dtype, False)
    sos, eos, unk, pad = vocab["<sos>"], vocab["<eos>"], vocab["<unk>"], vocab["<blank>"]
    idx, _ = dh.make_batch_indices(data, 1, separate_caption=True)
    turns = _turns(cs)
    assert len(turns) == len(data["dialogs"])
    D._SESSIONS.clear()
    worst = 0.0
    for qa, turn in enumerate(turns):
        toks = [vocab[w] for w in turn["answer"].split()]
        n_logged = len(turn["contrastive"]["logp"])
        assert n_logged in (len(toks), len(toks) + 1) and (n_logged == len(toks) + 1 or len(toks) == MAXLEN - 1)
        chosen = toks + ([eos] if n_logged == len(toks) + 1 else [])
        sess = D.DecodeSession(model, dh.make_batch(corpus, idx[qa], vocab, separate_caption=True), MAXLEN, 1, pad=pad, use_graph=False)
        prefix = [sos]
        for l, y in enumerate(chosen):
            row = sess.step([prefix]).float().cpu().numpy()[0].astype(np.float64)
            row[[unk, pad, sos]] = -np.inf
            if l < 1:                                   # --min-length 1
                row[eos] = -np.inf
            gap = row.max() - row[y]
            worst = max(worst, gap)
            assert gap <= BAR[dtype] * max(1.0, abs(row.max())), (qa, l, y, gap)
            assert abs(turn["contrastive"]["logp"][l] - row[y]) <= BAR[dtype] * max(1.0, abs(row[y])), (qa, l)
            prefix = prefix + [y]
    print("alpha 0, %s: largest distance to the row maximum %.3g" % (dtype, worst))


@pytest.fixture(scope="module")
def searches(run):
    """Per dtype: the eager traced search and the captured search of one batch of three QAs, K = 5, alpha = 0.6."""
    from mtn_amd import decode as D
    out = {}
    for dtype in ("fp32", "bf16"):
        vocab, _, data, corpus, model, _ = _reference_side(run, dtype, False)
        sos, eos, unk, pad = vocab["<sos>"], vocab["<eos>"], vocab["<unk>"], vocab["<blank>"]
        kw = dict(k=K, alpha=ALPHA, banned=(unk, pad, sos), min_len=1, penalty=1.0)
        batch = _batch_of(data, corpus, vocab, [0, 3, 7])
        D._SESSIONS.clear()
        eager_tr, graph_tr = [], []
        eager = D.contrastive_decode_many(model, batch, MAXLEN, sos, eos, pad, use_graph=False, trace=eager_tr, **kw)
        graph = D.contrastive_decode_many(model, batch, MAXLEN, sos, eos, pad, use_graph=True, trace=graph_tr, **kw)
        out[dtype] = dict(eager=eager, graph=graph, eager_tr=eager_tr[0], graph_tr=graph_tr[0], vocab=vocab, kw=kw, model=model, data=data, corpus=corpus)
    D._SESSIONS.clear()
    return out


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_eager_search_follows_the_definition_step_by_step(searches, dtype):
    """Every step of the traced search against the float64 reference on the traced device inputs: the choice agrees wherever the reference's
    margin exceeds 4 bounds — at most one scored step in ten may fall under that and be left out — and every logged penalty is within the
    cosine bound of the reference's penalty of the chosen row."""
    s = searches[dtype]
    tok, lp, pen, rank, steps = s["eager_tr"]
    vocab, kw = s["vocab"], s["kw"]
    eos = vocab["<eos>"]
    assert len(steps) == MAXLEN
    D_, d = tok.shape[1], steps[0]["hidden"].shape[2]
    B = R.bound(float(np.float32(ALPHA)), d)
    scored = close = 0
    worst_pen, smallest = 0.0, np.inf
    for i, st_in in enumerate(steps):
        st = R.State(D_, K, MAXLEN)
        st.tokens, st.cand_logp, st.step, st.done = st_in["tokens"].copy(), st_in["cand_logp"].copy(), st_in["step"].copy(), st_in["done"].copy()
        assert (st.step == i).all()
        R.advance(st, st_in["hidden"], st_in["top"], alpha=ALPHA, eos=eos, min_len=kw["min_len"], banned=kw["banned"])
        for (l, dlg), margin in st.margins.items():
            assert l == i
            scored += 1
            p64 = R.penalties(st_in["hidden"][dlg * K:dlg * K + K], l)
            worst_pen = max(worst_pen, abs(float(pen[l, dlg]) - p64[rank[l, dlg]]))
            assert abs(float(pen[l, dlg]) - p64[rank[l, dlg]]) <= R.cos_bound(d), (l, dlg)
            assert lp[l, dlg] == st_in["cand_logp"][dlg * K + rank[l, dlg]] and tok[l, dlg] == st_in["tokens"][dlg * K + rank[l, dlg], l]
            if margin > 4 * B:
                smallest = min(smallest, margin)
                assert rank[l, dlg] == st.log_rank[l, dlg] and tok[l, dlg] == st.log_tok[l, dlg], (l, dlg, margin, B)
            else:
                close += 1
        if i + 1 < MAXLEN:                               # where the choice agreed, the next step's inputs are the reference's outputs
            nxt = steps[i + 1]
            agree = [dlg for dlg in range(D_) if (i, dlg) not in st.margins or rank[i, dlg] == st.log_rank[i, dlg]]
            for dlg in agree:
                rows = slice(dlg * K, dlg * K + K)
                assert (nxt["tokens"][rows] == st.tokens[rows]).all() and (nxt["done"][dlg] == st.done[dlg])
                assert (nxt["cand_logp"][rows].view(np.int32) == st.cand_logp[rows].view(np.int32)).all()
    print("%s: %d scored steps, %d under 4 B (B = %.3g), smallest other margin %.3g, largest penalty error %.3g (bound %.3g)"
          % (dtype, scored, close, B, smallest, worst_pen, R.cos_bound(d)))
    assert scored >= 10 and close * 10 <= scored, (scored, close)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_captured_search_gives_the_eager_logs_byte_for_byte(searches, dtype):
    s = searches[dtype]
    for a, b in zip(s["eager_tr"][:4], s["graph_tr"][:4]):
        assert a.dtype == b.dtype and a.shape == b.shape and (a.view(np.uint8) == b.view(np.uint8)).all()
    assert len(s["graph_tr"]) == 4                      # (the captured search has no per-step trace)
    assert s["eager"] == s["graph"]


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_result_structure(run, searches, dtype, caplog, monkeypatch):
    """Lengths, banned ids, --min-length and the scores recomputed from the log, on the CLI run and on the function's results."""
    cs, logged = _main(run, "contrastive", dtype, "cs_%s.json" % dtype, ["--min-length", "3", "--penalty", "1.0", "--evaluate"], caplog)
    vocab = searches[dtype]["vocab"]
    vl = sorted(vocab, key=vocab.get)
    banned_words = {vl[vocab[w]] for w in ("<unk>", "<blank>", "<sos>")}
    turns = _turns(cs)
    assert "eval" in cs and [t["answer"] for t in turns] == logged
    for t in turns:
        words, c = t["answer"].split(), t["contrastive"]
        n = len(words)
        assert 3 <= n <= MAXLEN - 1 and not banned_words & set(words) and "<eos>" not in words
        assert len(c["logp"]) == len(c["penalty"]) == len(c["rank"]) and len(c["logp"]) in (n, n + 1)
        assert len(c["logp"]) == n + 1 or n == MAXLEN - 1
        assert all(0 <= r < K for r in c["rank"]) and all(v <= 0 for v in c["logp"]) and all(-1.0 - 1e-4 <= p <= 1.0 + 1e-4 for p in c["penalty"])
        assert abs(c["score"] - (float(np.sum(np.asarray(c["logp"], dtype=np.float64))) + 1.0 * (n + 1))) <= 2e-6
    eos = vocab["<eos>"]
    tok, lp = searches[dtype]["eager_tr"][:2]
    for dlg, (toks, score, logp, pens, ranks) in enumerate(searches[dtype]["eager"]):
        want_toks, want_score, used = R.response(tok, lp, dlg, eos, penalty=1.0)
        assert toks == want_toks and abs(score - want_score) <= 2e-6 and len(logp) == len(pens) == len(ranks) == used
        assert not set(toks) & set(searches[dtype]["kw"]["banned"]) and 1 <= len(toks) <= MAXLEN - 1


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_a_reused_session_equals_a_fresh_one(searches, dtype):
    """Two batches of one padded shape: the second search of a session — after load, on the graph captured for the first — gives what a
    fresh session gives."""
    from mtn_amd import data_handler as dh
    from mtn_amd import decode as D
    s = searches[dtype]
    vocab, model, data, corpus = s["vocab"], s["model"], s["data"], s["corpus"]
    sos, eos, pad = vocab["<sos>"], vocab["<eos>"], vocab["<blank>"]
    idx, _ = dh.make_batch_indices(data, 1, separate_caption=True)
    ids_a, ids_b = [0, 3, 7], [11, 12, 1]
    lens = [idx[i] for i in ids_a + ids_b]
    dims = ([max(l[2][f] for l in lens) for f in range(len(lens[0][2]))], max(l[3] for l in lens), max(l[4] for l in lens),
            max(l[5] for l in lens), max(l[6] for l in lens))
    mk = lambda ids: dh.make_batch(corpus, ([data["dialogs"][i][0] for i in ids], list(ids)) + dims + (len(ids),), vocab, separate_caption=True)
    D._SESSIONS.clear()
    fresh = D.contrastive_decode_many(model, mk(ids_b), MAXLEN, sos, eos, pad, **s["kw"])
    D._SESSIONS.clear()
    first = D.contrastive_decode_many(model, mk(ids_a), MAXLEN, sos, eos, pad, **s["kw"])
    n_sessions = len(D._SESSIONS)
    again = D.contrastive_decode_many(model, mk(ids_b), MAXLEN, sos, eos, pad, **s["kw"])
    assert len(D._SESSIONS) == n_sessions == 1 and again == fresh and first != fresh
    D._SESSIONS.clear()
