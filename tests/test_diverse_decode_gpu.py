"""Diverse beam search (beam_groups, diversity_penalty) through decode.py on the GPU: the model and batch of
tests/test_constrain_decode_gpu.py — d_model 128, one block, V 300, two dominant tokens, so the plain n-best lists are near-copies of one
sentence — for D = 2 dialogues, beam 4, max_len 16, in bf16 (persistent step: the search is ONE captured graph with csrc/diverse.hip in
mtn_beam_advance's place) and fp32 (launch-per-sublayer pass: groups of decode._Beam on the host).

Bars, the project's own for the same pairs of paths: the captured search against the same session stepped from the host — equal; against
use_graph=False — identical tokens, scores within 1e-3; fp32 with the prefix K/V cache — identical tokens; the bf16 persistent step against
the bf16 launch path — best score within 1e-2 (relative, floor 1).  The fp32 host-stepped search is held to tests/diverse_refs.py's whole
search on the session's own rows."""
import collections
import math
import os

import numpy as np
import pytest
import torch

from tests import diverse_refs as R
from tests.constrain_refs import has_repeated_ngram

pytestmark = pytest.mark.gpu
V, SOS, UNK, EOS, PAD = 300, 2, 0, 3, 1
D_, BEAM, MAXLEN, MINLEN = 2, 4, 16, 8
DOMINANT, SHIFT = (11, 29), 14.0
SETTINGS = [(2, 0.5), (4, 0.5), (4, 64.0)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


def _model(dev, dtype, seed=4):
    from mtn_amd import make_model
    torch.manual_seed(seed)
    m = make_model(V, V, N=1, d_model=128, d_ff=256, h=4, dropout=0.1, ft_sizes=[64, 32], diff_encoder=True, auto_encoder_ft="query",
                   compute_dtype=dtype)
    with torch.no_grad():
        m.generator.proj.bias[list(DOMINANT)] += SHIFT        # two tokens hold almost all the mass at every step
    return m.to(dev).eval()


def _batch(dev, seed=50):
    from mtn_amd.synthetic import synthetic_batch
    return synthetic_batch(V, D_, 9, 30, 14, 8, [11, 7], [64, 32], device=dev, seed=seed, ragged=True)


def _beam(model, b, **kw):
    from mtn_amd import decode as D
    return D.beam_search_decode_many(model, b, MAXLEN, SOS, UNK, EOS, PAD, beam=BEAM, penalty=1.0, nbest=4, min_len=MINLEN, **kw)


def _mega_sessions():
    from mtn_amd import decode as D
    return [s[0] for s in D._SESSIONS.values() if isinstance(s[0], D.MegaDecodeSession) and s[0].width == BEAM]


@pytest.fixture(scope="module", params=[torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def setup(request, dev):
    from mtn_amd import decode as D
    D._SESSIONS.clear()
    model, b = _model(dev, request.param), _batch(dev)
    plain = _beam(model, b)
    # non-vacuity — a condition of every test below: the plain n-best of EVERY dialogue is near-copies of one sentence
    for nbest, _ in plain:
        assert len(nbest) == 4
        first = collections.Counter(t[0] for t, _ in nbest)
        assert first.most_common(1)[0][1] >= 3, nbest
    yield model, b, request.param, plain
    D._SESSIONS.clear()


class _Spy:
    """decode._diverse_advance with its inputs and outcome recorded: per step the heads' values and, per dialogue and group, the newest
    tokens of the new beam."""

    def __init__(self, D):
        self.real, self.heads, self.trace = D._diverse_advance, [], []

    def __call__(self, beams, G, l, lam, vals, idx, eos, k, rows, tie):
        self.heads.append(np.array(vals))
        self.real(beams, G, l, lam, vals, idx, eos, k, rows, tie)
        self.trace += [(l, j // G, j % G, [h[2][-1] for h in bm.hyps]) for j, bm in enumerate(beams)]


@pytest.mark.parametrize("G,lam", SETTINGS)
def test_paths_agree(setup, G, lam, monkeypatch):
    from mtn_amd import decode as D
    model, b, dtype, plain = setup
    kw = dict(beam_groups=G, diversity_penalty=lam)
    captured = []
    real_search = D.MegaDecodeSession.search

    def search(self, *a, **k):
        r = real_search(self, *a, **k)
        captured.append(r is not None)
        return r

    with monkeypatch.context() as mp:
        mp.setattr(D.MegaDecodeSession, "search", search)
        res = _beam(model, b, **kw)
    if dtype == torch.bfloat16:
        mega = _mega_sessions()
        assert mega and captured == [True], "the diverse search did not run as the captured graph"
        assert mega[0]._search_key[-2:] == (G, float(lam)) and len(mega[0]._search_key) == 11
        assert not mega[0].timed_out()
    else:
        assert captured == []
    assert len(res) == D_
    for (nbest, best), (pn, _) in zip(res, plain):
        assert len(nbest) == 4 and best == nbest[0][1] and [s for _, s in nbest] == sorted((s for _, s in nbest), reverse=True)
        assert len({tuple(t) for t, _ in nbest}) == 4                          # no duplicate token lists
        for toks, score in nbest:
            assert len(toks) >= MINLEN - 1 and UNK not in toks and EOS not in toks and math.isfinite(score)
        assert [t for t, _ in nbest] != [t for t, _ in pn]                    # the groups did change the search
    # the same session stepped from the host: the per-step kernels are the same and the bookkeeping is defined bit for bit — EQUAL
    if dtype == torch.bfloat16:
        with monkeypatch.context() as mp:
            mp.setattr(D.MegaDecodeSession, "search", lambda self, *a, **k: None)
            assert _beam(model, b, **kw) == res
    eager = _beam(model, b, use_graph=False, **kw)
    for (n1, b1), (n0, b0) in zip(res, eager):
        assert [t for t, _ in n1] == [t for t, _ in n0]
        assert max(abs(x[1] - y[1]) for x, y in zip(n1, n0)) < 1e-3 and abs(b1 - b0) < 1e-3
    if dtype == torch.float32:
        cached = _beam(model, b, kv_cache=True, **kw)
        for (n1, _), (n0, _) in zip(res, cached):
            assert [t for t, _ in n1] == [t for t, _ in n0]


@pytest.mark.parametrize("G,lam", SETTINGS)
def test_bf16_persistent_step_and_launch_path_agree(dev, G, lam):
    from mtn_amd import decode as D
    D._SESSIONS.clear()
    model, b = _model(dev, torch.bfloat16), _batch(dev)
    kw = dict(beam_groups=G, diversity_penalty=lam)
    res = _beam(model, b, **kw)
    assert any(isinstance(s[0], D.MegaDecodeSession) for s in D._SESSIONS.values()), "the persistent step was not taken"
    os.environ["MTN_DECODE_MEGA"] = "0"
    try:
        D._SESSIONS.clear()
        launch = _beam(model, b, **kw)
        assert not any(isinstance(s[0], D.MegaDecodeSession) for s in D._SESSIONS.values())
    finally:
        del os.environ["MTN_DECODE_MEGA"]
        D._SESSIONS.clear()
    for (n1, b1), (n0, b0) in zip(res, launch):
        assert len(n1) == len(n0)
        assert abs(b1 - b0) < 1e-2 * max(1.0, abs(b0))


@pytest.mark.parametrize("G,lam", SETTINGS)
def test_fp32_host_search_equals_the_definition(dev, G, lam, monkeypatch):
    """The stepped search of decode.py against diverse_refs.search driven by the very session's rows: n-best tokens, and the tokens every
    group places at every step, in group order."""
    from mtn_amd import decode as D
    D._SESSIONS.clear()
    model, b = _model(dev, torch.float32), _batch(dev)
    spy = _Spy(D)
    monkeypatch.setattr(D, "_diverse_advance", spy)
    res = _beam(model, b, beam_groups=G, diversity_penalty=lam)
    (sess, _), = D._SESSIONS.values()
    trace = []
    ref = R.search(lambda pl: [t.cpu().numpy() for t in sess.step_many(pl)], D_, BEAM, G, lam, MAXLEN, SOS, UNK, EOS, 1.0, MINLEN, 4, trace=trace)
    assert spy.trace == trace
    for (n1, b1), (n0, b0) in zip(res, ref):
        assert [t for t, _ in n1] == [t for t, _ in n0]
    D._SESSIONS.clear()


def test_a_large_penalty_keeps_the_groups_apart(setup, monkeypatch):
    """(4, 64): one hypothesis per group, and 64 exceeds the spread of every row's head — so a token an earlier group took falls below every
    free entry of the head, and the four groups of a dialogue place four different tokens at every step."""
    from mtn_amd import decode as D
    model, b, dtype, _ = setup
    kw = dict(beam_groups=4, diversity_penalty=64.0)
    spy = _Spy(D)
    with monkeypatch.context() as mp:
        mp.setattr(D, "_diverse_advance", spy)
        mp.setattr(D.MegaDecodeSession, "search", lambda self, *a, **k: None)
        stepped = _beam(model, b, **kw)
    assert len(spy.heads) == MAXLEN
    for vals in spy.heads:
        assert np.isfinite(vals).all() and float((vals[:, 0] - vals[:, -1]).max()) < 64.0
    placed = collections.defaultdict(list)
    if dtype == torch.bfloat16:
        assert _beam(model, b, **kw) == stepped
        sess = _mega_sessions()[0]
        tok, n_new = sess._log_views[1], sess._log_views[3]                   # the captured search's step log: (L, W) tokens, (L, D x G) live counts
        assert n_new.shape == (MAXLEN, D_ * 4) and (n_new == 1).all()
        for l in range(MAXLEN):
            for p in range(D_ * 4):
                placed[(l, p // 4)].append(int(tok[l, p]))                    # (beam / groups = 1: pseudo-dialogue p owns row p)
    else:
        for l, d, g, toks in spy.trace:
            placed[(l, d)] += toks
    assert len(placed) == MAXLEN * D_
    for key, toks in placed.items():
        assert len(toks) == 4 and len(set(toks)) == 4, (key, toks)
    for nbest, _ in stepped:
        assert len({tuple(t) for t, _ in nbest}) == len(nbest) == 4


class _CountingLib:
    """The loaded HIP library with every call of an `mtn_*` entry counted by name."""

    def __init__(self, real, counts):
        self._real, self._counts = real, counts

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not name.startswith("mtn_"):
            return fn

        def counted(*a):
            self._counts[name] += 1
            return fn(*a)
        return counted


def test_one_group_is_the_plain_search(setup, monkeypatch):
    from mtn_amd import decode as D
    from mtn_amd import lib
    model, b, dtype, plain = setup
    counts = collections.Counter()
    counting = _CountingLib(lib.load(), counts)
    monkeypatch.setattr(lib, "load", lambda: counting)
    D._SESSIONS.clear()
    base = _beam(model, b)
    assert base == plain
    assert _beam(model, b, beam_groups=1, diversity_penalty=0.0) == base
    assert counts["mtn_diverse_advance"] == 0 and counts["mtn_topk_rows"] > 0
    if dtype == torch.bfloat16:
        sess = _mega_sessions()[0]
        assert len(sess._search_key) == 9 and sess._search_key[-2:] == (0, 1.0)      # the plain key: no (G, lambda)
        assert counts["mtn_beam_advance"] == 2 * MAXLEN                               # warm-up + capture, once: the second call only replayed
        _beam(model, b, beam_groups=2, diversity_penalty=0.5)
        assert counts["mtn_diverse_advance"] == 2 * MAXLEN and counts["mtn_beam_advance"] == 2 * MAXLEN
    for bad in (dict(beam_groups=3), dict(beam_groups=0), dict(beam_groups=2, diversity_penalty=-0.5), dict(diversity_penalty=0.5),
                dict(beam_groups=2, diversity_penalty=float("nan")), dict(beam_groups=2, diversity_penalty=float("inf"))):
        before = sum(counts.values())
        with pytest.raises(ValueError):
            _beam(model, b, **bad)
        assert sum(counts.values()) == before, "the keywords are checked before anything runs"
    D._SESSIONS.clear()


def test_with_ngram_blocking(dev, monkeypatch):
    from mtn_amd import decode as D
    D._SESSIONS.clear()
    model, b = _model(dev, torch.bfloat16), _batch(dev)
    kw = dict(beam_groups=2, diversity_penalty=0.5, no_repeat_ngram=2)
    res = _beam(model, b, **kw)
    sess = _mega_sessions()[0]
    assert sess._search_key[-4:] == (2, 1.0, 2, 0.5) and sess._log_views[6][0] == 0, "not the captured graph"
    for nbest, _ in res:
        assert len(nbest) == 4 and not any(has_repeated_ngram(t, 2) for t, _ in nbest)
    with monkeypatch.context() as mp:
        mp.setattr(D.MegaDecodeSession, "search", lambda self, *a, **k: None)
        assert _beam(model, b, **kw) == res
    D._SESSIONS.clear()


def test_with_an_ensemble(dev, monkeypatch):
    from mtn_amd import decode as D
    D._SESSIONS.clear()
    ens, b = D.Ensemble([_model(dev, torch.bfloat16, 4), _model(dev, torch.bfloat16, 5)]), _batch(dev)
    kw = dict(beam_groups=2, diversity_penalty=0.5)
    res = _beam(ens, b, **kw)
    sess = [s[0] for s in D._SESSIONS.values() if isinstance(s[0], D.EnsembleMegaSession)]
    assert sess and sess[0]._search_key[-2:] == (2, 0.5) and sess[0]._log_views[6][0] == 0, "not the captured graph"
    assert all(len(nbest) == 4 and len({tuple(t) for t, _ in nbest}) == 4 for nbest, _ in res)
    with monkeypatch.context() as mp:
        mp.setattr(D.MegaDecodeSession, "search", lambda self, *a, **k: None)
        assert _beam(ens, b, **kw) == res
    D._SESSIONS.clear()
