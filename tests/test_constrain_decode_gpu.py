"""Constrained decoding (no_repeat_ngram, repetition_penalty) through decode.py on the GPU: a small model (d_model 128, one block) whose
generator bias is shifted so that two tokens dominate — unconstrained, every search loops over them — decoded for D = 2 dialogues with
beam 4, max_len 16, min_len 8, in bf16 (persistent step: the search is ONE captured graph with csrc/constrain.hip inside) and fp32
(launch-per-sublayer pass: the kernel runs step by step on explicit histories).

Bars, as tests/test_decode_gpu.py holds the same pairs of paths to: the captured search against the same session stepped from the host —
equal; against use_graph=False — identical n-best tokens, scores within 1e-3; the bf16 persistent step against the bf16 launch path — best
score within 1e-2 (relative, floor 1)."""
import os

import pytest
import torch

from tests.constrain_refs import has_repeated_ngram

pytestmark = pytest.mark.gpu
V, SOS, UNK, EOS, PAD = 300, 2, 0, 3, 1
D_, BEAM, MAXLEN, MINLEN = 2, 4, 16, 8
DOMINANT, SHIFT = (11, 29), 14.0
SETTINGS = [(2, 1.0), (3, 1.0), (2, 1.2), (3, 1.2)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


def _model(dev, dtype):
    from mtn_amd import make_model
    torch.manual_seed(4)
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


@pytest.fixture(scope="module", params=[torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def setup(request, dev):
    from mtn_amd import decode as D
    D._SESSIONS.clear()
    model, b = _model(dev, request.param), _batch(dev)
    plain = _beam(model, b)
    # non-vacuity — a condition of every test below: left alone, the search of EVERY dialogue repeats bigrams and trigrams
    for nbest, _ in plain:
        assert len(nbest[0][0]) >= MINLEN - 1
        assert has_repeated_ngram(nbest[0][0], 2) and has_repeated_ngram(nbest[0][0], 3), nbest[0][0]
    yield model, b, request.param, plain
    D._SESSIONS.clear()


@pytest.mark.parametrize("N,theta", SETTINGS)
def test_paths_agree_and_no_hypothesis_repeats_an_ngram(setup, N, theta, monkeypatch):
    from mtn_amd import decode as D
    model, b, dtype, plain = setup
    kw = dict(no_repeat_ngram=N, repetition_penalty=theta)
    res = _beam(model, b, **kw)
    if dtype == torch.bfloat16:
        mega = [s[0] for s in D._SESSIONS.values() if isinstance(s[0], D.MegaDecodeSession) and s[0].width == BEAM]
        assert mega and mega[0]._search_key[-2:] == (N, float(theta)), "the constrained search did not run as the captured graph"
        assert not mega[0].timed_out()
    assert len(res) == D_
    for (nbest, best), (pn, _) in zip(res, plain):
        assert len(nbest) == 4 and best == nbest[0][1]
        for toks, score in nbest:
            assert len(toks) >= MINLEN - 1 and not has_repeated_ngram(toks, N), (N, toks)
            assert UNK not in toks and EOS not in toks and score == score and score > -1e30
        assert [t for t, _ in nbest] != [t for t, _ in pn]              # the constraint did change the search
    # the same session stepped from the host (explicit histories): the per-step kernels are the same, so everything is EQUAL
    if dtype == torch.bfloat16:
        with monkeypatch.context() as mp:
            mp.setattr(D.MegaDecodeSession, "search", lambda self, *a, **k: None)
            assert _beam(model, b, **kw) == res
    # eager launches instead of graphs
    eager = _beam(model, b, use_graph=False, **kw)
    for (n1, b1), (n0, b0) in zip(res, eager):
        assert [t for t, _ in n1] == [t for t, _ in n0]
        assert max(abs(x[1] - y[1]) for x, y in zip(n1, n0)) < 1e-3 and abs(b1 - b0) < 1e-3
    # the prefix K/V cache pass (what searches longer than KV_CACHE_FROM take where the persistent step does not apply)
    if dtype == torch.float32:
        cached = _beam(model, b, kv_cache=True, **kw)
        for (n1, b1), (n0, b0) in zip(res, cached):
            assert [t for t, _ in n1] == [t for t, _ in n0] and abs(b1 - b0) < 1e-3


@pytest.mark.parametrize("N,theta", SETTINGS)
def test_bf16_persistent_step_and_launch_path_agree(dev, N, theta):
    from mtn_amd import decode as D
    D._SESSIONS.clear()
    model, b = _model(dev, torch.bfloat16), _batch(dev)
    kw = dict(no_repeat_ngram=N, repetition_penalty=theta)
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
        assert not any(has_repeated_ngram(t, N) for t, _ in n0)


@pytest.mark.parametrize("N,theta", SETTINGS)
def test_greedy_and_samples_repeat_no_ngram(setup, N, theta, monkeypatch):
    from mtn_amd import decode as D
    model, b, dtype, _ = setup
    kw = dict(no_repeat_ngram=N, repetition_penalty=theta)
    free = D.greedy_decode_many(model, b, MAXLEN, SOS, PAD).tolist()
    assert all(has_repeated_ngram(y[1:], N) for y in free)                # non-vacuity
    many = D.greedy_decode_many(model, b, MAXLEN, SOS, PAD, **kw)
    assert many.shape == (D_, MAXLEN)
    for y in many.tolist():
        assert y[0] == SOS and not has_repeated_ngram(y[1:], N), y
    if dtype == torch.bfloat16:
        # one graph replay against the same session stepped from the host
        with monkeypatch.context() as mp:
            mp.setattr(D.MegaDecodeSession, "greedy", lambda self, *a, **k: None)
            assert D.greedy_decode_many(model, b, MAXLEN, SOS, PAD, **kw).tolist() == many.tolist()
    else:
        assert D.greedy_decode_many(model, b, MAXLEN, SOS, PAD, use_graph=False, **kw).tolist() == many.tolist()
    # samples: S = 4 per dialogue, each checked up to its <eos>
    skw = dict(samples=4, temperature=1.0, top_k=0, top_p=1.0, seed=3, banned=(UNK, PAD, SOS), min_len=MINLEN)
    loose = D.sample_decode_many(model, b, MAXLEN, SOS, EOS, PAD, **skw)
    assert all(has_repeated_ngram(t, N) for hyps in loose for t, _ in hyps)   # non-vacuity
    drawn = D.sample_decode_many(model, b, MAXLEN, SOS, EOS, PAD, **skw, **kw)
    assert len(drawn) == D_ and all(len(h) == 4 for h in drawn)
    for hyps in drawn:
        for toks, score in hyps:
            assert EOS not in toks and len(toks) >= MINLEN - 1 and not has_repeated_ngram(toks, N), (N, toks)
    assert D.sample_decode_many(model, b, MAXLEN, SOS, EOS, PAD, **skw, **kw) == drawn            # repeatable under one seed
    if dtype == torch.bfloat16:
        # the launch-per-sublayer pass runs the same constraint off its own token log
        os.environ["MTN_DECODE_MEGA"] = "0"
        try:
            launch = D.sample_decode_many(model, b, MAXLEN, SOS, EOS, PAD, **skw, **kw)
        finally:
            del os.environ["MTN_DECODE_MEGA"]
        assert not any(has_repeated_ngram(t, N) for hyps in launch for t, _ in hyps)


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


def test_off_means_unchanged(setup, monkeypatch):
    """N = 0 and theta = 1: the results of a call without the keywords, bit for bit; the constraint kernel is never launched; the captured
    search is the very graph of the unconstrained call (one search key, no new capture, the same log bytes).  The body of the captured
    search is counted launch by launch at the library's entries (every kernel of the body is launched through one: persistent step,
    generator, row heads, beam bookkeeping) while it is warmed up and captured: a constraint adds exactly one launch per token to it and
    changes no other count."""
    import collections
    from mtn_amd import decode as D
    from mtn_amd import lib
    model, b, dtype, plain = setup
    counts = collections.Counter()
    counting = _CountingLib(lib.load(), counts)
    monkeypatch.setattr(lib, "load", lambda: counting)
    searches = []                    # per MegaDecodeSession._search_log call: (constraint values, entries called inside it, tie / not applicable?)
    real_log = D.MegaDecodeSession._search_log

    def spy(self, *a, **k):
        before = collections.Counter(counts)
        r = real_log(self, *a, **k)
        searches.append((getattr(self, "_search_key", (None, None))[-2:], collections.Counter(counts) - before, r is None))
        return r

    monkeypatch.setattr(D.MegaDecodeSession, "_search_log", spy)
    D._SESSIONS.clear()
    base = _beam(model, b)
    assert base == plain
    sess = [s[0] for s in D._SESSIONS.values()]
    graph = getattr(sess[0], "_search_graph", None)
    log_bytes = bytes(sess[0]._log_host.numpy()) if graph is not None else None
    off = _beam(model, b, no_repeat_ngram=0, repetition_penalty=1.0)
    assert off == base and counts["mtn_constrain_rows"] == 0
    g_base = D.greedy_decode_many(model, b, MAXLEN, SOS, PAD)
    assert torch.equal(D.greedy_decode_many(model, b, MAXLEN, SOS, PAD, no_repeat_ngram=0, repetition_penalty=1.0), g_base)
    skw = dict(samples=4, seed=3, banned=(UNK, PAD, SOS), min_len=MINLEN)
    assert (D.sample_decode_many(model, b, MAXLEN, SOS, EOS, PAD, no_repeat_ngram=0, repetition_penalty=1.0, **skw)
            == D.sample_decode_many(model, b, MAXLEN, SOS, EOS, PAD, **skw))
    assert counts["mtn_constrain_rows"] == 0
    if dtype == torch.bfloat16:
        assert graph is not None and sess[0]._search_graph is graph, "the off call captured a graph of its own"
        assert bytes(sess[0]._log_host.numpy()) == log_bytes
        (k_plain, body_plain, tie_plain), (k_off, body_off, tie_off) = searches[0], searches[1]
        assert not tie_plain and not tie_off and k_plain == k_off == (0, 1.0)      # (a tie would have sent the search down the step-by-step path)
        # warm-up + capture of the plain body: max_len x [persistent step, generator, row heads, bookkeeping]; the off call only replays
        # (the generator is two entries: its GEMM and the row log-softmax)
        for entry in ("mtn_decode_step", "mtn_log_softmax_rows", "mtn_topk_rows", "mtn_beam_advance"):
            assert body_plain[entry] == 2 * MAXLEN, (entry, body_plain)
        assert set(body_plain.values()) == {2 * MAXLEN}, body_plain                  # nothing in the body runs off the per-token beat
        assert not body_off, body_off
        n = len(searches)
        _beam(model, b, no_repeat_ngram=2)
        assert len(searches) == n + 1
        k_con, body_con, tie_con = searches[n]
        assert not tie_con and k_con == (2, 1.0)
        assert body_con - body_plain == collections.Counter(mtn_constrain_rows=2 * MAXLEN) and not body_plain - body_con, (body_con, body_plain)
    with pytest.raises(ValueError):
        _beam(model, b, no_repeat_ngram=9)
    with pytest.raises(ValueError):
        _beam(model, b, repetition_penalty=0.5)
