"""--mbr / --mbr-weights / --mbr-temperature of mtn_amd.generate without a GPU: parser defaults and refusals, the way the values travel
through generate_response and decode_searches into decode.sample_decode_many / decode.mbr_rerank, and the form of the log and the JSON."""
import logging
import re
import types

import pytest

from mtn_amd import generate as G

VOCAB = {"<unk>": 0, "<blank>": 1, "<sos>": 2, "<eos>": 3, "a": 4, "man": 5, "walks": 6}
SAMPLE = ["--decode-style", "sample", "--samples", "4"]
BEAM = ["--decode-style", "beam_search", "--beam", "5"]


def test_parser_defaults_are_off():
    a = G.parse([])
    assert (a.mbr, a.mbr_weights, a.mbr_temperature) == (0, "uniform", 1.0)
    a = G.parse(SAMPLE + ["--mbr", "2"])
    assert (a.mbr, a.mbr_weights, a.mbr_temperature) == (2, "uniform", 1.0)
    a = G.parse(BEAM + ["--mbr", "4", "--mbr-weights", "score", "--mbr-temperature", "0.5", "--nbest", "16"])
    assert (a.mbr, a.mbr_weights, a.mbr_temperature, a.nbest) == (4, "score", 0.5, 16)
    for style in ("greedy", "sample", "score", "beam_search"):                       # --mbr 0 spelled out goes with every style
        assert G.parse(["--decode-style", style, "--mbr", "0"]).mbr == 0
    assert G.parse(BEAM + ["--nbest", "20"]).nbest == 20                             # a long n-best list is fine without --mbr


@pytest.mark.parametrize("argv,flag", [
    (SAMPLE + ["--mbr", "5"], "--mbr"),
    (SAMPLE + ["--mbr", "-1"], "--mbr"),
    (["--decode-style", "greedy", "--mbr", "2"], "--mbr"),
    (["--decode-style", "score", "--mbr", "2"], "--mbr"),
    (["--mbr", "2"], "--mbr"),                                                       # (greedy is the default style)
    (BEAM + ["--mbr", "2", "--nbest", "17"], "--nbest"),
    (SAMPLE + ["--mbr", "2", "--mbr-temperature", "0"], "--mbr-temperature"),
    (SAMPLE + ["--mbr", "2", "--mbr-temperature", "-1.5"], "--mbr-temperature"),
    (SAMPLE + ["--mbr", "2", "--mbr-temperature", "nan"], "--mbr-temperature"),
    (SAMPLE + ["--mbr-weights", "score"], "--mbr-weights"),                          # given with --mbr 0
    (SAMPLE + ["--mbr-weights", "uniform"], "--mbr-weights"),
    (SAMPLE + ["--mbr", "0", "--mbr-temperature", "2"], "--mbr-temperature"),
    (BEAM + ["--mbr-temperature", "1"], "--mbr-temperature"),
    (SAMPLE + ["--mbr", "2", "--mbr-weights", "rank"], "--mbr-weights"),
])
def test_parser_refuses(argv, flag, capsys):
    with pytest.raises(SystemExit) as e:
        G.parse(argv)
    assert e.value.code == 2
    assert flag in capsys.readouterr().err


def _data(n=5):
    """The fields of data_handler.load's result that generate_response reads, for n single-turn dialogues without features."""
    dialogs = [("v%d" % i, i, [1], [4, 5, 6][:1 + i % 3], [4, 5], None, [4, 5, 6]) for i in range(n)]
    original = {"dialogs": [{"image_id": "v%d" % i, "dialog": [{"question": "a man", "answer": "walks"}]} for i in range(n)]}
    return dict(dialogs=dialogs, features=None, original=original)


TRIPLES = [([4, 5], -2.0, 0.625), ([6], -1.0, 0.1 + 0.2), ([4, 5, 6], -3.0, 0.0)]


def test_values_reach_decode_searches_and_shape_the_output(monkeypatch, caplog):
    seen = {}

    def fake(model, corpus, searches, vids, vocab, decode_style, maxlen, beam, penalty, nbest, **kw):
        seen.clear()
        seen.update(kw, decode_style=decode_style)
        mbr = kw.get("mbr", 0)
        hyps = TRIPLES if mbr else [h[:2] for h in TRIPLES]
        one = {"beam_search": (hyps, -1.0), "sample": hyps}[decode_style]
        return {i: one for ids, n, _ in searches for i in ids[:n]}

    monkeypatch.setattr(G, "decode_searches", fake)
    corpus = types.SimpleNamespace(device="cpu")
    caplog.set_level(logging.INFO)
    for style in ("sample", "beam_search"):
        caplog.clear()
        res = G.generate_response(None, _data(), corpus, VOCAB, decode_style=style, beam=5, dialogues_per_search=2, sampling=dict(samples=3),
                                  mbr=3, mbr_weights="score", mbr_temperature=0.5)
        assert (seen["mbr"], seen["mbr_weights"], seen["mbr_temperature"]) == (3, "score", 0.5)
        msgs = [r.getMessage() for r in caplog.records]
        per_qa = [i for i, m in enumerate(msgs) if m.startswith("HYP[1]: ")]
        assert len(per_qa) == 5
        for i in per_qa:
            assert msgs[i:i + 4] == ["HYP[1]: a man  ( -2.000000 )", "HYP[2]: walks  ( -1.000000 )", "HYP[3]: a man walks  ( -3.000000 )",
                                     "MBR: 0.625 0.30000000000000004 0.0"]
        assert all(re.fullmatch(r"HYP\[\d+\]: .*  \( \S+ \)", m) for m in msgs if m.startswith("HYP"))
        for d in res["dialogs"]:
            turn = d["dialog"][0]
            assert turn["answer"] == "a man"
            assert turn["mbr"] == [dict(hypothesis="a man", score=-2.0, expected=0.625), dict(hypothesis="walks", score=-1.0, expected=0.1 + 0.2),
                                   dict(hypothesis="a man walks", score=-3.0, expected=0.0)]
        # off: nothing about it reaches decode_searches, the log or the JSON
        caplog.clear()
        res = G.generate_response(None, _data(), corpus, VOCAB, decode_style=style, beam=5, dialogues_per_search=2, sampling=dict(samples=3))
        assert not any(k.startswith("mbr") for k in seen)
        assert not any(r.getMessage().startswith("MBR") for r in caplog.records)
        assert all("mbr" not in d["dialog"][0] for d in res["dialogs"])
    for kw in (dict(decode_style="greedy", mbr=2), dict(decode_style="score", mbr=2), dict(decode_style="sample", mbr=5),
               dict(decode_style="sample", mbr=2, mbr_temperature=0.0), dict(decode_style="sample", mbr=2, mbr_weights="rank"),
               dict(decode_style="beam_search", mbr=2, nbest=17), dict(decode_style="sample", mbr=2, maxlen=129)):
        with pytest.raises(ValueError, match="mbr"):
            G.generate_response(None, _data(), corpus, VOCAB, dialogues_per_search=2, **kw)


def test_values_reach_the_decode_functions(monkeypatch):
    from mtn_amd import data_handler as dh
    from mtn_amd import decode as D
    calls = []
    monkeypatch.setattr(dh, "make_batch", lambda corpus, index, pad, **kw: types.SimpleNamespace(n=index[-1]))
    pairs = [h[:2] for h in TRIPLES]

    def sample(model, batch, *a, **kw):
        calls.append(("sample", kw.get("mbr", 0)))
        return [list(TRIPLES) if kw.get("mbr") else list(pairs)] * batch.n

    def beam(model, batch, *a, **kw):
        calls.append(("beam", kw.get("nbest")))
        return [(list(pairs), -1.0)] * batch.n

    def rerank(lists, ngram, weights="uniform", temperature=1.0, device=None):
        calls.append(("rerank", ngram, weights, temperature, [len(l) for l in lists]))
        return [[h + (0.5,) for h in reversed(l)] for l in lists]

    monkeypatch.setattr(D, "sample_decode_many", sample)
    monkeypatch.setattr(D, "beam_search_decode_many", beam)
    monkeypatch.setattr(D, "mbr_rerank", rerank)
    searches = G.plan_searches(G.qa_lengths(_data()), 2)
    vids = {i: "v%d" % i for i in range(5)}
    smp = dict(samples=3, temperature=1.0, top_k=0, top_p=1.0, seed=1)
    run = lambda style, nbest=5, **kw: G.decode_searches(None, None, searches, vids, VOCAB, style, 30, 5, 1.0, nbest, sampling=smp, **kw)
    # sample, uniform: inside the search, no second launch
    res = run("sample", mbr=2)
    assert set(calls) == {("sample", 2)} and res[0] == TRIPLES
    calls.clear()
    # sample, score weights: the plain search, then mbr_rerank
    res = run("sample", mbr=2, mbr_weights="score", mbr_temperature=0.5)
    assert {c[0] for c in calls} == {"sample", "rerank"} and ("sample", 0) in calls and ("rerank", 2, "score", 0.5, [3, 3]) in calls
    assert res[0] == [h + (0.5,) for h in reversed(pairs)]
    calls.clear()
    # beam search: the n-best list is cut to --nbest before the selection, and the best score rides along
    res = run("beam_search", nbest=2, mbr=4)
    assert ("rerank", 4, "uniform", 1.0, [2, 2]) in calls and ("beam", 2) in calls
    assert res[0] == ([h + (0.5,) for h in reversed(pairs[:2])], -1.0)
    calls.clear()
    # off: today's calls
    assert run("sample")[0] == pairs and run("beam_search")[0] == (pairs, -1.0)
    assert not any(c[0] == "rerank" for c in calls) and ("sample", 0) in calls


def test_decode_keywords_are_checked_before_anything_runs():
    from mtn_amd import decode as D
    long = ([4] * 129, -1.0)
    with pytest.raises(ValueError):
        D.mbr_rerank([[long]], 2)
    with pytest.raises(ValueError):
        D.mbr_rerank([[([4], -1.0)] * 17], 2)
    for kw in (dict(temperature=0.0), dict(temperature=-1.0), dict(weights="rank")):
        with pytest.raises(ValueError):
            D.mbr_rerank([[([4], -1.0)]], 2, **kw)
    for n in (0, 5):
        with pytest.raises(ValueError):
            D.mbr_rerank([[([4], -1.0)]], n)
    assert D.mbr_rerank([], 2) == []
    batch = types.SimpleNamespace(query=types.SimpleNamespace(size=lambda i: 1))
    for kw in (dict(mbr=5), dict(mbr=-1), dict(mbr=2, samples=17)):
        with pytest.raises(ValueError, match="mbr"):
            D.sample_decode_many(None, batch, 16, 2, 3, 1, **kw)
    with pytest.raises(ValueError, match="mbr"):
        D.sample_decode_many(None, batch, 129, 2, 3, 1, mbr=2)
