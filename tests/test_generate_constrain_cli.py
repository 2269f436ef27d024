"""--no-repeat-ngram / --repetition-penalty / --min-length of mtn_amd.generate without a GPU: parser defaults and refusals, and the way
the values travel through generate_response and decode_searches into the decode calls."""
import types

import pytest

from mtn_amd import generate as G

VOCAB = {"<unk>": 0, "<blank>": 1, "<sos>": 2, "<eos>": 3, "a": 4, "man": 5, "walks": 6}


def test_parser_defaults_are_off():
    a = G.parse([])
    assert (a.no_repeat_ngram, a.repetition_penalty, a.min_length) == (0, 1.0, 1)
    a = G.parse(["--decode-style", "beam_search", "--no-repeat-ngram", "3", "--repetition-penalty", "1.2", "--min-length", "6"])
    assert (a.no_repeat_ngram, a.repetition_penalty, a.min_length) == (3, 1.2, 6)
    for style in ("greedy", "sample"):
        a = G.parse(["--decode-style", style, "--no-repeat-ngram", "8", "--repetition-penalty", "1"])
        assert (a.no_repeat_ngram, a.repetition_penalty) == (8, 1.0)
    # a scoring run with the defaults spelled out is no constrained run
    assert G.parse(["--decode-style", "score", "--no-repeat-ngram", "0", "--repetition-penalty", "1.0"]).decode_style == "score"


@pytest.mark.parametrize("argv", [["--no-repeat-ngram", "9"], ["--no-repeat-ngram", "-1"], ["--repetition-penalty", "0.99"],
                                  ["--repetition-penalty", "nan"], ["--decode-style", "score", "--no-repeat-ngram", "2"],
                                  ["--decode-style", "score", "--repetition-penalty", "1.5"], ["--min-length", "-1"]])
def test_parser_refuses(argv, capsys):
    with pytest.raises(SystemExit) as e:
        G.parse(argv)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "--no-repeat-ngram" in err or "--repetition-penalty" in err or "--min-length" in err


def _data(n=5):
    """The fields of data_handler.load's result that generate_response reads, for n single-turn dialogues without features."""
    dialogs = [("v%d" % i, i, [1], [4, 5, 6][:1 + i % 3], [4, 5], None, [4, 5, 6]) for i in range(n)]
    original = {"dialogs": [{"image_id": "v%d" % i, "dialog": [{"question": "a man", "answer": "walks"}]} for i in range(n)]}
    return dict(dialogs=dialogs, features=None, original=original)


@pytest.mark.parametrize("style", ["beam_search", "greedy", "sample"])
def test_values_reach_decode_searches(style, monkeypatch):
    seen = {}

    def fake(model, corpus, searches, vids, vocab, decode_style, maxlen, beam, penalty, nbest, **kw):
        seen.update(kw, decode_style=decode_style)
        one = {"beam_search": ([([4, 5], -1.0)], -1.0), "greedy": [2, 4, 5, 3], "sample": [([4, 5], -1.0)]}[decode_style]
        return {i: one for ids, n, _ in searches for i in ids[:n]}

    monkeypatch.setattr(G, "decode_searches", fake)
    corpus = types.SimpleNamespace(device="cpu")
    res = G.generate_response(None, _data(), corpus, VOCAB, decode_style=style, dialogues_per_search=2, no_repeat_ngram=3,
                              repetition_penalty=1.2, min_len=6)
    assert (seen["no_repeat_ngram"], seen["repetition_penalty"], seen["min_len"], seen["decode_style"]) == (3, 1.2, 6, style)
    assert [d["dialog"][0]["answer"] for d in res["dialogs"]] == ["a man"] * 5
    seen.clear()
    G.generate_response(None, _data(), corpus, VOCAB, decode_style=style, dialogues_per_search=2)
    assert (seen["no_repeat_ngram"], seen["repetition_penalty"], seen["min_len"]) == (0, 1.0, 1)
    with pytest.raises(ValueError):
        G.generate_response(None, _data(), corpus, VOCAB, decode_style="score", no_repeat_ngram=2)


def test_values_reach_the_decode_calls(monkeypatch):
    """decode_searches hands the constraints to beam search, greedy and sample alike, min_len to the two that finish hypotheses."""
    import torch
    from mtn_amd import data_handler as dh
    from mtn_amd import decode as D
    calls = []
    monkeypatch.setattr(dh, "make_batch", lambda corpus, index, pad, **kw: types.SimpleNamespace(n=index[-1]))
    monkeypatch.setattr(D, "beam_search_decode_many", lambda model, batch, *a, **kw: calls.append(("beam", kw)) or [([([4], -1.0)], -1.0)] * batch.n)
    monkeypatch.setattr(D, "greedy_decode_many", lambda model, batch, *a, **kw: calls.append(("greedy", kw)) or torch.zeros(batch.n, 3, dtype=torch.long))
    monkeypatch.setattr(D, "sample_decode_many", lambda model, batch, *a, **kw: calls.append(("sample", kw)) or [[([4], -1.0)]] * batch.n)
    searches = G.plan_searches(G.qa_lengths(_data()), 2)
    vids = {i: "v%d" % i for i in range(5)}
    for style in ("beam_search", "greedy", "sample"):
        calls.clear()
        res = G.decode_searches(None, None, searches, vids, VOCAB, style, 30, 5, 1.0, 5, sampling=dict(samples=2, seed=1),
                                no_repeat_ngram=2, repetition_penalty=1.3, min_len=4)
        assert sorted(res) == list(range(5)) and len(calls) == len(searches)
        for name, kw in calls:
            assert (kw["no_repeat_ngram"], kw["repetition_penalty"]) == (2, 1.3), name
            assert name == "greedy" or kw["min_len"] == 4
        calls.clear()
        G.decode_searches(None, None, searches, vids, VOCAB, style, 30, 5, 1.0, 5, sampling=dict(samples=2, seed=1))
        for name, kw in calls:
            assert (kw["no_repeat_ngram"], kw["repetition_penalty"]) == (0, 1.0), name
            assert name == "greedy" or kw["min_len"] == 1


def test_decode_keywords_are_checked_before_anything_runs():
    from mtn_amd import decode as D
    for kw in (dict(no_repeat_ngram=9), dict(no_repeat_ngram=-1), dict(repetition_penalty=0.5), dict(repetition_penalty=float("nan"))):
        with pytest.raises(ValueError):
            D._constraints(**dict(dict(no_repeat_ngram=0, repetition_penalty=1.0), **kw))
    assert D._constraints(0, 1.0) == (0, 1.0, False) and D._constraints(2, 1.0)[2] and D._constraints(0, 1.5)[2]
