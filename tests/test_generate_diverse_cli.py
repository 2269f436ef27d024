"""--beam-groups / --diversity-penalty of mtn_amd.generate without a GPU: parser defaults and refusals, and the way the values travel
through generate_response and decode_searches into beam_search_decode_many."""
import types

import pytest

from mtn_amd import generate as G

VOCAB = {"<unk>": 0, "<blank>": 1, "<sos>": 2, "<eos>": 3, "a": 4, "man": 5, "walks": 6}


def test_parser_defaults_are_off():
    a = G.parse([])
    assert (a.beam_groups, a.diversity_penalty) == (1, 0.0)
    a = G.parse(["--decode-style", "beam_search", "--beam", "6", "--beam-groups", "3", "--diversity-penalty", "0.5"])
    assert (a.beam, a.beam_groups, a.diversity_penalty) == (6, 3, 0.5)
    a = G.parse(["--decode-style", "beam_search", "--beam", "4", "--beam-groups", "2"])          # groups without a penalty: allowed
    assert (a.beam_groups, a.diversity_penalty) == (2, 0.0)
    # the defaults spelled out go with every style
    for style in ("greedy", "sample", "score", "beam_search"):
        assert G.parse(["--decode-style", style, "--beam-groups", "1", "--diversity-penalty", "0"]).decode_style == style


BS = ["--decode-style", "beam_search", "--beam", "4"]


@pytest.mark.parametrize("argv,flag", [
    (BS + ["--beam-groups", "3"], "--beam-groups"),                                     # does not divide the beam
    (BS + ["--beam-groups", "0"], "--beam-groups"),
    (BS + ["--beam-groups", "8"], "--beam-groups"),
    (BS + ["--beam-groups", "2", "--diversity-penalty", "-0.1"], "--diversity-penalty"),
    (BS + ["--beam-groups", "2", "--diversity-penalty", "nan"], "--diversity-penalty"),
    (BS + ["--beam-groups", "2", "--diversity-penalty", "inf"], "--diversity-penalty"),
    (BS + ["--diversity-penalty", "0.5"], "--diversity-penalty"),                       # a penalty with one group
    (["--decode-style", "greedy", "--beam", "4", "--beam-groups", "2"], "--beam-groups"),
    (["--decode-style", "sample", "--beam", "4", "--beam-groups", "2"], "--beam-groups"),
    (["--decode-style", "score", "--beam", "4", "--beam-groups", "2"], "--beam-groups"),
    (["--decode-style", "greedy", "--diversity-penalty", "0.5"], "--diversity-penalty"),
    (["--decode-style", "sample", "--diversity-penalty", "0.5"], "--diversity-penalty"),
    (["--decode-style", "score", "--diversity-penalty", "0.5"], "--diversity-penalty"),
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


def test_values_reach_decode_searches(monkeypatch):
    seen = {}

    def fake(model, corpus, searches, vids, vocab, decode_style, maxlen, beam, penalty, nbest, **kw):
        seen.update(kw, decode_style=decode_style, beam=beam)
        one = {"beam_search": ([([4, 5], -1.0)], -1.0), "greedy": [2, 4, 5, 3], "sample": [([4, 5], -1.0)]}[decode_style]
        return {i: one for ids, n, _ in searches for i in ids[:n]}

    monkeypatch.setattr(G, "decode_searches", fake)
    corpus = types.SimpleNamespace(device="cpu")
    res = G.generate_response(None, _data(), corpus, VOCAB, decode_style="beam_search", beam=6, dialogues_per_search=2, beam_groups=3,
                              diversity_penalty=0.5)
    assert (seen["beam"], seen["beam_groups"], seen["diversity_penalty"]) == (6, 3, 0.5)
    assert [d["dialog"][0]["answer"] for d in res["dialogs"]] == ["a man"] * 5
    seen.clear()
    G.generate_response(None, _data(), corpus, VOCAB, decode_style="beam_search", dialogues_per_search=2)
    assert (seen["beam_groups"], seen["diversity_penalty"]) == (1, 0.0)
    for style in ("greedy", "sample", "score"):
        for kw in (dict(beam_groups=2), dict(diversity_penalty=0.5)):
            with pytest.raises(ValueError, match="beam_groups"):
                G.generate_response(None, _data(), corpus, VOCAB, decode_style=style, beam=4, dialogues_per_search=2, **kw)
    for kw in (dict(beam_groups=3), dict(beam_groups=2, diversity_penalty=-1.0), dict(diversity_penalty=0.5)):
        with pytest.raises(ValueError):
            G.generate_response(None, _data(), corpus, VOCAB, decode_style="beam_search", beam=4, dialogues_per_search=2, **kw)


def test_values_reach_beam_search_decode_many(monkeypatch):
    from mtn_amd import data_handler as dh
    from mtn_amd import decode as D
    calls = []
    monkeypatch.setattr(dh, "make_batch", lambda corpus, index, pad, **kw: types.SimpleNamespace(n=index[-1]))
    monkeypatch.setattr(D, "beam_search_decode_many", lambda model, batch, *a, **kw: calls.append(kw) or [([([4], -1.0)], -1.0)] * batch.n)
    searches = G.plan_searches(G.qa_lengths(_data()), 2)
    vids = {i: "v%d" % i for i in range(5)}
    res = G.decode_searches(None, None, searches, vids, VOCAB, "beam_search", 30, 6, 1.0, 5, beam_groups=3, diversity_penalty=0.5)
    assert sorted(res) == list(range(5)) and len(calls) == len(searches)
    assert all((kw["beam"], kw["beam_groups"], kw["diversity_penalty"]) == (6, 3, 0.5) for kw in calls)
    calls.clear()
    G.decode_searches(None, None, searches, vids, VOCAB, "beam_search", 30, 6, 1.0, 5)
    assert all((kw["beam_groups"], kw["diversity_penalty"]) == (1, 0.0) for kw in calls)


def test_decode_keywords_are_checked_before_anything_runs():
    from mtn_amd import decode as D
    for beam, G_, lam in ((4, 3, 0.0), (4, 0, 0.0), (4, -2, 0.0), (4, 2, -0.5), (4, 2, float("nan")), (4, 2, float("inf")), (4, 1, 0.5), (4, 1.5, 0.0)):
        with pytest.raises(ValueError):
            D._diverse(beam, G_, lam)
    assert D._diverse(5, 1, 0.0) == (1, 0.0) and D._diverse(6, 3, 0.5) == (3, 0.5) and D._diverse(4, 4, 0) == (4, 0.0)
    # a model is never touched: the check comes first
    with pytest.raises(ValueError):
        D.beam_search_decode_many(None, None, 16, 2, 0, 3, 1, beam=4, beam_groups=3)
    with pytest.raises(ValueError):
        D.beam_search_decode(None, types.SimpleNamespace(query=types.SimpleNamespace(size=lambda i: 1)), 16, 2, 0, 3, 1, beam=4, diversity_penalty=0.5)
