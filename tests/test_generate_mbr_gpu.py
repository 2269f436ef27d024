"""`python generate.py --mbr N` (mtn_amd.generate) on the GPU, end to end, on the mini AVSD fixture and the one-epoch checkpoint of
test_generate_gpu.py.  Selection adds nothing and loses nothing: the HYP lines of a --mbr run are those of the run without it, in
another order — the order, the `MBR:` line and the answers the definition (tests/mbr_refs.py) gives on the search's own hypotheses —
and the JSON "mbr" lists say what the log says."""
import json
import logging
import re

import pytest

from tests import mbr_refs as R
from tests.test_generate_gpu import _argv, run  # noqa: F401  (run: the module's fixture)

pytestmark = pytest.mark.gpu
S = 4


def _main(caplog, argv):
    """(result, per QA in log order: ([(hypothesis, score as logged)], the MBR line's fields or None))."""
    from mtn_amd import generate as G
    caplog.clear()
    caplog.set_level(logging.INFO)
    result = G.main(argv)
    out = []
    for rec in caplog.records:
        msg = rec.getMessage()
        if re.fullmatch(r"\d+ \S+_\d+", msg):
            out.append(([], None))
        elif re.fullmatch(r"HYP\[\d+\]: .*  \( \S+ \)", msg):
            m = re.fullmatch(r"HYP\[(\d+)\]: (.*)  \( (\S+) \)", msg)
            assert int(m.group(1)) == len(out[-1][0]) + 1
            out[-1][0].append((m.group(2), m.group(3)))
        elif msg.startswith("MBR: "):
            assert out[-1][1] is None
            out[-1] = (out[-1][0], msg[len("MBR: "):].split(" "))
    return result, out


def _vocablist(run):
    from mtn_amd import generate as G
    vocab, _ = G.load_conf(run["prefix"] + ".conf")
    return vocab, sorted(vocab, key=vocab.get)


def _json_matches_log(result, logged):
    turns = [t for d in result["dialogs"] for t in d["dialog"]]
    assert len(turns) == len(logged)
    for turn, (hyps, mbr) in zip(turns, logged):
        assert turn["answer"] == hyps[0][0]
        assert [h["hypothesis"] for h in turn["mbr"]] == [h for h, _ in hyps]
        assert ["%f" % h["score"] for h in turn["mbr"]] == [s for _, s in hyps]
        assert [repr(h["expected"]) for h in turn["mbr"]] == mbr


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_sample_mbr_reorders_the_same_samples_as_the_definition_says(run, dtype, caplog, monkeypatch):
    from mtn_amd import decode as D
    from mtn_amd import generate as G
    vocab, vl = _vocablist(run)
    eos = vocab["<eos>"]
    out = str(run["tmp"] / f"mbr_sample_{dtype}.json")
    argv = _argv(run, "sample", dtype, 0, out) + ["--temperature", "0.9", "--top-k", "20", "--top-p", "0.9", "--samples", str(S), "--sample-seed", "5"]
    plain, plain_log = _main(caplog, argv)
    assert all(m is None for _, m in plain_log) and all("mbr" not in t for d in plain["dialogs"] for t in d["dialog"])
    D._SESSIONS.clear()                                      # (every run builds its own model: the plain run's sessions are not this run's)
    fallbacks = D.MegaDecodeSession.FALLBACKS
    traces, seen = [], []
    real = D.sample_decode_many
    monkeypatch.setattr(D, "sample_decode_many", lambda *a, **k: seen.append(k.get("mbr")) or real(*a, **dict(k, trace=traces)))
    result, logged = _main(caplog, argv + ["--mbr", "2"])
    monkeypatch.undo()
    assert json.load(open(out)) == result
    assert seen and set(seen) == {2}                                                  # uniform weights: selected inside the search
    if dtype == "bf16":
        mega = [s[0] for s in D._SESSIONS.values() if isinstance(s[0], D.MegaDecodeSession)]
        assert mega and all(s._sample_key[-1] == 2 for s in mega if getattr(s, "_sample_key", None)), "bf16 at d_model 128 must sample on the persistent step"
        assert D.MegaDecodeSession.FALLBACKS == fallbacks
    by_key = {}
    for keys, tok, _, _ in traces:
        for r, k in enumerate(keys):
            by_key.setdefault(k, tok[:, r:r + 1])
    n_qa = len(logged)
    assert n_qa == len(plain_log) > 0 and sorted(by_key) == list(range(n_qa * S))
    moved = 0
    for qa in range(n_qa):
        hyps, mbr = logged[qa]
        assert sorted(hyps) == sorted(plain_log[qa][0]), qa                           # the same samples with the same scores
        mine = [R.cut_log(by_key[qa * S + s], eos)[0] for s in range(S)]
        _, expected, best, order = R.select(mine, 2)
        assert [h for h, _ in hyps] == [G.detokenize(mine[j], vl, eos) for j in order.tolist()], qa
        assert mbr == [repr(float(expected[j])) for j in order.tolist()], qa
        moved += hyps[0] != plain_log[qa][0][0]
    _json_matches_log(result, logged)
    print(f"{dtype}: the answer differs from the best-scoring sample in {moved} of {n_qa} QAs")


@pytest.mark.parametrize("extra", [[], ["--beam-groups", "5", "--diversity-penalty", "0.5"]], ids=["plain", "beam-groups"])
def test_beam_search_mbr_reorders_the_nbest_list(run, extra, caplog, monkeypatch):
    from mtn_amd import decode as D
    from mtn_amd import generate as G
    vocab, vl = _vocablist(run)
    eos = vocab["<eos>"]
    out = str(run["tmp"] / f"mbr_beam_{len(extra)}.json")
    argv = _argv(run, "beam_search", "bf16", 0, out) + extra                         # (--beam 5 --nbest 5)
    _, plain_log = _main(caplog, argv)
    calls, final = [], {}
    real_rerank, real_searches = D.mbr_rerank, G.decode_searches
    monkeypatch.setattr(D, "mbr_rerank", lambda lists, *a, **k: calls.append(([list(l) for l in lists], a, k, real_rerank(lists, *a, **k))) or calls[-1][3])
    monkeypatch.setattr(G, "decode_searches", lambda *a, **k: final.update(real_searches(*a, **k)) or final)
    result, logged = _main(caplog, argv + ["--mbr", "4", "--mbr-weights", "score"])
    monkeypatch.undo()
    assert json.load(open(out)) == result and calls
    for lists, a, k, got in calls:                                                    # every launch against the definition
        assert a == (4,) and k == dict(weights="score", temperature=1.0)
        for l, g in zip(lists, got):
            assert 0 < len(l) <= 5
            _, expected, _, order = R.select([h for h, _ in l], 4, R.score_weights([s for _, s in l], 1.0))
            assert g == [(l[j][0], l[j][1], float(expected[j])) for j in order.tolist()]
    n_qa = len(logged)
    assert n_qa == len(plain_log) == len(final) > 0
    for qa in range(n_qa):
        hyps, mbr = logged[qa]
        assert sorted(hyps) == sorted(plain_log[qa][0]), qa                           # the same n-best list
        triples = final[qa][0]
        assert hyps == [(G.detokenize(t, vl, eos), "%f" % s) for t, s, _ in triples] and mbr == [repr(e) for _, _, e in triples], qa
    _json_matches_log(result, logged)
