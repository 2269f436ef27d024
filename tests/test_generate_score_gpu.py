"""`generate.py --decode-style score` on the GPU, end to end, on the mini AVSD fixture and the one-epoch checkpoint of
test_generate_gpu.py: a candidates file that holds every QA's own answer as gt_index among distractors.  Bucketed multi-QA scoring
against one QA per pass at its own shape (--no-buckets), the result JSON, the logged corpus numbers, and beam search before and after."""
import json
import logging
import math
import re

import pytest
import torch

from tests.test_generate_gpu import BEAM, MAXLEN, NBEST, PENALTY, _reference_side, run  # noqa: F401  (run: the module's fixture)

pytestmark = pytest.mark.gpu
BAR = {"fp32": 1e-3, "bf16": 1e-2}            # the bars test_generate_gpu.py holds bucketed against single-QA scores to


def _candidates_file(run, raw):
    """Per QA: its own answer at a varying position among answers of other QAs, an unknown word, an empty text; one QA has no entry
    (falls back to its own answer), one has no gt_index."""
    answers = [t["answer"] for d in raw["dialogs"] for t in d["dialog"]]
    spec, qa = {}, 0
    for d in raw["dialogs"]:
        for t, turn in enumerate(d["dialog"]):
            others = [answers[(qa + k) % len(answers)] for k in (1, 3, 5, 8)] + ["zzz-never-seen " + turn["answer"], ""]
            others = others[:2 + qa % 5]
            gt = qa % (len(others) + 1)
            cands = others[:gt] + [turn["answer"]] + others[gt:]
            if qa != 2:
                spec["%s_%d" % (d["image_id"], t)] = {"candidates": cands, "gt_index": gt} if qa != 5 else {"candidates": cands}
            qa += 1
    path = str(run["tmp"] / "candidates.json")
    json.dump(spec, open(path, "w"))
    return path, spec


def _flat_scores(result):
    return [t["scores"] for d in result["dialogs"] for t in d["dialog"]]


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_bucketed_scores_equal_per_qa_scores(run, dtype, caplog):
    from mtn_amd import decode as D
    from mtn_amd import generate as G
    vocab, targs, data, corpus, model, _ = _reference_side(run, dtype, False)
    raw = data["original"]
    path, spec = _candidates_file(run, raw)
    kw = dict(maxlen=MAXLEN, beam=BEAM, penalty=PENALTY, nbest=NBEST)
    D._SESSIONS.clear()
    beam_before = G.generate_response(model, data, corpus, vocab, decode_style="beam_search", **kw)
    caplog.set_level(logging.INFO)
    caplog.clear()
    bucketed = G.generate_response(model, data, corpus, vocab, decode_style="score", candidates=path, **kw)
    text = caplog.text
    records = [r.getMessage() for r in caplog.records]
    assert any(k[-1] == "score" for k in D._SESSIONS), "score sessions carry their own mode in the cache key"
    assert not any(isinstance(s[0], D.MegaDecodeSession) for k, s in D._SESSIONS.items() if k[-1] == "score")
    beam_after = G.generate_response(model, data, corpus, vocab, decode_style="beam_search", **kw)
    assert beam_after == beam_before                                           # the score run disturbed no search
    single = G.generate_response(model, data, corpus, vocab, decode_style="score", candidates=path, buckets=False, **kw)

    # the reference's structure, plus "scores" in input order
    plain = G.build_result(raw, False, [t["answer"] for d in bucketed["dialogs"] for t in d["dialog"]])
    assert [d["image_id"] for d in bucketed["dialogs"]] == [d["image_id"] for d in raw["dialogs"]]
    cands = G.load_candidates(path, raw, vocab)
    worst, qa = 0.0, 0
    for db, ds, dp in zip(bucketed["dialogs"], single["dialogs"], plain["dialogs"]):
        for tb, ts, tp in zip(db["dialog"], ds["dialog"], dp["dialog"]):
            assert {k: v for k, v in tb.items() if k != "scores"} == tp
            sb, ss = tb["scores"], ts["scores"]
            assert [s["candidate"] for s in sb] == cands[qa]["texts"] == [s["candidate"] for s in ss]
            assert [s["n_tokens"] for s in sb] == [len(t) + 1 for t in cands[qa]["tokens"]] == [s["n_tokens"] for s in ss]
            for a, b in zip(sb, ss):
                assert set(a) == {"candidate", "score", "logp", "n_tokens"}
                assert abs(a["score"] - (a["logp"] + PENALTY * a["n_tokens"])) < 1e-9
                err = abs(a["score"] - b["score"]) / max(1.0, abs(b["score"]))
                worst = max(worst, err)
                assert err < BAR[dtype], (qa, a, b)
            assert tb["answer"] == sb[G.candidate_order([s["score"] for s in sb])[0]]["candidate"]
            qa += 1
    print(f"{dtype}: bucketed vs --no-buckets worst score error {worst:.3g} (bar {BAR[dtype]:g})")
    assert qa == len(cands) and cands[2]["texts"] == [raw["dialogs"][0]["dialog"][2]["answer"]] and not cands[2]["ranked"]

    # the log: CAND lines best first per QA, and the corpus numbers recomputed from the returned scores
    n_cand = sum(1 for m in records if re.fullmatch(r"CAND\[\d+\]: .*  \( \S+, \S+, \d+ \)", m))
    assert n_cand == sum(len(c["texts"]) for c in cands)
    firsts = [float(re.fullmatch(r"CAND\[1\]: .*  \( (\S+), \S+, \d+ \)", m).group(1)) for m in records if m.startswith("CAND[1]: ")]
    flat = _flat_scores(bucketed)
    assert len(firsts) == len(flat) and all(abs(f - max(s["score"] for s in sc)) < 1e-5 for f, sc in zip(firsts, flat))
    lp = sum(sc[c["gt_index"]]["logp"] for sc, c in zip(flat, cands) if c["gt_index"] is not None)
    nt = sum(sc[c["gt_index"]]["n_tokens"] for sc, c in zip(flat, cands) if c["gt_index"] is not None)
    m = re.search(r"perplexity = (\S+)  \( (\d+) answers, (\d+) tokens", text)
    assert m and int(m.group(2)) == len(cands) - 1 and int(m.group(3)) == nt
    assert abs(float(m.group(1)) - math.exp(-lp / nt)) <= 1e-8 * math.exp(-lp / nt)
    want = G.score_metrics([dict(score=[s["score"] for s in sc], logp=[s["logp"] for s in sc], n_tokens=[s["n_tokens"] for s in sc],
                                 gt_index=c["gt_index"], ranked=c["ranked"]) for sc, c in zip(flat, cands)])
    m = re.search(r"MRR = (\S+)  R@1 = (\S+)  R@5 = (\S+)  R@10 = (\S+)  mean rank = (\S+)  \( (\d+) QAs", text)
    assert m and int(m.group(6)) == want["n_ranked"] == len(cands) - 2
    got = [float(m.group(i)) for i in range(1, 6)]
    assert all(abs(g - w) < 1e-4 for g, w in zip(got, [want["mrr"], want["r1"], want["r5"], want["r10"], want["mean_rank"]]))


def test_own_answers_without_a_candidates_file(run, caplog):
    """Without --candidates every QA's own answer is scored — the labelled set's with --undisclosed-only — and only the perplexity is
    logged."""
    from mtn_amd import generate as G
    vocab, targs, data, corpus, model, _ = _reference_side(run, "bf16", True)
    labelled = json.load(open(run["full"]))
    caplog.set_level(logging.INFO)
    res = G.generate_response(model, data, corpus, vocab, maxlen=MAXLEN, penalty=PENALTY, decode_style="score", undisclosed_only=True,
                              ref_data=labelled)
    assert all(len(d["dialog"]) == 1 for d in res["dialogs"])
    for d, ref in zip(res["dialogs"], labelled["dialogs"]):
        (turn,) = d["dialog"]
        assert turn["answer"] == ref["dialog"][-1]["answer"] == turn["scores"][0]["candidate"] and len(turn["scores"]) == 1
        assert turn["scores"][0]["n_tokens"] == len(ref["dialog"][-1]["answer"].split()) + 1
    flat = _flat_scores(res)
    ppl = math.exp(-sum(s[0]["logp"] for s in flat) / sum(s[0]["n_tokens"] for s in flat))
    m = re.search(r"perplexity = (\S+)  \( (\d+) answers", caplog.text)
    assert m and int(m.group(2)) == len(flat) and abs(float(m.group(1)) - ppl) <= 1e-8 * ppl
    assert "MRR" not in caplog.text and 1.0 < ppl < len(vocab) ** 2
