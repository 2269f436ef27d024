"""`python generate.py --ensemble-model ...` (mtn_amd.generate) on the GPU, end to end, on the mini AVSD fixture and the two checkpoints of a
two-epoch run (built the way tests/test_generate_constrain_gpu.py builds its one): beam search and score, fp32.  The result JSON has the
reference's structure; with --no-buckets every QA's logged n-best list is what decode.beam_search_decode_many gives for that QA alone with a
decode.Ensemble of the same checkpoints built by hand; the score run's logged perplexity is the one its returned token log-probabilities give;
and the same command without the ensemble flags gives the single-model output."""
import json
import logging
import math
import os
import re

import pytest
import torch

from tests.test_dataset_frontend import _features

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
BEAM, PENALTY, NBEST, MAXLEN = 3, 1.0, 3, 12
WEIGHTS = ["3", "1"]


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """Two epochs of training through mtn_amd.train.main -> one conf, checkpoints <prefix>_1 and <prefix>_2."""
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    from mtn_amd import train
    tmp = tmp_path_factory.mktemp("gen_ensemble")
    raw = json.load(open(os.path.join(GOLD, "mini_avsd.json")))
    _, fea_path = _features(tmp, raw)
    prefix = str(tmp / "exp" / "mtn")
    train.main(["--fea-type", "i3d", "vgg", "--train-path", fea_path, "--train-set", os.path.join(GOLD, "mini_avsd.json"),
                "--num-epochs", "2", "--batch-size", "4", "--max-length", "256", "--model", prefix, "--include-caption", "caption,summary",
                "--separate-caption", "1", "--max-history-length", "3", "--nb-blocks", "1", "--d-model", "128", "--d-ff", "256",
                "--att-h", "4", "--dropout", "0.1", "--warmup-steps", "20", "--report-interval", "1000"])
    assert os.path.exists(prefix + "_1.pth.tar") and os.path.exists(prefix + "_2.pth.tar")
    return dict(tmp=tmp, fea_path=fea_path, prefix=prefix, full=os.path.join(GOLD, "mini_avsd.json"))


def _argv(run, style, out, extra=()):
    return ["--gpu", "0", "--test-path", run["fea_path"], "--test-set", run["full"], "--model-conf", run["prefix"] + ".conf",
            "--model", run["prefix"] + "_1", "--beam", str(BEAM), "--penalty", str(PENALTY), "--nbest", str(NBEST), "--maxlen", str(MAXLEN),
            "--output", out, "--decode-style", style, "--undisclosed-only", "0", "--compute-dtype", "fp32"] + list(extra)


def _ens_flags(run):
    return ["--ensemble-model", run["prefix"] + "_2", "--ensemble-conf", run["prefix"] + ".conf", "--ensemble-weights"] + WEIGHTS


def _logged_hyps(records):
    out = []
    for rec in records:
        msg = rec.getMessage()
        if re.fullmatch(r"\d+ \S+_\d+", msg):
            out.append([])
        else:
            m = re.fullmatch(r"HYP\[\d+\]: (.*)  \( (\S+) \)", msg)
            if m:
                out[-1].append((m.group(1), float(m.group(2))))
    return out


def _main(caplog, argv):
    from mtn_amd import generate as G
    caplog.clear()
    caplog.set_level(logging.INFO)
    result = G.main(argv)
    return result, list(caplog.records)


def _same_structure(result, raw):
    assert list(result) == ["dialogs"] and len(result["dialogs"]) == len(raw["dialogs"])
    for got, want in zip(result["dialogs"], raw["dialogs"]):
        assert got["image_id"] == want["image_id"] and len(got["dialog"]) == len(want["dialog"])
        for g, w in zip(got["dialog"], want["dialog"]):
            assert g["question"] == w["question"] and isinstance(g["answer"], str)


def test_beam_search_with_an_ensemble_equals_decode_called_directly(run, caplog):
    from mtn_amd import data_handler as dh
    from mtn_amd import decode as D
    from mtn_amd import generate as G
    D._SESSIONS.clear()
    raw = json.load(open(run["full"]))
    out = str(run["tmp"] / "ens_beam.json")
    result, records = _main(caplog, _argv(run, "beam_search", out, _ens_flags(run) + ["--no-buckets"]))
    assert json.load(open(out)) == result
    _same_structure(result, raw)
    logged = _logged_hyps(records)
    assert any("ensemble of 2 members" in r.getMessage() for r in records)
    answers = [t["answer"] for d in result["dialogs"] for t in d["dialog"]]
    # the bucketed run (padded multi-QA searches): the same hypotheses, to the fp32 bar of tests/test_generate_gpu.py
    bucketed, records_b = _main(caplog, _argv(run, "beam_search", out, _ens_flags(run)))
    logged_b = _logged_hyps(records_b)
    assert len(logged_b) == len(logged) == len(answers) > 0
    for got, want in zip(logged_b, logged):
        assert [g[0] for g in got] == [w[0] for w in want]
        assert max(abs(g[1] - w[1]) for g, w in zip(got, want)) < 1e-3
    # decode called directly with an Ensemble built by hand, one QA per search at its own shape
    vocab, targs = G.load_conf(run["prefix"] + ".conf")
    data = dh.load(targs.fea_type, run["fea_path"], run["full"], vocab=vocab, include_caption=targs.include_caption,
                   separate_caption=bool(targs.separate_caption), max_history_length=targs.max_history_length,
                   merge_source=bool(targs.merge_source), undisclosed_only=False)
    dev = torch.device("cuda", 0)
    members = [G.build_model(vocab, targs, dh.feature_shape(data), G.load_state_dict(run["prefix"] + "_%d.pth.tar" % k), "fp32", dev)
               for k in (1, 2)]
    ens = D.Ensemble(members, weights=[float(w) for w in WEIGHTS])
    corpus = dh.DeviceCorpus(data, dev)
    lens = G.qa_lengths(data)
    vids = {it[1]: it[0] for it in data["dialogs"]}
    vocablist = sorted(vocab.keys(), key=lambda s: vocab[s])
    sos, eos, unk, pad = vocab["<sos>"], vocab["<eos>"], vocab["<unk>"], vocab["<blank>"]
    differs = 0
    for qa, l in enumerate(lens):
        index = ([vids[qa]], [qa], list(l[0]), l[1], l[2], l[3], l[4], 1)
        batch = dh.make_batch(corpus, index, pad, separate_caption=True)
        nbest, _ = D.beam_search_decode_many(ens, batch, MAXLEN, sos, unk, eos, pad, beam=BEAM, penalty=PENALTY, nbest=NBEST)[0]
        want = [(G.detokenize(t, vocablist, eos), s) for t, s in nbest[:NBEST]]
        assert [w[0] for w in want] == [g[0] for g in logged[qa]], qa
        assert max(abs(w[1] - g[1]) for w, g in zip(want, logged[qa])) < 1e-3
        assert answers[qa] == want[0][0]
        solo, _ = D.beam_search_decode_many(members[0], batch, MAXLEN, sos, unk, eos, pad, beam=BEAM, penalty=PENALTY, nbest=NBEST)[0]
        differs += [(t, round(s, 3)) for t, s in solo] != [(t, round(s, 3)) for t, s in nbest]
    assert differs > 0, "the second checkpoint changed no QA's n-best list: the ensemble run shows nothing"
    D._SESSIONS.clear()


def test_score_with_an_ensemble_logs_its_own_perplexity(run, caplog):
    from mtn_amd import decode as D
    D._SESSIONS.clear()
    raw = json.load(open(run["full"]))
    out = str(run["tmp"] / "ens_score.json")
    result, records = _main(caplog, _argv(run, "score", out, _ens_flags(run)))
    _same_structure(result, raw)
    ppl = [r.getMessage() for r in records if r.getMessage().startswith("perplexity = ")]
    assert len(ppl) == 1
    m = re.match(r"perplexity = (\S+)  \( (\d+) answers, (\d+) tokens", ppl[0])
    turns = [t for d in result["dialogs"] for t in d["dialog"]]
    assert all(len(t["scores"]) == 1 for t in turns)                            # no --candidates: every QA is scored on its own answer
    lp = sum(t["scores"][0]["logp"] for t in turns)
    nt = sum(t["scores"][0]["n_tokens"] for t in turns)
    assert int(m.group(2)) == len(turns) and int(m.group(3)) == nt
    assert abs(float(m.group(1)) - math.exp(-lp / nt)) <= 1e-8 * math.exp(-lp / nt)
    # ... and it is the ENSEMBLE's: neither member's own
    single, records1 = _main(caplog, _argv(run, "score", out))
    lp1 = sum(t["scores"][0]["logp"] for d in single["dialogs"] for t in d["dialog"])
    assert abs(lp1 - lp) > 1e-3 * abs(lp)
    D._SESSIONS.clear()


def test_without_the_flags_nothing_changes(run, caplog, monkeypatch):
    """The same command without the ensemble flags: the single-model output, and decode never sees an Ensemble."""
    from mtn_amd import decode as D
    from mtn_amd import generate as G
    D._SESSIONS.clear()
    seen = []
    real = G.decode_searches
    monkeypatch.setattr(G, "decode_searches", lambda model, *a, **k: (seen.append(type(model).__name__), real(model, *a, **k))[1])
    out = str(run["tmp"] / "plain_beam.json")
    plain, records = _main(caplog, _argv(run, "beam_search", out))
    assert seen == ["EncoderDecoder"] and not any(isinstance(s[0], (D.EnsembleSession, D.EnsembleMegaSession)) for s in D._SESSIONS.values())
    # an ensemble whose second member weighs nothing IS the first member: the same answers and scores
    solo, records_s = _main(caplog, _argv(run, "beam_search", out, ["--ensemble-model", run["prefix"] + "_2", "--ensemble-weights", "1", "0"]))
    assert seen == ["EncoderDecoder", "Ensemble"]
    a, b = _logged_hyps(records), _logged_hyps(records_s)
    assert len(a) == len(b) > 0
    for x, y in zip(a, b):
        assert [h[0] for h in x] == [h[0] for h in y] and max(abs(p[1] - q[1]) for p, q in zip(x, y)) < 1e-3
    assert [t["answer"] for d in plain["dialogs"] for t in d["dialog"]] == [t["answer"] for d in solo["dialogs"] for t in d["dialog"]]
    D._SESSIONS.clear()
