"""`python generate.py --no-repeat-ngram 2 --min-length 6` (mtn_amd.generate) on the GPU, end to end, on the mini AVSD fixture and a
one-epoch checkpoint (the `run` fixture of tests/test_generate_gpu.py, copied): beam search and greedy, fp32 and bf16.  Every QA decoded
inside a bucketed, padded multi-QA search must give what the --no-buckets run (one QA per search at its own shape) gives — to the bars of
tests/test_generate_gpu.py: fp32 the same hypotheses and scores within 1e-3; bf16 the best score within 1e-2 (relative, floor 1) and the
same best hypothesis unless one of that QA's two searches met a tie; greedy the same text — and no logged hypothesis repeats a bigram.  Then
--decode-style sample --repetition-penalty 1.3: repeatable under one seed, and (fp32, where a row's arithmetic does not depend on the rows
beside it) the same whatever --dialogues-per-search."""
import json
import logging
import os
import re

import pytest
import torch

from tests.constrain_refs import has_repeated_ngram
from tests.test_dataset_frontend import _features

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
BEAM, PENALTY, NBEST = 5, 1.0, 5


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """One epoch of training through mtn_amd.train.main (d_model 128: bf16 decodes on the persistent step) -> conf + checkpoint."""
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    from mtn_amd import train
    tmp = tmp_path_factory.mktemp("gen_constrain")
    raw = json.load(open(os.path.join(GOLD, "mini_avsd.json")))
    _, fea_path = _features(tmp, raw)
    prefix = str(tmp / "exp" / "mtn")
    train.main(["--fea-type", "i3d", "vgg", "--train-path", fea_path, "--train-set", os.path.join(GOLD, "mini_avsd.json"),
                "--num-epochs", "1", "--batch-size", "4", "--max-length", "256", "--model", prefix, "--include-caption", "caption,summary",
                "--separate-caption", "1", "--max-history-length", "3", "--nb-blocks", "1", "--d-model", "128", "--d-ff", "256",
                "--att-h", "4", "--dropout", "0.1", "--warmup-steps", "20", "--report-interval", "1000"])
    return dict(tmp=tmp, fea_path=fea_path, prefix=prefix, full=os.path.join(GOLD, "mini_avsd.json"))


def _argv(run, style, dtype, out, extra=()):
    return ["--gpu", "0", "--test-path", run["fea_path"], "--test-set", run["full"], "--model-conf", run["prefix"] + ".conf",
            "--model", run["prefix"] + "_1", "--beam", str(BEAM), "--penalty", str(PENALTY), "--nbest", str(NBEST), "--output", out,
            "--decode-style", style, "--undisclosed-only", "0", "--compute-dtype", dtype] + list(extra)


def _logged_hyps(records):
    """Per QA (log order): beam / sample -> [(hypothesis string, score)], greedy -> hypothesis string."""
    out = []
    for rec in records:
        msg = rec.getMessage()
        if re.fullmatch(r"\d+ \S+_\d+", msg):
            out.append([])
        elif re.fullmatch(r"HYP\[\d+\]: .*  \( \S+ \)", msg):
            m = re.fullmatch(r"HYP\[\d+\]: (.*)  \( (\S+) \)", msg)
            out[-1].append((m.group(1), float(m.group(2))))
        elif msg.startswith("HYP: "):
            out[-1] = msg[len("HYP: "):]
    return out


def _main(caplog, argv):
    from mtn_amd import generate as G
    caplog.clear()
    caplog.set_level(logging.INFO)
    result = G.main(argv)
    return result, _logged_hyps(caplog.records)


def _no_repeat(text, N):
    return not has_repeated_ngram([hash(w) for w in text.split()], N)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("style", ["beam_search", "greedy"])
def test_constrained_generate_equals_its_no_buckets_run(run, style, dtype, caplog, monkeypatch):
    from mtn_amd import decode as D
    con = ["--no-repeat-ngram", "2", "--min-length", "6"]
    # the QAs one of whose searches (bucketed or alone) met a tie in a row's head and so ran step by step: per search, not per run
    from mtn_amd import generate as G
    tied, flags = set(), []
    real_search, real_many, real_run = D.MegaDecodeSession.search, D.beam_search_decode_many, G.decode_searches

    def search(self, *a, **k):
        r = real_search(self, *a, **k)
        flags[-1] = flags[-1] or r is None
        return r

    def many(*a, **k):
        flags.append(False)
        return real_many(*a, **k)

    def run_searches(model, corpus, searches, *a, **k):
        del flags[:]
        res = real_run(model, corpus, searches, *a, **k)
        assert len(flags) == len(searches)
        tied.update(i for (ids, n_real, _), tie in zip(searches, flags) if tie for i in ids[:n_real])
        return res

    if style == "beam_search":
        monkeypatch.setattr(D.MegaDecodeSession, "search", search)
        monkeypatch.setattr(D, "beam_search_decode_many", many)
        monkeypatch.setattr(G, "decode_searches", run_searches)
    D._SESSIONS.clear()
    fallbacks = D.MegaDecodeSession.FALLBACKS
    out = str(run["tmp"] / f"con_{style}_{dtype}.json")
    result, logged = _main(caplog, _argv(run, style, dtype, out, con))
    assert json.load(open(out)) == result
    mega_used = any(isinstance(s[0], D.MegaDecodeSession) for s in D._SESSIONS.values())
    single, logged1 = _main(caplog, _argv(run, style, dtype, out, con + ["--no-buckets"]))
    if dtype == "bf16":
        assert mega_used, "bf16 at d_model 128 must decode on the persistent step"
        assert D.MegaDecodeSession.FALLBACKS == fallbacks
    n_qa = len(logged)
    assert n_qa == len(logged1) > 0
    answers = [t["answer"] for d in result["dialogs"] for t in d["dialog"]]
    for qa in range(n_qa):
        got, want = logged[qa], logged1[qa]
        if style == "greedy":
            assert got == want == answers[qa], qa
            assert _no_repeat(got, 2), (qa, got)
            continue
        assert len(got) == len(want) and answers[qa] == got[0][0]
        if dtype == "fp32":
            assert [g[0] for g in got] == [w[0] for w in want], qa
            assert max(abs(g[1] - w[1]) for g, w in zip(got, want)) < 1e-3, qa
        else:
            if qa not in tied:
                assert got[0][0] == want[0][0], qa
            assert abs(got[0][1] - want[0][1]) < 1e-2 * max(1.0, abs(want[0][1])), qa
        for text, _ in list(got) + list(want):
            assert _no_repeat(text, 2) and len(text.split()) >= 6, (qa, text)       # (--min-length 6: no hypothesis ends before six tokens)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_sampling_under_a_repetition_penalty_is_repeatable(run, dtype, caplog):
    from mtn_amd import decode as D
    D._SESSIONS.clear()
    out = str(run["tmp"] / f"con_sample_{dtype}.json")
    smp = ["--temperature", "0.9", "--top-k", "20", "--top-p", "0.9", "--samples", "2", "--sample-seed", "5"]
    pen = ["--repetition-penalty", "1.3"]
    a, log_a = _main(caplog, _argv(run, "sample", dtype, out, smp + pen))
    b, log_b = _main(caplog, _argv(run, "sample", dtype, out, smp + pen))
    plain, log_plain = _main(caplog, _argv(run, "sample", dtype, out, smp))
    assert a == b and log_a == log_b
    assert log_a != log_plain                                             # the penalty reaches the draws
    assert all(len(h) == 2 and h[0][1] >= h[1][1] for h in log_a)
    if dtype == "fp32":
        c, log_c = _main(caplog, _argv(run, "sample", dtype, out, smp + pen + ["--dialogues-per-search", "1"]))
        assert [[h[0] for h in hyps] for hyps in log_c] == [[h[0] for h in hyps] for hyps in log_a]
        assert max(abs(x[1] - y[1]) for hc, ha in zip(log_c, log_a) for x, y in zip(hc, ha)) < 1e-3
