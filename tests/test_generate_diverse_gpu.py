"""`python generate.py --decode-style beam_search --beam 4 --beam-groups 2 --diversity-penalty 0.5` (mtn_amd.generate) on the GPU, end to
end, on the mini AVSD fixture and a one-epoch checkpoint (the `run` fixture of tests/test_generate_gpu.py, copied).  Every QA decoded inside
a bucketed, padded multi-QA search must give what the --no-buckets run (one QA per search at its own shape) gives — to the bars of
tests/test_generate_gpu.py: fp32 the same n-best hypotheses and scores within 1e-3; bf16 the same best hypothesis and its score within
1e-2 (relative, floor 1)."""
import json
import logging
import os
import re

import pytest
import torch

from tests.test_dataset_frontend import _features

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
BEAM, PENALTY, NBEST = 4, 1.0, 4
DIVERSE = ["--beam-groups", "2", "--diversity-penalty", "0.5"]


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """One epoch of training through mtn_amd.train.main (d_model 128: bf16 decodes on the persistent step) -> conf + checkpoint."""
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    from mtn_amd import train
    tmp = tmp_path_factory.mktemp("gen_diverse")
    raw = json.load(open(os.path.join(GOLD, "mini_avsd.json")))
    _, fea_path = _features(tmp, raw)
    prefix = str(tmp / "exp" / "mtn")
    train.main(["--fea-type", "i3d", "vgg", "--train-path", fea_path, "--train-set", os.path.join(GOLD, "mini_avsd.json"),
                "--num-epochs", "1", "--batch-size", "4", "--max-length", "256", "--model", prefix, "--include-caption", "caption,summary",
                "--separate-caption", "1", "--max-history-length", "3", "--nb-blocks", "1", "--d-model", "128", "--d-ff", "256",
                "--att-h", "4", "--dropout", "0.1", "--warmup-steps", "20", "--report-interval", "1000"])
    return dict(tmp=tmp, fea_path=fea_path, prefix=prefix, full=os.path.join(GOLD, "mini_avsd.json"))


def _argv(run, dtype, out, extra=()):
    return ["--gpu", "0", "--test-path", run["fea_path"], "--test-set", run["full"], "--model-conf", run["prefix"] + ".conf",
            "--model", run["prefix"] + "_1", "--beam", str(BEAM), "--penalty", str(PENALTY), "--nbest", str(NBEST), "--output", out,
            "--decode-style", "beam_search", "--undisclosed-only", "0", "--compute-dtype", dtype] + list(extra)


def _logged_hyps(records):
    """Per QA (log order): [(hypothesis string, score)]."""
    out = []
    for rec in records:
        msg = rec.getMessage()
        if re.fullmatch(r"\d+ \S+_\d+", msg):
            out.append([])
        elif re.fullmatch(r"HYP\[\d+\]: .*  \( \S+ \)", msg):
            m = re.fullmatch(r"HYP\[\d+\]: (.*)  \( (\S+) \)", msg)
            out[-1].append((m.group(1), float(m.group(2))))
    return out


def _main(caplog, argv):
    from mtn_amd import generate as G
    caplog.clear()
    caplog.set_level(logging.INFO)
    result = G.main(argv)
    return result, _logged_hyps(caplog.records)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_diverse_generate_equals_its_no_buckets_run(run, dtype, caplog, monkeypatch):
    from mtn_amd import decode as D
    seen = []
    real_many = D.beam_search_decode_many
    monkeypatch.setattr(D, "beam_search_decode_many", lambda *a, **k: seen.append((k.get("beam_groups"), k.get("diversity_penalty"))) or real_many(*a, **k))
    D._SESSIONS.clear()
    fallbacks = D.MegaDecodeSession.FALLBACKS
    out = str(run["tmp"] / f"div_{dtype}.json")
    result, logged = _main(caplog, _argv(run, dtype, out, DIVERSE))
    assert json.load(open(out)) == result
    assert seen and set(seen) == {(2, 0.5)}
    mega = [s[0] for s in D._SESSIONS.values() if isinstance(s[0], D.MegaDecodeSession)]
    n_multi = len(seen)
    single, logged1 = _main(caplog, _argv(run, dtype, out, DIVERSE + ["--no-buckets"]))
    if dtype == "bf16":
        assert mega and all(s._search_key[-2:] == (2, 0.5) for s in mega if getattr(s, "_search_key", None)), "bf16 at d_model 128 must decode on the persistent step"
        assert D.MegaDecodeSession.FALLBACKS == fallbacks
    n_qa = len(logged)
    assert n_qa == len(logged1) > 0 and len(seen) - n_multi == n_qa > n_multi          # one search per QA against several QAs per search
    plain, logged_plain = _main(caplog, _argv(run, dtype, out))
    assert logged_plain != logged                                                     # the groups reach the searches
    answers = [t["answer"] for d in result["dialogs"] for t in d["dialog"]]
    for qa in range(n_qa):
        got, want = logged[qa], logged1[qa]
        assert len(got) == len(want) == NBEST and answers[qa] == got[0][0]
        assert len({g[0] for g in got}) == NBEST, (qa, got)                            # no hypothesis twice
        if dtype == "fp32":
            assert [g[0] for g in got] == [w[0] for w in want], qa
            assert max(abs(g[1] - w[1]) for g, w in zip(got, want)) < 1e-3, qa
        else:
            assert got[0][0] == want[0][0], qa
            assert abs(got[0][1] - want[0][1]) < 1e-2 * max(1.0, abs(want[0][1])), qa
