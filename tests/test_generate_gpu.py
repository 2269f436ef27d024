"""`python generate.py` (mtn_amd.generate) on the GPU, end to end: a checkpoint trained for one epoch on the mini annotation file
(tests/golden/mini_avsd.json, features synthesised as in test_dataset_frontend.py), then generate.main for beam search and greedy,
fp32 and bf16, every turn and undisclosed-only.  Every QA decoded inside a bucketed, padded multi-QA search must give what a
search over that QA alone, at its own unpadded shape, gives (and on a few QAs what the CPU oracle gives)."""
import json
import logging
import os
import re
import subprocess
import sys

import pytest
import torch

from tests.test_dataset_frontend import _features

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
BEAM, PENALTY, NBEST, MAXLEN = 5, 1.0, 5, 30              # run.sh:48-50; generate.py's --maxlen default


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """One epoch of training through mtn_amd.train.main (d_model 128: bf16 decodes on the persistent step) -> conf + checkpoint;
    the mini test set and an undisclosed-only variant of it."""
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    from mtn_amd import train
    tmp = tmp_path_factory.mktemp("gen")
    raw = json.load(open(os.path.join(GOLD, "mini_avsd.json")))
    _, fea_path = _features(tmp, raw)
    prefix = str(tmp / "exp" / "mtn")
    train.main(["--fea-type", "i3d", "vgg", "--train-path", fea_path, "--train-set", os.path.join(GOLD, "mini_avsd.json"),
                "--num-epochs", "1", "--batch-size", "4", "--max-length", "256", "--model", prefix, "--include-caption", "caption,summary",
                "--separate-caption", "1", "--max-history-length", "3", "--nb-blocks", "1", "--d-model", "128", "--d-ff", "256",
                "--att-h", "4", "--dropout", "0.1", "--warmup-steps", "20", "--report-interval", "1000"])
    und = json.loads(json.dumps(raw))
    for d in und["dialogs"]:
        d["dialog"][-1]["answer"] = "__UNDISCLOSED__"
    und_path = tmp / "undisclosed.json"
    json.dump(und, open(und_path, "w"))
    return dict(tmp=tmp, fea_path=fea_path, prefix=prefix, full=os.path.join(GOLD, "mini_avsd.json"), und=str(und_path))


def _argv(run, style, dtype, undisclosed, out):
    return ["--gpu", "0", "--test-path", run["fea_path"], "--test-set", run["und"] if undisclosed else run["full"],
            "--model-conf", run["prefix"] + ".conf", "--model", run["prefix"] + "_1", "--beam", str(BEAM), "--penalty", str(PENALTY),
            "--nbest", str(NBEST), "--output", out, "--decode-style", style, "--undisclosed-only", str(int(undisclosed)),
            "--compute-dtype", dtype] + (["--labeled-test", run["full"]] if undisclosed else [])


def _logged_hyps(records):
    """Per QA (log order): beam -> [(hypothesis string, score)], greedy -> hypothesis string."""
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


def _reference_side(run, dtype, undisclosed):
    """The conf's model in the given compute dtype, the test data and its device corpus, as generate loads them."""
    from mtn_amd import data_handler as dh
    from mtn_amd import generate as G
    vocab, targs = G.load_conf(run["prefix"] + ".conf")
    data = dh.load(targs.fea_type, run["fea_path"], run["und"] if undisclosed else run["full"], vocab, include_caption=targs.include_caption,
                   separate_caption=bool(targs.separate_caption), max_history_length=targs.max_history_length,
                   merge_source=bool(targs.merge_source), undisclosed_only=undisclosed)
    sd = G.load_state_dict(run["prefix"] + "_1.pth.tar")
    dev = torch.device("cuda:0")
    model = G.build_model(vocab, targs, dh.feature_shape(data), sd, dtype, dev)
    return vocab, targs, data, dh.DeviceCorpus(data, dev), model, sd


@pytest.mark.parametrize("undisclosed", [0, 1], ids=["all-turns", "undisclosed"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("style", ["beam_search", "greedy"])
def test_generate_equals_per_qa_decode(run, style, dtype, undisclosed, caplog, monkeypatch):
    from mtn_amd import data_handler as dh
    from mtn_amd import decode as D
    from mtn_amd import generate as G
    out = str(run["tmp"] / f"result_{style}_{dtype}_{undisclosed}.json")
    D._SESSIONS.clear()
    fallbacks = D.MegaDecodeSession.FALLBACKS
    caplog.set_level(logging.INFO)
    result = G.main(_argv(run, style, dtype, undisclosed, out))
    mega_used = any(isinstance(s[0], D.MegaDecodeSession) for s in D._SESSIONS.values())
    logged = _logged_hyps(caplog.records)
    assert json.load(open(out)) == result

    vocab, targs, data, corpus, model, sd = _reference_side(run, dtype, bool(undisclosed))
    n_qa = len(data["dialogs"])
    assert len(logged) == n_qa and "wall time" in caplog.text and "QA/s" in caplog.text
    answers = [t["answer"] for d in result["dialogs"] for t in d["dialog"]]
    raw = json.load(open(run["und"] if undisclosed else run["full"]))
    assert [d["image_id"] for d in result["dialogs"]] == [d["image_id"] for d in raw["dialogs"]]
    assert len(answers) == n_qa and all(len(d["dialog"]) == 1 for d in result["dialogs"]) == bool(undisclosed)

    if undisclosed:
        # 7 QAs: whatever the buckets, some search of D = 3 (bf16 beam 5), 8 (fp32) or 16 (greedy) holds padding copies
        width = BEAM if style == "beam_search" else 1
        searches = G.plan_searches(G.qa_lengths(data), lambda shape: G.auto_dialogues(model, corpus.device, shape, MAXLEN, width))
        assert any(len(ids) > n for ids, n, _ in searches)

    if dtype == "bf16":
        assert mega_used, "bf16 at d_model 128 must decode on the persistent step"
        assert D.MegaDecodeSession.FALLBACKS == fallbacks
    vl = sorted(vocab, key=vocab.get)
    sos, eos, unk, pad = vocab["<sos>"], vocab["<eos>"], vocab["<unk>"], vocab["<blank>"]
    idx, _ = dh.make_batch_indices(data, 1, separate_caption=True)         # one QA per entry, its own lengths (no bucket padding)
    ties = []
    real_search = D.MegaDecodeSession.search

    def spy(self, *a, **k):
        r = real_search(self, *a, **k)
        ties.append(r is None)
        return r

    monkeypatch.setattr(D.MegaDecodeSession, "search", spy)
    singles = []
    for qa in range(n_qa):
        ix = idx[qa]
        assert ix[1] == [qa]
        b = dh.make_batch(corpus, ix, vocab, separate_caption=True)
        ties.clear()
        if style == "beam_search":
            nb, _ = D.beam_search_decode(model, b, MAXLEN, sos, unk, eos, pad, beam=BEAM, penalty=PENALTY, nbest=NBEST)
            singles.append(nb)
            got = logged[qa]
            want = [(G.detokenize(t, vl, eos), s) for t, s in nb[:NBEST]]
            if dtype == "fp32":
                assert [g[0] for g in got] == [w[0] for w in want], qa
                assert max(abs(g[1] - w[1]) for g, w in zip(got, want)) < 1e-3, qa
            else:
                if not any(ties):
                    assert got[0][0] == want[0][0], qa
                assert abs(got[0][1] - want[0][1]) < 1e-2 * max(1.0, abs(want[0][1])), qa
            assert answers[qa] == got[0][0]
        else:
            ys = D.greedy_decode(model, b, MAXLEN, sos, pad)[0].tolist()
            singles.append(ys)
            assert logged[qa] == G.greedy_text(ys, vl, eos) == answers[qa], qa

    if dtype == "fp32":
        # on three QAs, the CPU oracle on the oracle's own batch
        from oracle import batch_oracle, mtn_oracle as orc
        from oracle.mtn_oracle import OracleBatch, OracleConfig, OracleMTN
        cfg = OracleConfig(vocab=len(vocab), n_layers=targs.nb_blocks, d_model=targs.d_model, d_ff=targs.d_ff, heads=targs.att_h,
                           ft_sizes=tuple(dh.feature_shape(data)), diff_encoder=bool(targs.diff_encoder), diff_embed=bool(targs.diff_embed),
                           diff_gen=bool(targs.diff_gen), auto_encoder_ft=targs.auto_encoder_ft)
        m_or = OracleMTN(cfg, {k: v.float() for k, v in sd.items()})
        for qa in range(min(3, n_qa)):
            r = batch_oracle.assemble(data, idx[qa], pad, True)
            t = torch.from_numpy
            ob = OracleBatch(query=t(r["query"]), his=t(r["his"]), cap=t(r["cap"]), trg=t(r["trg"]), trg_y=t(r["trg_y"]),
                             fts=[t(f) for f in r["fts_padded_with_ones"]], pad=pad)
            with torch.no_grad():
                if style == "beam_search":
                    ref_n, _ = orc.beam_search(m_or, ob, MAXLEN, sos, unk, eos, beam=BEAM, penalty=PENALTY, nbest=NBEST)
                    assert [list(x) for x, _ in singles[qa]] == [list(x) for x, _ in ref_n], qa
                    assert max(abs(a[1] - b[1]) for a, b in zip(singles[qa], ref_n)) < 1e-3, qa
                else:
                    assert orc.greedy_search(m_or, ob, MAXLEN, sos) == singles[qa], qa


def test_greedy_decode_many_equals_one_by_one(run):
    """greedy_decode_many on a Batch of D QAs (bf16, persistent step): row d is greedy_decode of QA d."""
    from mtn_amd import data_handler as dh
    from mtn_amd import decode as D
    vocab, _, data, corpus, model, _ = _reference_side(run, "bf16", False)
    idx, _ = dh.make_batch_indices(data, 1, separate_caption=True)
    ids = [0, 3, 7, 11, 12]
    lens = [idx[i] for i in ids]
    many_ix = ([data["dialogs"][i][0] for i in ids], ids, [max(l[2][f] for l in lens) for f in range(len(lens[0][2]))],
               max(l[3] for l in lens), max(l[4] for l in lens), max(l[5] for l in lens), max(l[6] for l in lens), len(ids))
    D._SESSIONS.clear()
    many = D.greedy_decode_many(model, dh.make_batch(corpus, many_ix, vocab, separate_caption=True), 16, vocab["<sos>"], vocab["<blank>"])
    assert any(isinstance(s[0], D.MegaDecodeSession) for s in D._SESSIONS.values())
    assert many.shape == (len(ids), 16)
    for r, i in enumerate(ids):
        one = D.greedy_decode(model, dh.make_batch(corpus, idx[i], vocab, separate_caption=True), 16, vocab["<sos>"], vocab["<blank>"])
        assert many[r].tolist() == one[0].tolist(), i


def test_generate_py_subprocess_writes_the_json(run):
    """`python generate.py ...` from the repository root, as run.sh stage 3 calls it (under a time limit)."""
    out = str(run["tmp"] / "result_cli.json")
    argv = _argv(run, "beam_search", "bf16", 1, out)
    p = subprocess.run(["timeout", "-k", "10", "600", sys.executable, "generate.py"] + argv, cwd=ROOT, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    res = json.load(open(out))
    assert list(res) == ["dialogs"] and len(res["dialogs"]) == 7 and all(len(d["dialog"]) == 1 for d in res["dialogs"])
    assert all(d["dialog"][0]["answer"] != "__UNDISCLOSED__" for d in res["dialogs"])
    assert "wall time" in p.stderr and "QA/s" in p.stderr
