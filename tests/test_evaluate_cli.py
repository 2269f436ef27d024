"""evaluate.py (mtn_amd.evaluate) and `generate.py --evaluate` without a GPU: ops.eval_metrics is replaced by the Python definition
(tests/eval_refs.py) on host tensors, so everything above the kernel runs — tokenisation, the stopword file, pairing, --last, "answers"
lists, the printed lines and the refusals, and how the values reach generate's log and result JSON."""
import argparse
import json
import logging
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from mtn_amd import evaluate as E
from mtn_amd import generate as G
from tests import eval_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def definition(monkeypatch):
    """ops.eval_metrics := the definition; returns the list of (hyps, refs) it was called with."""
    from mtn_amd import ops
    calls = []

    def fake(hyp, hyp_len, ref, ref_len, n_ref, *, workspace=None, out=None, df_of_ref=False):
        hyps = [hyp[q, :int(hyp_len[q])].tolist() for q in range(hyp.size(0))]
        refs = [[ref[q, r, :int(ref_len[q, r])].tolist() for r in range(int(n_ref[q]))] for q in range(ref.size(0))]
        calls.append((hyps, refs))
        ev = R.evaluate(hyps, refs)
        t = torch.from_numpy
        return t(ev["stats"]), t(ev["rouge"]), t(ev["cider"]), t(ev["corpus"]), None

    monkeypatch.setattr(ops, "eval_metrics", fake)
    return calls


# ---------------------------------------------------------------------------------------------------------------- text to ids
def test_tokenize_lowers_splits_and_drops_punctuation_tokens():
    assert E.tokenize("A Man  walks ,  then STOPS .") == ["a", "man", "walks", "then", "stops"]
    assert E.tokenize("yes , he does . -LRB- twice -RRB- ; -- ... ? ! : - ' '' ` ``") == ["yes", "he", "does", "twice"]
    assert E.tokenize("-lcb- x -RCB-") == ["x"]
    # only whole tokens are punctuation: there is no PTB splitting
    assert E.tokenize("yes, he doesn't.") == ["yes,", "he", "doesn't."]
    assert E.tokenize("") == [] and E.tokenize(" . ") == []
    assert len(E.PUNCTUATIONS) == 17


def test_stopword_file_three_line_forms(tmp_path):
    f = tmp_path / "stop.txt"
    f.write_text("a\nth.*\tTHE\nuh+\n\nthree words here\ncats? animal\ncat never\n")
    sw = E.StopwordFilter(str(f))
    assert len(sw.pats) == 5                                                   # the empty and the three-column line are ignored
    assert sw(["a", "cat", "and", "cats", "uhhh", "there", "aa", "catsx"]) == ["animal", "and", "animal", "THE", "aa", "catsx"]
    # anchored to the whole word ("a" does not touch "and"); the first matching line wins ("cat never" is never reached)
    assert E.tokenize("A man , uh , sees the cat", sw) == ["man", "sees", "THE", "animal"]
    assert E.tokenize("a uh", sw) == []


def test_ids_come_from_the_words_that_occur():
    pairs = [("v_0", "a <unk> walks", ["a man walks", "the man"]), ("v_1", "Zebra", ["zebra !"])]
    hyps, refs = E.to_ids(pairs)
    assert hyps == [[0, 1, 2], [5]] and refs == [[[0, 3, 2], [4, 3]], [[5]]]
    with pytest.raises(SystemExit, match="v_1"):
        E.to_ids([("v_0", "a", ["a"]), ("v_1", " ".join(["w"] * 129), ["a"])])


# ---------------------------------------------------------------------------------------------------------------- pairing
def _files(tmp_path, result, reference):
    rp, fp = tmp_path / "result.json", tmp_path / "reference.json"
    json.dump(result, open(rp, "w"))
    json.dump(reference, open(fp, "w"))
    return str(rp), str(fp)


REFERENCE = {"dialogs": [
    {"image_id": "vidB", "dialog": [{"question": "q", "answer": "a man walks ."}, {"question": "q", "answer": "he is cooking"}]},
    {"image_id": "vidA", "dialog": [{"question": "q", "answer": "unused", "answers": ["Two dogs run", "two dogs are running"]},
                                    {"question": "q", "answers": ["yes"]}, {"question": "q", "answer": "no , he sits"}]}]}
RESULT = {"dialogs": [                                                          # another dialogue order than the reference's
    {"image_id": "vidA", "dialog": [{"question": "q", "answer": "two dogs run"}, {"question": "q", "answer": "yes"},
                                    {"question": "q", "answer": "no he stands"}]},
    {"image_id": "vidB", "dialog": [{"question": "q", "answer": "a man walks"}, {"question": "q", "answer": "he is eating"}]}]}


def test_pairing_by_image_id_and_turn():
    pairs = E.pair(RESULT, REFERENCE)
    assert [p[0] for p in pairs] == ["vidA_0", "vidA_1", "vidA_2", "vidB_0", "vidB_1"]
    assert pairs[0][1:] == ("two dogs run", ["Two dogs run", "two dogs are running"])          # "answers" wins over "answer"
    assert pairs[1][2] == ["yes"] and pairs[3][1:] == ("a man walks", ["a man walks ."])
    last = E.pair(RESULT, REFERENCE, last=True)
    assert [(p[0], p[1], p[2]) for p in last] == [("vidA (last turn)", "no he stands", ["no , he sits"]), ("vidB (last turn)", "he is eating", ["he is cooking"])]
    # an undisclosed-only result holds one turn per dialogue: with --last it meets the reference's last turn
    und = {"dialogs": [{"image_id": d["image_id"], "dialog": d["dialog"][-1:]} for d in RESULT["dialogs"]]}
    assert E.pair(und, REFERENCE, last=True) == last


def test_main_prints_the_six_lines(tmp_path, definition, capsys):
    rp, fp = _files(tmp_path, RESULT, REFERENCE)
    out = tmp_path / "per_qa.json"
    res = E.main([rp, fp, "--per-qa", str(out)])
    hyps, refs = definition[-1]
    assert len(hyps) == 5 and [len(r) for r in refs] == [2, 1, 1, 1, 1]
    want = R.evaluate(hyps, refs)
    lines = capsys.readouterr().out.splitlines()
    assert lines == ["%s: %.3f" % (k, v) for k, v in zip(["Bleu_1", "Bleu_2", "Bleu_3", "Bleu_4", "ROUGE_L", "CIDEr"], want["corpus"][:6])]
    assert hyps[3] == refs[3][0]                                               # "a man walks" == "a man walks ." without its full stop
    assert res["Bleu_1"] == want["corpus"][0] and res["hyp_len"] == 13
    per = json.load(open(out))
    assert [i["id"] for i in per["items"]] == ["vidA_0", "vidA_1", "vidA_2", "vidB_0", "vidB_1"] and per["n_items"] == 5
    assert per["items"][3]["ROUGE_L"] == 1.0 and per["items"][0]["match_1"] == 3 and per["CIDEr"] == want["corpus"][5]
    # --last scores two items, and other numbers
    E.main([rp, fp, "--last"])
    assert len(definition[-1][0]) == 2
    assert capsys.readouterr().out.splitlines()[0] == "Bleu_1: %.3f" % R.evaluate(*definition[-1])["corpus"][0]


def test_run_sh_summary_reads_the_output(tmp_path, definition, capsys):
    rp, fp = _files(tmp_path, RESULT, REFERENCE)
    E.main([rp, fp])
    text = capsys.readouterr().out
    awk = subprocess.run(["awk", '/^(Bleu_[1-4]|METEOR|ROUGE_L|CIDEr):/{print $0; if($1=="CIDEr:"){exit}}'], input=text, capture_output=True, text=True)
    assert awk.stdout == text and len(text.splitlines()) == 6


def test_stopwords_reach_both_sides(tmp_path, definition, capsys):
    rp, fp = _files(tmp_path, RESULT, REFERENCE)
    sw = tmp_path / "stop.txt"
    sw.write_text("he\nis\ncooking eating\n")
    E.main([rp, fp, "--last", "--stopwords", str(sw)])
    hyps, refs = definition[-1]
    assert hyps[1] == refs[1][0] and len(hyps[1]) == 1                         # "he is eating" / "he is cooking" -> "eating" on both sides


def test_refusals(tmp_path, definition):
    bad = json.loads(json.dumps(RESULT))
    bad["dialogs"][1]["dialog"].append({"question": "q", "answer": "extra"})
    with pytest.raises(SystemExit, match="vidB_2"):                            # the first result turn without a reference
        E.main(list(_files(tmp_path, bad, REFERENCE)))
    bad = json.loads(json.dumps(RESULT))
    bad["dialogs"][0]["image_id"] = "vidC"
    with pytest.raises(SystemExit, match="vidC_0"):
        E.main(list(_files(tmp_path, bad, REFERENCE)))
    many = json.loads(json.dumps(REFERENCE))
    many["dialogs"][1]["dialog"][1]["answers"] = ["yes"] * 9
    with pytest.raises(SystemExit, match="vidA_1.*9 answers"):
        E.main(list(_files(tmp_path, RESULT, many)))
    none = json.loads(json.dumps(REFERENCE))
    del none["dialogs"][0]["dialog"][0]["answer"]
    with pytest.raises(SystemExit, match="vidB_0"):
        E.main(list(_files(tmp_path, RESULT, none)))
    with pytest.raises(SystemExit, match="no turn"):
        E.main(list(_files(tmp_path, {"dialogs": []}, REFERENCE)))
    with pytest.raises(SystemExit):                                            # argparse: the two files are required
        E.parse(["only_one.json"])


def test_root_shim_is_the_module():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "evaluate.py"), "--help"], capture_output=True, text=True, cwd=ROOT)
    assert out.returncode == 0 and "--last" in out.stdout and "--stopwords" in out.stdout and "--per-qa" in out.stdout


def test_evaluate_responses_checks_before_anything_runs(definition):
    from mtn_amd import decode as D
    with pytest.raises(ValueError, match="item 1"):
        D.evaluate_responses([[1], [2] * 129], [[[1]], [[2]]])
    with pytest.raises(ValueError, match="item 2"):
        D.evaluate_responses([[1], [2], [3]], [[[1]], [[2]], [[3]] * 9])
    with pytest.raises(ValueError, match="item 0"):
        D.evaluate_responses([[1]], [[]])
    with pytest.raises(ValueError):
        D.evaluate_responses([[1]], [[[1]], [[2]]])
    with pytest.raises(ValueError):
        D.evaluate_responses([], [])
    assert not definition
    res = D.evaluate_responses([[5, 6], []], [[[5, 6], [5]], [[7]]], device="cpu")
    assert definition == [([[5, 6], []], [[[5, 6], [5]], [[7]]])] and res["stats"].shape == (2, 10) and res["ref_len"] == 3


def test_the_operator_itself_runs_on_the_gpu_only():
    from mtn_amd import lib, ops
    z = lambda *s: torch.zeros(*s, dtype=torch.int32)
    with pytest.raises(lib.MtnHipError):
        ops.eval_metrics(z(2, 4), z(2), z(2, 1, 4), z(2, 1), z(2))


# ---------------------------------------------------------------------------------------------------------------- generate.py --evaluate
def test_generate_parser():
    a = G.parse([])
    assert a.evaluate is False and a.stopwords == ""
    assert G.parse(["--evaluate"]).evaluate is True
    a = G.parse(["--evaluate", "--stopwords", "s.txt", "--decode-style", "beam_search"])
    assert a.evaluate and a.stopwords == "s.txt"
    a = G.parse(["--evaluate", "--undisclosed-only", "1", "--labeled-test", "lbl.json", "--decode-style", "sample"])
    assert a.evaluate and a.undisclosed_only and a.labeled_test == "lbl.json"
    assert G.parse(["--undisclosed-only", "1", "--labeled-test"]).labeled_test is None        # run.sh's bare flag still parses without --evaluate


@pytest.mark.parametrize("argv", [
    ["--evaluate", "--decode-style", "score"],
    ["--evaluate", "--undisclosed-only", "1"],
    ["--evaluate", "--undisclosed-only", "1", "--labeled-test"],
    ["--evaluate", "--undisclosed-only", "1", "--labeled-test", ""],
    ["--stopwords", "s.txt"],
    ["--stopwords", "s.txt", "--decode-style", "beam_search"],
])
def test_generate_parser_refuses(argv, capsys):
    with pytest.raises(SystemExit) as e:
        G.parse(argv)
    assert e.value.code == 2 and "--evaluate" in capsys.readouterr().err


def _ns(**kw):
    return argparse.Namespace(**dict(dict(evaluate=False, stopwords="", undisclosed_only=False, output=""), **kw))


def test_generate_values_reach_the_log_and_the_json(tmp_path, definition, caplog):
    caplog.set_level(logging.INFO)
    out = tmp_path / "result.json"
    result = json.loads(json.dumps(RESULT))
    got = G.write_result(_ns(evaluate=True, output=str(out)), result, REFERENCE)
    hyps, refs = definition[-1]
    want = R.evaluate(hyps, refs)
    lines = ["%s: %.3f" % (k, v) for k, v in zip(R.NAMES, want["corpus"][:6])]
    msgs = [r.getMessage() for r in caplog.records]
    i = msgs.index(lines[0])
    assert msgs[i:i + 6] == lines and msgs[i + 6] == "writing results to " + str(out)
    written = json.load(open(out))
    assert written == got and written["dialogs"] == RESULT["dialogs"]
    assert written["eval"] == dict({k: float(v) for k, v in zip(R.NAMES, want["corpus"][:6])}, hyp_len=13, ref_len=int(want["corpus"][7]), n_items=5)
    # undisclosed-only: the labelled file's last answers
    und = {"dialogs": [{"image_id": d["image_id"], "dialog": [dict(d["dialog"][-1])]} for d in RESULT["dialogs"]]}
    own = json.loads(json.dumps(und))
    for d in own["dialogs"]:
        d["dialog"][0]["answer"] = "__UNDISCLOSED__"
    got = G.write_result(_ns(evaluate=True, undisclosed_only=True), json.loads(json.dumps(und)), own, REFERENCE)
    hyps, refs = definition[-1]
    assert len(hyps) == 2 and got["eval"]["n_items"] == 2 and got["eval"]["ROUGE_L"] == R.evaluate(hyps, refs)["corpus"][4]
    assert E.to_ids(E.pair(und, REFERENCE, last=True)) == (hyps, refs)


def test_generate_json_is_unchanged_without_the_flag(tmp_path, definition, caplog):
    caplog.set_level(logging.INFO)
    out = tmp_path / "result.json"
    result = json.loads(json.dumps(RESULT))
    G.write_result(_ns(output=str(out)), result, REFERENCE)
    assert open(out).read() == json.dumps(RESULT, indent=4)                   # the bytes generate.py wrote before it had the flag
    assert [r.getMessage() for r in caplog.records] == ["writing results to " + str(out)] and not definition
    assert "eval" not in result
