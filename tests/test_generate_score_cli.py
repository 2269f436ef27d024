"""--decode-style score at the command line, its candidate files and metric arithmetic, and mtn_score_rows at the ABI boundary (no GPU
needed)."""
import json
import math
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MINI = os.path.join(ROOT, "tests", "golden", "mini_avsd.json")


def test_parse_accepts_the_score_style_and_its_flag(capsys):
    from mtn_amd import generate as G
    a = G.parse(["--decode-style", "score", "--candidates", "c.json"])
    assert (a.decode_style, a.candidates) == ("score", "c.json")
    assert G.parse(["--decode-style", "score"]).candidates is None
    # the other styles are parsed as before, and still carry no candidates
    for style in ("greedy", "beam_search", "sample"):
        b = G.parse(["--decode-style", style])
        assert b.decode_style == style and b.candidates is None
    with pytest.raises(SystemExit) as e:
        G.parse(["--decode-style", "nucleus"])
    assert e.value.code == 2
    with pytest.raises(SystemExit):
        G.parse(["--decode-style", "greedy", "--candidates", "c.json"])
    assert "--candidates" in capsys.readouterr().err


@pytest.fixture(scope="module")
def mini():
    from mtn_amd import data_handler as dh
    raw = json.load(open(MINI))
    return raw, dh.get_vocabulary(MINI, include_caption="caption,summary")


def test_tokenize_answer_is_the_data_handlers(mini):
    from mtn_amd import data_handler as dh
    from mtn_amd import generate as G
    raw, vocab = mini
    text = raw["dialogs"][0]["dialog"][0]["answer"]
    assert G.tokenize_answer(text, vocab) == dh.words2ids(text, vocab)[1:-1].tolist()
    ids = G.tokenize_answer("kitchen zzz-never-seen .", vocab)
    assert ids == [vocab["kitchen"], vocab["<unk>"], vocab["."]]
    assert G.tokenize_answer("", vocab) == []


def test_load_candidates_entries_and_fallback(mini, tmp_path):
    from mtn_amd import generate as G
    raw, vocab = mini
    n_qa = sum(len(d["dialog"]) for d in raw["dialogs"])
    keys = G.qa_keys(raw, False)
    assert len(keys) == n_qa and keys[0][0] == "VID00_0" and keys[4][0] == "VID01_0" and keys[-1][0] == "VID06_0"
    spec = {"VID00_1": {"candidates": ["kitchen .", "qqq-unknown kitchen", ""], "gt_index": 1},
            "VID03_4": {"candidates": ["does ."]}}
    path = tmp_path / "c.json"
    json.dump(spec, open(path, "w"))
    for src in (spec, str(path)):
        c = G.load_candidates(src, raw, vocab)
        assert len(c) == n_qa and [q["key"] for q in c] == [k for k, _ in keys]
        one = c[1]
        assert one["texts"] == spec["VID00_1"]["candidates"] and one["gt_index"] == 1 and one["ranked"]
        assert one["tokens"] == [[vocab["kitchen"], vocab["."]], [vocab["<unk>"], vocab["kitchen"]], []]
        k34 = [k for k, _ in keys].index("VID03_4")
        assert c[k34]["gt_index"] is None and not c[k34]["ranked"] and c[k34]["texts"] == ["does ."]
        # a QA without an entry: its own answer, its ground truth, not ranked
        own = raw["dialogs"][0]["dialog"][0]["answer"]
        assert c[0]["texts"] == [own] and c[0]["gt_index"] == 0 and not c[0]["ranked"] and c[0]["tokens"] == [G.tokenize_answer(own, vocab)]
    # no file at all: every QA on its own answer
    c = G.load_candidates(None, raw, vocab)
    assert [q["texts"][0] for q in c] == [t["answer"] for d in raw["dialogs"] for t in d["dialog"]]
    # undisclosed-only: one QA per dialogue, keyed turn 0, the answer from the labelled set
    und = json.loads(json.dumps(raw))
    for d in und["dialogs"]:
        d["dialog"][-1]["answer"] = "__UNDISCLOSED__"
    c = G.load_candidates(None, und, vocab, undisclosed_only=True, ref_data=raw)
    assert [q["key"] for q in c] == ["%s_0" % d["image_id"] for d in raw["dialogs"]]
    assert [q["texts"][0] for q in c] == [d["dialog"][-1]["answer"] for d in raw["dialogs"]]
    assert G.load_candidates(None, und, vocab, undisclosed_only=True)[0]["texts"] == ["__UNDISCLOSED__"]


@pytest.mark.parametrize("entry", [{"candidates": ["a", "b"], "gt_index": 2}, {"candidates": ["a", "b"], "gt_index": -1},
                                   {"candidates": ["a"], "gt_index": "0"}, {"candidates": ["a"], "gt_index": True}, {"candidates": []},
                                   {"gt_index": 0}, {"candidates": ["a", 3]}])
def test_load_candidates_refuses_bad_entries(mini, entry):
    from mtn_amd import generate as G
    raw, vocab = mini
    with pytest.raises(ValueError):
        G.load_candidates({"VID02_1": entry}, raw, vocab)
    with pytest.raises(ValueError):
        G.load_candidates({"VID99_0": {"candidates": ["a"]}}, raw, vocab)


def test_score_metrics_on_hand_made_scores():
    from mtn_amd import generate as G
    q = lambda score, gt, ranked=True, logp=None, n=None: dict(score=score, logp=logp or score, n_tokens=n or [2] * len(score), gt_index=gt,
                                                               ranked=ranked)
    qas = [q([-1.0, -3.0, -2.0], 0),                      # rank 1
           q([-5.0, -1.0, -2.0, -4.0], 3),                # rank 3
           q([-2.0, -2.0, -2.0], 1),                      # a three-way tie: input order -> rank 2
           q([-2.0, -1.0, -1.5, -1.2, -1.1, -1.3, -2.0], 6),     # tied with candidate 0, five better -> rank 7
           q([-9.0], 0, ranked=False, n=[5]),             # an own answer: counts for the perplexity only
           q([-1.0, -2.0], None, ranked=False)]           # no ground truth: counts for nothing
    m = G.score_metrics(qas)
    assert m["ranks"] == [1, 3, 2, 7] and m["n_ranked"] == 4 and m["n_answers"] == 5
    assert m["mrr"] == pytest.approx((1 + 1 / 3 + 1 / 2 + 1 / 7) / 4, rel=1e-12)
    assert (m["r1"], m["r5"], m["r10"]) == (0.25, 0.75, 1.0) and m["mean_rank"] == 13 / 4
    assert m["n_tokens"] == 2 + 2 + 2 + 2 + 5
    assert m["perplexity"] == pytest.approx(math.exp(-(-1.0 - 4.0 - 2.0 - 2.0 - 9.0) / 13), rel=1e-12)
    # logp, not score, enters the perplexity
    m2 = G.score_metrics([q([0.0, 1.0], 1, logp=[-4.0, -6.0], n=[2, 3])])
    assert m2["perplexity"] == pytest.approx(math.exp(2.0), rel=1e-12) and m2["ranks"] == [1]
    none = G.score_metrics([q([-1.0], None, ranked=False)])
    assert none["perplexity"] is None and none["mrr"] is None and none["n_ranked"] == 0
    assert G.candidate_order([-2.0, -1.0, -2.0, -1.0]) == [1, 3, 0, 2]


def test_build_result_keeps_the_structure_and_adds_scores(mini):
    from mtn_amd import generate as G
    raw, _ = mini
    n_qa = sum(len(d["dialog"]) for d in raw["dialogs"])
    plain = G.build_result(raw, False, ["x"] * n_qa)
    scored = G.build_result(raw, False, ["x"] * n_qa, scores=[[dict(candidate="x", score=-1.0, logp=-1.0, n_tokens=1)]] * n_qa)
    assert all("scores" not in t for d in plain["dialogs"] for t in d["dialog"])
    for a, b in zip(plain["dialogs"], scored["dialogs"]):
        assert a["image_id"] == b["image_id"]
        for ta, tb in zip(a["dialog"], b["dialog"]):
            assert set(tb) == set(ta) | {"scores"} and {k: tb[k] for k in ta} == ta


def test_abi_declares_and_binds_the_scoring_kernel():
    import ctypes
    from mtn_amd import lib
    hdr = open(os.path.join(ROOT, "include", "mtn_hip.h")).read()
    m = re.search(r"\bint\s+mtn_score_rows\s*\(([^)]*)\)\s*;", hdr)
    assert m and re.match(r"\s*const\s+mtn_score_args\s*\*", m.group(1))
    n_args = len(re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(","))
    assert "mtn_score_rows" in lib.SYMBOLS and len(lib.SYMBOLS["mtn_score_rows"][1]) == n_args == 2
    assert lib.SYMBOLS["mtn_score_rows"][1][0]._type_ is lib.ScoreArgs
    # the ctypes mirror follows the C struct field by field
    body = re.search(r"typedef struct \{([^}]*)\} mtn_score_args;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip().lstrip("*").strip() for decl in body.split(";") if decl.strip()
             for n in re.sub(r"^\s*(const\s+)?\w+\s*\**", "", decl.strip()).split(",")]
    assert names == [f[0] for f in lib.ScoreArgs._fields_], names
    assert ctypes.sizeof(lib.ScoreArgs) % 8 == 0
    assert "score.hip" in __import__("mtn_amd.build", fromlist=["SOURCES"]).SOURCES
    assert os.path.exists(os.path.join(ROOT, "mtn_amd", "csrc", "score.hip"))


def test_score_args_struct_size_matches_c(tmp_path):
    import ctypes
    import subprocess
    from mtn_amd import lib
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mtn_hip.h"\nint main(){printf("%zu %zu %zu %zu\\n", sizeof(mtn_score_args),'
                   ' offsetof(mtn_score_args, ldz), offsetof(mtn_score_args, logits), offsetof(mtn_score_args, seq_len));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    sizes = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    S = lib.ScoreArgs
    assert sizes == [ctypes.sizeof(S), S.ldz.offset, S.logits.offset, S.seq_len.offset]


def test_decode_exposes_candidate_scoring():
    import inspect
    from mtn_amd import decode, mtn, ops
    sig = inspect.signature(decode.score_candidates)
    assert list(sig.parameters)[:6] == ["model", "batch", "candidates", "start", "eos", "pad"]
    for name, default in (("penalty", 0.0), ("max_len", None), ("width", None), ("use_graph", True)):
        assert sig.parameters[name].default == default and sig.parameters[name].kind is inspect.Parameter.KEYWORD_ONLY
    assert callable(ops.score_rows) and callable(decode.DecodeSession.score) and callable(decode.DecodeSession._pass_score)
    assert callable(mtn.Generator.logits)
