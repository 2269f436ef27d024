"""mtn_amd.generate without a GPU: run.sh's stage-3 command line, the bucket planner, detokenisation, the result JSON's shape,
conf loading and the refusal of pickled modules."""
import argparse
import json
import os
import pickle

import numpy as np
import pytest
import torch

from mtn_amd import generate as G

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def test_run_sh_stage3_command_line_parses():
    """run.sh:156-168 with its default variable values (beam 5, penalty 1.0, nbest 5, beam_search, labeled_test='' -> a bare
    --labeled-test at the end of the line)."""
    argv = ["--gpu", "0", "--test-path", "data/features/<FeaType>_testset/<ImageID>.npy", "--test-set", "data/test_set.json",
            "--model-conf", "exps/x/mtn.conf", "--model", "exps/x/mtn_best", "--beam", "5", "--penalty", "1.0", "--nbest", "5",
            "--output", "exps/x/result_test_set_b5_p1.0_beam_search_undisclosed1.json", "--decode-style", "beam_search",
            "--undisclosed-only", "1", "--labeled-test"]
    a = G.parse(argv)
    assert (a.beam, a.penalty, a.nbest, a.decode_style, a.undisclosed_only, a.labeled_test) == (5, 1.0, 5, "beam_search", True, None)
    assert a.model == "exps/x/mtn_best" and a.maxlen == 30 and a.compute_dtype == "bf16"
    assert a.dialogues_per_search == 0 and not a.no_buckets
    d = G.parse([])                                   # the reference's defaults (generate.py:91-115)
    assert (d.maxlen, d.beam, d.penalty, d.nbest, d.decode_style, d.undisclosed_only, d.labeled_test) == (30, 3, 2.0, 5, "greedy", False, None)
    assert G.parse(["--labeled-test", "lbl.json", "--no-buckets", "--compute-dtype", "fp32"]).labeled_test == "lbl.json"


def _lens(n, seed=0):
    rs = np.random.RandomState(seed)
    return [((int(rs.randint(1, 200)), int(rs.randint(1, 45))), int(rs.choice([1, rs.randint(1, 160)])), int(rs.randint(3, 45)), int(rs.randint(2, 40)),
             int(rs.randint(20, 240))) for _ in range(n)]


@pytest.mark.parametrize("per", [3, 16, lambda shape: 2 if shape[1] > 64 else 5])
def test_planner_places_every_qa_once_and_pads_buckets(per):
    lens = _lens(500)
    searches = G.plan_searches(lens, per)
    real = [i for ids, n, _ in searches for i in ids[:n]]
    assert sorted(real) == list(range(len(lens)))                      # every qa_id exactly once
    by_shape = {}
    for ids, n, shape in searches:
        x, h, q, a, c = shape
        assert 1 <= n <= len(ids) and len(set(ids[:n])) == n
        assert all(i == ids[n - 1] for i in ids[n:])                    # padding: copies of the last real QA
        for i in ids:
            lx, lh, lq, la, lc = lens[i]
            assert all(b >= t for b, t in zip(x, lx)) and h >= lh and q >= lq and a >= la and c >= lc
            assert G.bucket_key(lens[i]) == (tuple(x), h, q, c)
            assert (h == 1) == (lh == 1)                                # a first turn's lone <blank> history is never padded
        by_shape.setdefault((tuple(x), h, q, a, c), set()).add(len(ids))
    assert all(len(ds) == 1 for ds in by_shape.values())               # one D per bucket
    # buckets come one after another (the session cache sees each shape once)
    order = [(tuple(s[2][0]),) + tuple(s[2][1:]) for s in searches]
    assert len({k for k in order}) == sum(1 for i, k in enumerate(order) if i == 0 or k != order[i - 1])
    if per == 3:
        assert sum(len(ids) - n for ids, n, _ in searches) > 0          # some bucket is not a multiple of D


def test_planner_drops_padding_copies_from_results():
    """decode_searches keeps the first n_real results of a search only: the padded copies never reach an answer."""
    lens = _lens(11, seed=4)
    searches = G.plan_searches(lens, 4)
    got = {}
    for ids, n, _ in searches:
        fake = [("qa%d" % i, k) for k, i in enumerate(ids)]            # what a search returns, one entry per row
        for i, r in zip(ids[:n], fake[:n]):
            assert i not in got
            got[i] = r
    assert sorted(got) == list(range(11)) and all(r[0] == "qa%d" % i for i, r in got.items())


def test_no_buckets_is_one_qa_per_search_at_its_own_lengths():
    lens = _lens(20, seed=2)
    searches = G.plan_searches(lens, 7, buckets=False)
    assert [s[0] for s in searches] == [[i] for i in range(20)]
    for (ids, n, (x, h, q, a, c)), l in zip(searches, lens):
        assert n == 1 and (tuple(x), h, q, a, c) == l


def test_detokenise_stops_at_eos_and_greedy_drops_sos():
    vocab = {"<unk>": 0, "<blank>": 1, "<sos>": 2, "<eos>": 3, "a": 4, "man": 5, "walks": 6}
    vl = sorted(vocab, key=vocab.get)
    assert G.detokenize([4, 5, 6, 3, 5, 5], vl, 3) == "a man walks"
    assert G.detokenize([3, 4], vl, 3) == ""
    assert G.detokenize([4, 5], vl, 3) == "a man"
    assert G.greedy_text([2, 4, 6, 3, 1, 1], vl, 3) == "a walks"
    assert G.greedy_text([2, 2, 4], vl, 3) == "<sos> a"           # only the leading <sos> goes (generate.py:71)


def _undisclosed(raw):
    u = json.loads(json.dumps(raw))
    for d in u["dialogs"]:
        d["dialog"][-1]["answer"] = "__UNDISCLOSED__"
    return u


@pytest.mark.parametrize("undisclosed", [False, True])
def test_result_json_has_the_reference_shape(tmp_path, undisclosed):
    raw = json.load(open(os.path.join(GOLD, "mini_avsd.json")))
    if undisclosed:
        raw = _undisclosed(raw)
    n_qa = sum(1 if undisclosed else len(d["dialog"]) for d in raw["dialogs"])
    answers = ["hyp %d" % i for i in range(n_qa)]
    res = G.build_result(raw, undisclosed, answers)
    assert list(res) == ["dialogs"] and len(res["dialogs"]) == len(raw["dialogs"])
    qa = 0
    for got, want in zip(res["dialogs"], raw["dialogs"]):
        assert list(got) == ["image_id", "dialog"] and got["image_id"] == want["image_id"]
        turns = want["dialog"][-1:] if undisclosed else want["dialog"]
        assert len(got["dialog"]) == len(turns)
        for g, w in zip(got["dialog"], turns):
            assert list(g) == list(w) and g["question"] == w["question"] and g["answer"] == answers[qa]
            qa += 1
    assert raw["dialogs"][0]["dialog"][-1]["answer"] != answers[0]   # the input is not modified
    p = tmp_path / "r.json"
    json.dump(res, open(p, "w"), indent=4)
    assert json.load(open(p)) == res


def test_reference_style_conf_without_newer_fields_loads(tmp_path):
    """A conf as the reference's train.py pickles it: (vocab, Namespace) with the reference's fields only."""
    ns = argparse.Namespace(gpu=0, fea_type=["vggish", "i3d_flow"], train_path="", train_set="t.json", valid_path="", valid_set="",
                            include_caption="caption,summary", separate_caption=True, model="exps/mtn", nb_blocks=2, d_model=128,
                            d_ff=256, att_h=4, dropout=0.2, num_epochs=1, rand_seed=1, batch_size=32, max_length=256)
    vocab = {"<unk>": 0, "<blank>": 1, "<sos>": 2, "<eos>": 3, "a": 4}
    p = tmp_path / "mtn.conf"
    with open(p, "wb") as f:
        pickle.dump((vocab, ns), f, -1)
    v, a = G.load_conf(str(p))
    assert v == vocab and a.nb_blocks == 2 and a.d_model == 128 and a.include_caption == "caption,summary"
    assert a.max_history_length == -1 and a.merge_source == 0 and a.diff_encoder == 0 and a.diff_embed == 0 and a.diff_gen == 0
    assert a.separate_his_embed == 0 and a.separate_cap_embed == 0 and a.auto_encoder_ft is None
    from mtn_amd import make_model
    m = make_model(len(v), len(v), N=a.nb_blocks, d_model=a.d_model, d_ff=a.d_ff, h=a.att_h, dropout=a.dropout, ft_sizes=[8, 4],
                   diff_encoder=bool(a.diff_encoder), auto_encoder_ft="query", compute_dtype="fp32")
    torch.save(m.state_dict(), tmp_path / "mtn_1.pth.tar")
    sd = G.load_state_dict(str(tmp_path / "mtn_1.pth.tar"))
    assert set(sd) == set(m.state_dict())


def test_pickled_module_is_refused_with_the_recipe(tmp_path):
    p = str(tmp_path / "mtn_best.pth.tar")
    torch.save(torch.nn.Sequential(torch.nn.Linear(4, 4)), p)        # what the reference's train.py writes: a whole module
    with pytest.raises(SystemExit) as e:
        G.load_state_dict(p)
    msg = str(e.value)
    assert "pickled nn.Module" in msg and "state_dict()" in msg and p in msg
