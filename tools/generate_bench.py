#!/usr/bin/env python
"""QA/s of `python generate.py` (mtn_amd.generate) on a test-set-sized synthetic corpus: N undisclosed-only dialogues with the
text lengths of the DSTC7-AVSD test set (history of up to 3 earlier turns, caption + summary), vggish (128) and i3d_flow (2048)
features of 10-40 and 30-180 frames, run.sh's model (6 blocks, d_model 512, d_ff 2048, 8 heads; random weights), beam 5,
penalty 1.0, maxlen 30.  Settings: buckets with automatic D, --no-buckets (on the first --no-buckets-qas QAs: it
captures graphs per QA shape), greedy, and --decode-style sample (1 and 4 samples per QA, next to greedy).  Prints one JSON line.
--styles picks a subset (beam, greedy, no_buckets, sample).  --no-repeat-ngram / --repetition-penalty constrain every search of the run
(generate.py's flags of the same names; off by default).  --ensemble M decodes with M random-init copies of the model (seeds 1..M)
combined on the device (decode.Ensemble; --ensemble-mode prob|logprob) and records the dialogues per search auto_dialogues chose.
--beam sets the beam of the beam-search settings (default 5; their keys carry it), --beam-groups / --diversity-penalty make them diverse
beam searches (generate.py's flags of the same names; greedy and sample are not touched).  --mbr N / --mbr-weights add minimum-Bayes-risk
selection of order N to the beam-search and sample settings (generate.py's flags; greedy is not touched), --samples sets the draws per QA
of the multi-sample setting (default 4; its key carries it).  --evaluate scores every pass's answers on the device against a labelled copy
of the corpus (random last answers of the same lengths), as generate.py --evaluate does after decoding: the time of a pass then holds the
scoring, and the run records the six corpus values of its last pass.

    python tools/generate_bench.py [--dialogs 1710] [--no-buckets-qas 300]
"""
import argparse
import json
import os
import pickle
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def synth(root, n, seed=1):
    rs = np.random.RandomState(seed)
    words = ["w%d" % i for i in range(3000)]
    sent = lambda lo, hi: " ".join(words[i] for i in rs.randint(0, len(words), size=rs.randint(lo, hi + 1)))
    dialogs = []
    for v in range(n):
        turns = [{"question": sent(4, 14), "answer": sent(5, 16)} for _ in range(int(rs.randint(1, 11)))]
        turns[-1]["answer"] = "__UNDISCLOSED__"
        dialogs.append({"image_id": "v%05d" % v, "caption": sent(15, 35), "summary": sent(15, 40), "dialog": turns})
    for ft, F, lo, hi in (("vggish", 128, 10, 40), ("i3d_flow", 2048, 30, 180)):
        os.makedirs(os.path.join(root, ft))
        for d in dialogs:
            np.save(os.path.join(root, ft, d["image_id"] + ".npy"), rs.randn(rs.randint(lo, hi + 1), F).astype(np.float32))
    path = os.path.join(root, "test_set.json")
    json.dump({"dialogs": dialogs}, open(path, "w"))
    vocab = {"<unk>": 0, "<blank>": 1, "<sos>": 2, "<eos>": 3}
    for w in words:
        vocab[w] = len(vocab)
    return path, os.path.join(root, "<FeaType>", "<ImageID>.npy"), vocab


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dialogs", type=int, default=1710)
    ap.add_argument("--no-buckets-qas", type=int, default=300)
    ap.add_argument("--maxlen", type=int, default=30)
    ap.add_argument("--styles", default="beam,greedy,no_buckets,sample", help="comma-separated: beam, greedy, no_buckets, sample")
    ap.add_argument("--no-repeat-ngram", type=int, default=0)
    ap.add_argument("--repetition-penalty", type=float, default=1.0)
    ap.add_argument("--beam", type=int, default=5)
    ap.add_argument("--beam-groups", type=int, default=1)
    ap.add_argument("--diversity-penalty", type=float, default=0.0)
    ap.add_argument("--mbr", type=int, default=0)
    ap.add_argument("--mbr-weights", default="uniform", choices=["uniform", "score"])
    ap.add_argument("--samples", type=int, default=4)
    ap.add_argument("--evaluate", action="store_true", help="score every pass's answers (generate.py --evaluate) inside its time")
    ap.add_argument("--ensemble", type=int, default=1, help="members: this many random-init copies with different seeds (1 = a plain model)")
    ap.add_argument("--ensemble-mode", default="prob", choices=["prob", "logprob"])
    a = ap.parse_args()
    import logging
    import torch
    from mtn_amd import data_handler as dh
    from mtn_amd import generate as G
    from mtn_amd import lib, make_model
    logging.basicConfig(level=logging.WARNING)
    lib.load()
    dev = torch.device("cuda:0")
    with tempfile.TemporaryDirectory() as root:
        test_set, fea_path, vocab = synth(root, a.dialogs)
        targs = argparse.Namespace(fea_type=["vggish", "i3d_flow"], include_caption="caption,summary", separate_caption=1,
                                   max_history_length=3, merge_source=0, nb_blocks=6, d_model=512, d_ff=2048, att_h=8, dropout=0.2,
                                   separate_his_embed=0, separate_cap_embed=0, diff_encoder=1, diff_embed=0, diff_gen=0,
                                   auto_encoder_ft="query")
        with open(os.path.join(root, "mtn.conf"), "wb") as f:
            pickle.dump((vocab, targs), f, -1)
        vocab, targs = G.load_conf(os.path.join(root, "mtn.conf"))
        data = dh.load(targs.fea_type, fea_path, test_set, vocab, include_caption=targs.include_caption, separate_caption=True,
                       max_history_length=targs.max_history_length, merge_source=False, undisclosed_only=True)
        ft = dh.feature_shape(data)
        members = []
        for seed in range(1, a.ensemble + 1):
            torch.manual_seed(seed)
            sd = make_model(len(vocab), len(vocab), N=6, d_model=512, d_ff=2048, h=8, ft_sizes=ft, diff_encoder=True,
                            auto_encoder_ft="query").state_dict()
            members.append(G.build_model(vocab, targs, ft, sd, "bf16", dev))
        model = members[0]
        if a.ensemble > 1:
            from mtn_amd.decode import Ensemble
            model = Ensemble(members, mode=a.ensemble_mode)
        corpus = dh.DeviceCorpus(data, dev)
        labelled, scores = None, {}
        if a.evaluate:                                           # a labelled copy: every undisclosed last answer gets a random sentence
            rs = np.random.RandomState(7)
            labelled = json.loads(json.dumps(data["original"]))
            for d in labelled["dialogs"]:
                d["dialog"][-1]["answer"] = " ".join("w%d" % i for i in rs.randint(0, 3000, size=rs.randint(5, 17)))
        lens = G.qa_lengths(data)
        n = len(lens)
        out = {"qas": n, "buckets": len({G.bucket_key(l) for l in lens}), "maxlen": a.maxlen, "beam": a.beam,
               "beam_groups": a.beam_groups, "diversity_penalty": a.diversity_penalty, "mbr": a.mbr, "mbr_weights": a.mbr_weights if a.mbr else None,
               "no_repeat_ngram": a.no_repeat_ngram, "repetition_penalty": a.repetition_penalty, "ensemble": a.ensemble, "ensemble_mode": a.ensemble_mode if a.ensemble > 1 else None}
        per_search = lambda width: sorted({len(ids) for ids, _, _ in G.plan_searches(
            lens, lambda shape: G.auto_dialogues(model, dev, shape, a.maxlen, width))})
        out["dialogues_per_search"] = {"beam%d" % a.beam: per_search(a.beam), "greedy": per_search(1)}

        def timed(style, buckets, subset=None, sampling=None):
            d = data if subset is None else dict(data, dialogs=data["dialogs"][:subset],
                                                 original={"dialogs": data["original"]["dialogs"][:subset]})
            torch.cuda.synchronize()
            t0 = time.time()
            div = dict(beam_groups=a.beam_groups, diversity_penalty=a.diversity_penalty) if style == "beam_search" else {}
            if a.mbr and style in ("beam_search", "sample"):
                div.update(mbr=a.mbr, mbr_weights=a.mbr_weights)
            res = G.generate_response(model, d, corpus, vocab, maxlen=a.maxlen, beam=a.beam, penalty=1.0, nbest=5, decode_style=style,
                                undisclosed_only=True, buckets=buckets, sampling=sampling, no_repeat_ngram=a.no_repeat_ngram,
                                repetition_penalty=a.repetition_penalty, **div)
            if labelled is not None:
                scores.clear()
                scores.update(G.evaluate_result(res, labelled, last=True))
            torch.cuda.synchronize()
            dt = time.time() - t0
            return {"qas": len(d["dialogs"]), "seconds": round(dt, 2), "qa_per_s": round(len(d["dialogs"]) / dt, 1)}

        styles = set(a.styles.split(","))
        if "beam" in styles:
            out["beam%d_buckets_auto_d" % a.beam] = timed("beam_search", True)
        if "greedy" in styles:
            out["greedy_buckets_auto_d"] = timed("greedy", True)
        if "sample" in styles:
            # sampling next to greedy, twice each (the first pass of a style captures its graphs), then four samples per QA
            smp = dict(temperature=1.0, top_k=40, top_p=0.9, seed=1)
            timed("sample", True, sampling=dict(smp, samples=1))
            out["greedy_buckets_auto_d_again"] = timed("greedy", True)
            out["sample1_buckets_auto_d"] = timed("sample", True, sampling=dict(smp, samples=1))
            out["sample1_plain_buckets_auto_d"] = timed("sample", True, sampling=dict(samples=1))
            timed("sample", True, sampling=dict(smp, samples=a.samples))
            out["sample%d_buckets_auto_d" % a.samples] = timed("sample", True, sampling=dict(smp, samples=a.samples))
            out["sample_over_greedy"] = round(out["sample1_buckets_auto_d"]["qa_per_s"] / out["greedy_buckets_auto_d_again"]["qa_per_s"], 3)
        if "no_buckets" in styles:
            out["beam%d_no_buckets" % a.beam] = timed("beam_search", False, min(n, a.no_buckets_qas))
        from mtn_amd.decode import MegaDecodeSession
        out["persistent_step_fallbacks"] = MegaDecodeSession.FALLBACKS
        if a.evaluate:
            out["evaluate"] = dict(scores)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
