#!/usr/bin/env python
"""What contrastive search costs (--decode-style contrastive; csrc/contrastive.hip), on tools/generate_bench.py's synthetic corpus and model
(run.sh's model, bf16, random weights, maxlen 30, penalty 1.0).

* Search cost: QA/s of contrastive search at K = 5 next to beam 5 on the same launch-per-sublayer pass (MTN_DECODE_MEGA=0): the same rows
  per pass and passes per token, but a host read per token that contrastive search does not have.  One warm-up pass each (it captures the
  graphs), then --runs passes each, alternated.
* Context, not judged: beam 5 and greedy on the persistent decode step.
* The kernel alone: mtn_contrastive_advance between events at l = 29, 8 dialogues x 5 rows, d = 512, next to mtn_topk_rows +
  mtn_beam_advance on as many rows (launch-bound).
* --parent DIR (a built checkout of the parent commit): existing paths did not move — `bench.py --gpus 1` and `tools/generate_bench.py
  --styles beam,greedy` (beam 5 and greedy QA/s) of DIR and of this tree, ALTERNATED in fresh processes, --runs each, medians and their
  ratio recorded (expected inside +-4 %).  Runs before this process touches the GPU.
Prints one JSON line and, with --out, writes it.

    python tools/contrastive_bench.py [--dialogs 1710] [--runs 3] [--parent ../parent] [--out profiles/contrastive_generate_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import pickle
import statistics
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def kernel_alone(dev, reps=200):
    """Microseconds per launch, median of `reps` event-timed launches after a warm-up."""
    import torch
    from mtn_amd import lib, ops
    D, K, Lm, d, V, l = 8, 5, 30, 512, 3004, 29
    W = D * K
    g = torch.Generator(device="cpu").manual_seed(1)
    hidden = torch.randn(W, Lm, d, generator=g).to(dev)
    logp = torch.log_softmax(torch.randn(W, V, generator=g), -1).to(dev)
    tokens = torch.randint(4, V, (W, Lm), generator=g).to(dev)
    pos, cand = torch.zeros(1, dtype=torch.long, device=dev), torch.full((W,), -1.0, device=dev)
    step, done = torch.zeros(D, dtype=torch.int32, device=dev), torch.zeros(D, dtype=torch.int32, device=dev)
    log = (torch.zeros(Lm, D, dtype=torch.int32, device=dev), torch.zeros(Lm, D, device=dev), torch.zeros(Lm, D, device=dev),
           torch.zeros(Lm, D, dtype=torch.int32, device=dev))
    top = ops.topk_rows(logp, K + 4, -1)
    a = ops.contrastive_args(hidden, top, tokens, pos, cand, step, done, log, k=K, alpha=0.6, eos=3, min_len=1, banned=(0, 1, 2))
    h = lib.load()
    # the beam search's pair on the same rows: heads of beam + 3 entries, bookkeeping of D dialogues of width 5
    b = lib.BeamArgs()
    b.dialogues, b.width, b.L, b.k_top, b.k, b.beam, b.unk, b.eos, b.pad, b.min_len, b.penalty = D, K, Lm, K + 3, K + 2, K, 0, 3, 1, 1, 1.0
    anc, lp = torch.arange(W, dtype=torch.int32, device=dev).repeat_interleave(Lm).view(W, Lm).contiguous(), torch.zeros(W, dtype=torch.float64, device=dev)
    n_live, bstep, flags = torch.full((D,), K, dtype=torch.int32, device=dev), torch.zeros(D, dtype=torch.int32, device=dev), torch.zeros(2, dtype=torch.int32, device=dev)
    btok, bpos = torch.zeros(W, dtype=torch.long, device=dev), torch.zeros(2, dtype=torch.int32, device=dev)
    li = lambda *s: torch.zeros(*s, dtype=torch.int32, device=dev)
    lf = lambda *s: torch.zeros(*s, dtype=torch.float64, device=dev)
    keep = [li(Lm, W), li(Lm, W), lf(Lm, W), lf(Lm, W), li(Lm, D), li(Lm, D)]
    b.tokens, b.pos, b.anc, b.lp, b.n_live, b.step, b.flags = (t.data_ptr() for t in (btok, bpos, anc, lp, n_live, bstep, flags))
    b.log_parent, b.log_tok, b.log_score, b.log_done, b.log_n_old, b.log_n_new = (t.data_ptr() for t in keep)

    def contrastive():
        step.fill_(l)
        done.zero_()
        return lambda: lib.check(h.mtn_contrastive_advance(C.byref(a), lib.stream_ptr()))

    def beam_pair():
        bstep.fill_(l - 1)
        n_live.fill_(K)

        def run():
            t = ops.topk_rows(logp, K + 3, 3)
            b.top = t.data_ptr()
            lib.check(h.mtn_beam_advance(C.byref(b), lib.stream_ptr()))
        return run

    def measure(setup):
        us = []
        for i in range(reps + 20):
            run = setup()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            run()
            e1.record()
            torch.cuda.synchronize()
            if i >= 20:
                us.append(e0.elapsed_time(e1) * 1e3)
        return round(statistics.median(us), 2)

    return {"shape": {"dialogues": D, "k": K, "L": Lm, "d": d, "l": l, "rows": W}, "contrastive_advance_us": measure(contrastive),
            "topk_rows_plus_beam_advance_us": measure(beam_pair), "note": "event-timed single launches: launch-bound"}


def _json_line(cmd, cwd, limit):
    """The last JSON line a fresh process prints (under a time limit; a failure ends the run)."""
    import subprocess
    env = {k: v for k, v in os.environ.items() if k not in ("MTN_HIP_LIB", "MTN_DECODE_MEGA", "PYTHONPATH")}
    p = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable] + cmd, cwd=cwd, env=env, capture_output=True, text=True)
    if p.returncode != 0:
        raise SystemExit("%s in %s ended with %d:\n%s" % (" ".join(cmd), cwd, p.returncode, p.stderr[-2000:]))
    print("done: %s in %s" % (" ".join(cmd), cwd), file=sys.stderr, flush=True)
    return json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])


def against_parent(parent, runs, dialogs):
    """bench.py and generate.py beam 5 / greedy of the parent checkout and of this tree, alternated in fresh processes (parent first)."""
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    trees = (("parent", os.path.abspath(parent)), ("this_tree", here))
    rec = {"bench_samples_per_s": {n: [] for n, _ in trees}, "beam5_qa_per_s": {n: [] for n, _ in trees}, "greedy_qa_per_s": {n: [] for n, _ in trees}}
    for _ in range(runs):
        for name, root in trees:
            rec["bench_samples_per_s"][name].append(_json_line(["bench.py", "--gpus", "1", "--steps", "30", "--warmup", "5"], root, 300)["value"])
    for _ in range(runs):
        for name, root in trees:
            g = _json_line(["tools/generate_bench.py", "--dialogs", str(dialogs), "--styles", "beam,greedy"], root, 600)
            rec["beam5_qa_per_s"][name].append(g["beam5_buckets_auto_d"]["qa_per_s"])
            rec["greedy_qa_per_s"][name].append(g["greedy_buckets_auto_d"]["qa_per_s"])
    for key in ("bench_samples_per_s", "beam5_qa_per_s", "greedy_qa_per_s"):
        mp, mt = statistics.median(rec[key]["parent"]), statistics.median(rec[key]["this_tree"])
        rec[key].update(median_parent=mp, median_this_tree=mt, this_tree_vs_parent_percent=round((mt / mp - 1) * 100, 2))
    rec["what"] = ("`bench.py --gpus 1 --steps 30 --warmup 5` and `tools/generate_bench.py --styles beam,greedy` (%d QAs, graph captures inside the "
                   "timed pass), both checkouts alternated in fresh processes, %d runs each" % (dialogs, runs))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, metavar="DIR", help="a built checkout of the parent commit: its bench.py and generate_bench.py run next to this tree's")
    ap.add_argument("--dialogs", type=int, default=1710)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--maxlen", type=int, default=30)
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--alpha", type=float, default=0.6)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    vs_parent = against_parent(a.parent, a.runs, a.dialogs) if a.parent else None
    if vs_parent is not None and a.out:                  # (kept even if the rest of the run does not finish)
        with open(a.out, "w") as f:
            f.write(json.dumps({"existing_paths_vs_parent": vs_parent}, indent=1) + "\n")
    import logging
    import torch
    from generate_bench import synth
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
        torch.manual_seed(1)
        sd = make_model(len(vocab), len(vocab), N=6, d_model=512, d_ff=2048, h=8, ft_sizes=ft, diff_encoder=True, auto_encoder_ft="query").state_dict()
        model = G.build_model(vocab, targs, ft, sd, "bf16", dev)
        corpus = dh.DeviceCorpus(data, dev)
        n = len(data["dialogs"])

        def timed(style, mega, **kw):
            os.environ["MTN_DECODE_MEGA"] = "1" if mega else "0"
            torch.cuda.synchronize()
            t0 = time.time()
            G.generate_response(model, data, corpus, vocab, maxlen=a.maxlen, beam=5, penalty=1.0, nbest=5, decode_style=style, undisclosed_only=True,
                                dialogues_per_search=G.LAUNCH_PASS_D if not mega else 0, **kw)
            torch.cuda.synchronize()
            return round(n / (time.time() - t0), 1)

        settings = {"contrastive%d_launch_path" % a.k: lambda: timed("contrastive", False, contrastive=dict(k=a.k, alpha=a.alpha)),
                    "beam5_launch_path": lambda: timed("beam_search", False),
                    "beam5_persistent_step": lambda: timed("beam_search", True),
                    "greedy_persistent_step": lambda: timed("greedy", True)}
        runs = {name: [] for name in settings}
        for name, fn in settings.items():                       # warm-up: every style captures its graphs
            fn()
        for _ in range(a.runs):
            for name, fn in settings.items():
                runs[name].append(fn())
                print("done: %s %.1f QA/s" % (name, runs[name][-1]), file=sys.stderr, flush=True)
        out = {"qas": n, "maxlen": a.maxlen, "k": a.k, "alpha": a.alpha, "dialogues_per_search_launch_path": G.LAUNCH_PASS_D, "runs": a.runs,
               "qa_per_s": runs, "median_qa_per_s": {name: statistics.median(v) for name, v in runs.items()}}
        m = out["median_qa_per_s"]
        out["contrastive_over_beam5_launch_path"] = round(m["contrastive%d_launch_path" % a.k] / m["beam5_launch_path"], 3)
        out["kernel_alone"] = kernel_alone(dev)
        if vs_parent is not None:
            out["existing_paths_vs_parent"] = vs_parent
        from mtn_amd.decode import MegaDecodeSession
        out["persistent_step_fallbacks"] = MegaDecodeSession.FALLBACKS
        out["note"] = "one box's numbers; random weights: nothing here says anything about response quality"
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
