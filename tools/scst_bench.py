#!/usr/bin/env python
"""ms per self-critical training step next to the plain captured step of the same process: cfg2 (run.sh's model), batch 32, bf16, dropout
0.1, S = 2 and S = 4 samples per dialogue on a synthetic corpus; the split of an RL step between the sampling search, the assemble /
reward / advantage launches (with the replication into the static batch) and the captured step; and the mean reward of the greedy
responses on a fixed held-out slice before and after --rl-steps RL steps from one seed.  Nobody has judged these numbers in advance.

    python tools/scst_bench.py [--steps 20] [--warmup 3] [--rl-steps 200] [--out profiles/scst_train_bench.json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rl-steps", type=int, default=200)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--samples", type=int, nargs="+", default=[2, 4])
    ap.add_argument("--max-length", type=int, default=20)
    ap.add_argument("--videos", type=int, default=24)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    from mtn_amd import decode, make_model
    from mtn_amd.data_handler import DeviceCorpus, make_batch, make_batch_indices
    from mtn_amd.train import synthetic_corpus
    from mtn_amd.train_step import BucketedTrainer, ScstConfig, TrainStep, corpus_reference
    dev = torch.device("cuda:0")
    V, fts, T = 3000, [2048, 128], args.max_length                   # cfg2: run.sh's model, bench.py's flagship sizes
    mk = lambda: make_model(V, V, N=6, d_model=512, d_ff=2048, h=8, dropout=0.1, ft_sizes=fts, diff_encoder=True, auto_encoder_ft="query",
                            compute_dtype="bf16").to(dev)
    data = synthetic_corpus(args.videos, V, fts, 1)
    corpus = DeviceCorpus(data, dev)
    indices, _ = make_batch_indices(data, batchsize=args.batch, max_length=256, separate_caption=True)
    full = [ix for ix in indices if ix[-1] == args.batch]
    held, train_ix = full[:2], full[2:]                               # a fixed held-out slice of two batches; the rest is trained on
    refs = corpus_reference(corpus, min_len=T)

    def timed(fn, steps, warmup):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / steps

    rec = {"workload": "cfg2", "batch": args.batch, "dtype": "bf16", "max_length": T, "steps": args.steps, "warmup": args.warmup,
           "rl_steps": args.rl_steps, "reward": "cider", "baseline": "mean", "plain_ms_per_step": None, "scst": {}}
    torch.manual_seed(2)
    model = mk().train()
    model.prepare()
    plain = TrainStep(model, make_batch(corpus, train_ix[0], 1, separate_caption=True), V, pad=1)
    rec["plain_ms_per_step"] = round(timed(plain, args.steps, args.warmup), 4)
    del plain, model

    for S in args.samples:
        torch.manual_seed(2)
        model = mk().train()
        model.prepare()
        cfg = ScstConfig(samples=S, max_length=T, refs=refs, seed=1)
        trainer = BucketedTrainer(model, corpus, V, pad=1, scst=cfg)

        def held_reward():
            """Mean CIDEr of the greedy responses on the held-out slice, through the step's own assemble and reward launches."""
            tot, n = 0.0, 0
            model.eval()
            with torch.no_grad():
                for ix in held:
                    b = make_batch(corpus, ix, 1, separate_caption=True)
                    ys = decode.greedy_decode_many(model, b, T, 2, 1)
                    log = torch.cat([ys[:, 1:].to(torch.int32), torch.full((ys.size(0), 1), 3, dtype=torch.int32, device=dev)], 1).t().contiguous()
                    any_step = next(iter(trainer.steps.values()))[1]
                    r = any_step._rewards(log, torch.tensor(list(ix[1]), dtype=torch.int32, device=dev))
                    tot, n = tot + float(r.sum()), n + r.numel()
            model.train()
            return tot / max(1, n)

        k = 0

        def one(timings=None):
            nonlocal k
            ix = train_ix[k % len(train_ix)]
            k += 1
            if timings is None:
                return trainer.step(ix)
            hit = trainer.steps[trainer._key(ix)]
            make_batch(corpus, trainer._padded(ix), 1, separate_caption=True, out=hit[0])
            return hit[1].rl_step(list(ix[1]), seed=cfg.seed + k, timings=timings)

        for ix in train_ix:                                           # every shape built and captured before anything is timed
            trainer.step(ix)
        torch.cuda.synchronize()
        before = held_reward()
        ms = timed(one, args.steps, args.warmup)
        split = {}
        for _ in range(args.steps):
            one(split)
        done = len(train_ix) + args.warmup + 2 * args.steps
        rewards = []
        for j in range(max(0, args.rl_steps - done)):
            one()
            if (j + 1) % 20 == 0:
                rewards.append(round(float(trainer.last_reward), 5))
        after = held_reward()
        sess = [type(v[0]).__name__ for v in decode._SESSIONS.values()]
        rec["scst"]["S%d" % S] = {
            "ms_per_rl_step": round(ms, 4), "ratio_to_plain": round(ms / rec["plain_ms_per_step"], 3),
            "split_ms_synchronised": {n: round(v / args.steps, 4) for n, v in split.items()},
            "search_pass": "launch-per-sublayer (B*S = %d rows; the persistent step takes at most 16)" % (args.batch * S),
            "decode_sessions": sorted(set(sess)), "shapes": len(trainer.steps),
            "held_out_greedy_cider": {"before": round(before, 5), "after_%d_rl_steps" % max(done, args.rl_steps): round(after, 5)},
            "train_mean_reward_every_20_steps": rewards}
        del trainer, model
        decode._SESSIONS.clear()
    print(json.dumps(rec))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
