#!/usr/bin/env python
"""ms/step of the knowledge-distilled training step next to the plain one: cfg2 (run.sh's model), batch 32, bf16, dropout 0.1, captured
graphs — no teacher, a same-size single teacher, a two-member ensemble teacher.  The expectation it confirms or refutes: a distilled
step costs one eval() forward per teacher member plus a small head (the distillation form of csrc/losshead.hip in the place of the plain one).

    python tools/distill_bench.py [--steps 30] [--warmup 5] [--out profiles/distill_train_bench.json]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    from mtn_amd import make_model
    from mtn_amd.decode import Ensemble
    from mtn_amd.synthetic import synthetic_batch
    from mtn_amd.train_step import TrainStep, teacher_rows
    dev = torch.device("cuda:0")
    V, fts = 3000, [2048, 128]                                     # cfg2: run.sh's model, bench.py's flagship shapes
    mk = lambda: make_model(V, V, N=6, d_model=512, d_ff=2048, h=8, dropout=0.1, ft_sizes=fts, diff_encoder=True, auto_encoder_ft="query",
                            compute_dtype="bf16").to(dev)
    batch = synthetic_batch(V, args.batch, 20, 128, 40, 20, [32, 32], fts, device=dev, seed=1)

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.steps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.steps

    torch.manual_seed(1)
    teachers = [mk().eval() for _ in range(2)]
    for t in teachers:
        t.prepare()
    rec = {"workload": "cfg2", "batch": args.batch, "dtype": "bf16", "steps": args.steps, "warmup": args.warmup, "ms_per_step": {}}
    for name, teacher in (("plain", None), ("one_teacher", teachers[0]), ("two_member_ensemble", Ensemble(teachers, [2.0, 1.0], "prob"))):
        torch.manual_seed(2)
        model = mk().train()
        model.prepare()
        step = TrainStep(model, batch, V, pad=1, teacher=teacher, distill_alpha=0.5, distill_temperature=2.0)
        rec["ms_per_step"][name] = round(timed(step), 4)
        if teacher is not None:
            rec.setdefault("kd_per_token", {})[name] = round(float(step.last_kd), 5)
        del step, model
    rec["teacher_pass_ms"] = {"one_teacher": round(timed(lambda: teacher_rows(teachers[0], batch)), 4)}      # eager: launch-bound upper bound
    p = rec["ms_per_step"]
    rec["ratio_to_plain"] = {k: round(v / p["plain"], 3) for k, v in p.items()}
    print(json.dumps(rec))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
