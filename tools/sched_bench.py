#!/usr/bin/env python
"""What scheduled sampling costs: cfg2 (run.sh's model), batch 32, bf16, dropout 0.1, in one process.

  * the captured step four ways, alternated, median of --passes passes of --steps steps: plain; with one same-size distillation teacher
    (the yardstick: the same eval() forward and generator GEMM, a dearer tail); with scheduled sampling at p = 0.25 and at p = 1.
    Expectation that is checked and recorded (not a test): the scheduled-sampling step takes no longer than the one-teacher step of
    the same process times 1.05 — the 5 % margin is just above the +-4 % run-to-run noise the README records;
  * the mix kernel alone over the step's 640 rows (B = 32, T = 20, V = 3000) at p = 0.25 and p = 1, arg-max and Gumbel-max: median of 5
    passes between HIP events on the launch stream.  Reported, not judged: it is launch-bound and there is nothing to time it against;
  * --parent-bench PATH/bench.py: this tree's bench.py (the flag-off step) and another checkout's, ALTERNATED in fresh processes,
    --ab-runs runs each; the medians are expected inside +-4 %.  The other checkout must be built.

    python tools/sched_bench.py [--steps 30] [--warmup 5] [--passes 5] [--parent-bench ../parent/bench.py] [--out profiles/sched_train_bench.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
V, FTS = 3000, [2048, 128]                                     # cfg2: run.sh's model, bench.py's flagship shapes
MARGIN = 1.05


def make(dev):
    from mtn_amd import make_model
    return make_model(V, V, N=6, d_model=512, d_ff=2048, h=8, dropout=0.1, ft_sizes=FTS, diff_encoder=True, auto_encoder_ft="query",
                      compute_dtype="bf16").to(dev)


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


def median_of_5(launch):
    """ms of one launch: median of 5 passes, each between its own pair of HIP events on the launch stream"""
    launch()
    torch.cuda.synchronize()
    ms = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        launch()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), ms


def last_json(text):
    for ln in reversed(text.strip().splitlines()):
        if ln.startswith("{"):
            return json.loads(ln)
    return None


def bench_ms(bench_py, steps, warmup):
    out = subprocess.run([sys.executable, bench_py, "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)], cwd=os.path.dirname(bench_py),
                         capture_output=True, text=True, timeout=300)
    rec = last_json(out.stdout)
    if rec is None:
        raise RuntimeError("no result line from %s: %s" % (bench_py, (out.stderr or out.stdout)[-400:]))
    print("%s: %.4f ms/step" % (bench_py, rec["ms_per_step"]), file=sys.stderr, flush=True)
    return rec["ms_per_step"]


def kernel_alone(dev, batch, rows_T):
    """The mix launch over logits of the step's shape: random Gaussian rows, the gold inputs of the step's batch."""
    from mtn_amd import ops
    B, T = rows_T
    z = torch.randn(B * T, V, device=dev)
    trg = batch.trg.contiguous()
    keys = torch.arange(B, dtype=torch.int64, device=dev)
    state = torch.tensor([100.0, 0, 0, 0, 0, 0, 0, 0], device=dev)
    out, stats = torch.empty_like(trg), torch.zeros(3, dtype=torch.int64, device=dev)
    rec = {}
    for pick in ("argmax", "sample"):
        for p in (0.25, 1.0):
            ms, all_ms = median_of_5(lambda: ops.sched_mix(z, trg, keys, state, pad=1, prob=p, pick=pick, banned=(2,), out=out, stats=stats))
            rec["%s_p%g" % (pick, p)] = {"ms": round(ms, 4), "ms_passes": [round(x, 4) for x in all_ms]}
    rec["rows"], rec["V"] = B * T, V
    rec["what"] = ("one mtn_sched_mix launch between HIP events (launch included), %d workgroups of 256 threads over (%d, %d) fp32 logits; "
                   "reported, not judged: it is launch-bound" % (B * T, B * T, V))
    return rec


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--parent-bench", default=None, metavar="PATH", help="bench.py of a built checkout of the parent commit")
    ap.add_argument("--ab-runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    rec = {"workload": "cfg2", "batch": args.batch, "dtype": "bf16", "steps": args.steps, "warmup": args.warmup, "passes": args.passes}
    # fresh processes first: nothing of this process is on the GPU yet
    if args.parent_bench:
        ours = os.path.join(ROOT, "bench.py")
        ab = {"parent": [], "this_tree_flag_off": []}
        for _ in range(args.ab_runs):
            ab["parent"].append(bench_ms(os.path.abspath(args.parent_bench), args.steps, args.warmup))
            ab["this_tree_flag_off"].append(bench_ms(ours, args.steps, args.warmup))
        mp, mt = statistics.median(ab["parent"]), statistics.median(ab["this_tree_flag_off"])
        ab.update(median_parent=mp, median_this_tree=mt, this_tree_vs_parent_percent=round((mt / mp - 1) * 100, 2),
                  inside_4_percent=bool(abs(mt / mp - 1) <= 0.04),
                  what="ms per step of `bench.py --gpus 1`, both checkouts alternated in fresh processes (order inside a pass: parent, this tree)")
        rec["flag_off_vs_parent"] = ab

    from mtn_amd.synthetic import synthetic_batch
    from mtn_amd.train_step import SchedConfig, TrainStep
    dev = torch.device("cuda:0")
    batch = synthetic_batch(V, args.batch, 20, 128, 40, 20, [32, 32], FTS, device=dev, seed=1)
    torch.manual_seed(3)
    teacher = make(dev).eval()
    for q in teacher.parameters():
        q.requires_grad_(False)
    variants = (("plain", {}), ("one_teacher", dict(teacher=teacher, distill_alpha=0.5)), ("sched_p0.25", dict(sched=SchedConfig(0.25))),
                ("sched_p1", dict(sched=SchedConfig(1.0))))
    steps = {}
    for key, kw in variants:
        torch.manual_seed(2)
        model = make(dev).train()
        model.prepare()
        steps[key] = TrainStep(model, batch, V, pad=1, **kw)
    ms = {k: [] for k, _ in variants}
    for _ in range(args.passes):                                 # alternated: plain, teacher, p 0.25, p 1, plain, ...
        for key, _ in variants:
            ms[key].append(round(timed(steps[key], args.steps, args.warmup), 4))
    med = {k: statistics.median(v) for k, v in ms.items()}
    rec["ms_per_step"] = {"passes": ms, "median": med,
                          "first_pass_cost_ms": {k: round(med[k] - med["plain"], 4) for k in med if k != "plain"},
                          "sched_vs_one_teacher": {k: round(med[k] / med["one_teacher"], 4) for k in ("sched_p0.25", "sched_p1")},
                          "expectation": "sched <= one_teacher x %.2f" % MARGIN,
                          "expectation_met": {k: bool(med[k] <= med["one_teacher"] * MARGIN) for k in ("sched_p0.25", "sched_p1")}}
    st = steps["sched_p0.25"].sched_stats.tolist()
    rec["counters_p0.25"] = {"eligible": st[0], "replaced": st[1], "differ_from_gold": st[2], "replaced_fraction": round(st[1] / max(1, st[0]), 4)}
    rec["mix_kernel"] = kernel_alone(dev, batch, tuple(batch.trg.shape))
    print(json.dumps(rec))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
