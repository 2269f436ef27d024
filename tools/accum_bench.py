#!/usr/bin/env python
"""What gradient accumulation costs: cfg2 (run.sh's model), batch 32, bf16, dropout 0.1, on one GPU.

  1. mtn_grad_accum's three modes alone over the model's flat gradient buffer, back to back between HIP events, median of the passes:
     GB/s (8 B per element for FIRST, 12 B for ADD and LAST) and the fraction of this box's own streaming-copy rate (bench.py's
     hbm_peak_measured), next to mtn_ema_step over the same n in the same process (the same traffic shape: two streams read, one written);
     LAST with clipping's partials against LAST followed by a separate mtn_grad_sumsq.
  2. Captured steps in ONE process, alternated passes, medians: the plain (fused-optimiser) step, the fuse_optimizer=False step, and
     windows of K = 2 and K = 4 micro-steps on the same batch, as ms per window and ms per micro-batch.

    python tools/accum_bench.py [--steps 30] [--warmup 5] [--passes 5] [--out profiles/accum_train_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30, help="optimiser updates per pass")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--windows", type=int, nargs="+", default=[2, 4])
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    import bench
    from mtn_amd import lib as L
    from mtn_amd import make_model
    from mtn_amd.synthetic import synthetic_batch
    from mtn_amd.train_step import TrainStep
    dev = torch.device("cuda:0")
    V, fts = 3000, [2048, 128]                                     # cfg2: run.sh's model, bench.py's flagship shapes
    batch = synthetic_batch(V, args.batch, 20, 128, 40, 20, [32, 32], fts, device=dev, seed=1)

    def timed(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n

    def window(step, K):
        def run():
            for k in range(K):
                step(k == K - 1)
        return run

    steps, runs = {}, {}
    variants = [("plain", {}, 1), ("separate_optimizer", dict(fuse_optimizer=False), 1)] + [("window_%d" % K, dict(accumulate=True), K) for K in args.windows]
    for name, kw, K in variants:
        torch.manual_seed(2)
        model = make_model(V, V, N=6, d_model=512, d_ff=2048, h=8, dropout=0.1, ft_sizes=fts, diff_encoder=True, auto_encoder_ft="query",
                           compute_dtype="bf16").to(dev).train()
        model.prepare()
        steps[name] = TrainStep(model, batch, V, pad=1, **kw)
        runs[name] = steps[name] if K == 1 else window(steps[name], K)
        for _ in range(args.warmup):
            runs[name]()
    torch.cuda.synchronize()
    passes = {k: [] for k in runs}
    for _ in range(args.passes):
        for name, fn in runs.items():
            passes[name].append(timed(fn, args.steps))
    rec = {"workload": "cfg2", "batch": args.batch, "dtype": "bf16", "updates_per_pass": args.steps, "warmup": args.warmup, "passes": args.passes,
           "ms_per_update": {k: round(statistics.median(v), 4) for k, v in passes.items()},
           "ms_per_update_passes": {k: [round(x, 4) for x in v] for k, v in passes.items()},
           "fused_optimizer": {k: bool(s._fused()) for k, s in steps.items()}}
    p = rec["ms_per_update"]
    rec["ms_per_micro_batch"] = {"window_%d" % K: round(p["window_%d" % K] / K, 4) for K in args.windows}
    rec["micro_batch_ratio_to_plain"] = {k: round(v / p["plain"], 4) for k, v in rec["ms_per_micro_batch"].items()}

    # the launches alone over the model's flat gradient buffer (as the last step left it)
    lib = L.load()
    first = steps["window_%d" % args.windows[0]]
    grad, acc = first.model.flat_buffers()[2], first.opt.optimizer.accum
    flat = first.model.flat_buffers()[0]
    ema = flat.clone()
    state = first.opt.optimizer.state
    n = grad.numel()
    npart = lib.mtn_grad_sumsq_partials(n)
    partial = torch.zeros(npart, device=dev, dtype=torch.float64)
    w = torch.ones(1, device=dev)
    tot = torch.ones(2, device=dev)
    sp = L.stream_ptr()
    g, a, wp, t0, t1 = grad.data_ptr(), acc.data_ptr(), w.data_ptr(), tot.data_ptr(), tot.data_ptr() + 4

    def last_then_sumsq():
        L.check(lib.mtn_grad_accum(L.MTN_ACCUM_LAST, n, a, g, wp, t0, t1, None, sp))
        L.check(lib.mtn_grad_sumsq(n, g, partial.data_ptr(), sp))

    launches = {"first": (lambda: L.check(lib.mtn_grad_accum(L.MTN_ACCUM_FIRST, n, a, g, wp, None, t1, None, sp)), 8),
                "add": (lambda: L.check(lib.mtn_grad_accum(L.MTN_ACCUM_ADD, n, a, g, wp, t0, t1, None, sp)), 12),
                "last": (lambda: L.check(lib.mtn_grad_accum(L.MTN_ACCUM_LAST, n, a, g, wp, t0, t1, None, sp)), 12),
                "last_with_partials": (lambda: L.check(lib.mtn_grad_accum(L.MTN_ACCUM_LAST, n, a, g, wp, t0, t1, partial.data_ptr(), sp)), 12),
                "last_then_grad_sumsq": (last_then_sumsq, 16),
                "ema_step": (lambda: L.check(lib.mtn_ema_step(n, ema.data_ptr(), flat.data_ptr(), state.data_ptr(), 0.999, None, sp)), 12)}
    for fn, _ in launches.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    alone = {k: [] for k in launches}
    for _ in range(args.passes):
        for name, (fn, _) in launches.items():
            alone[name].append(timed(fn, args.steps) * 1e3)
    us = {k: round(statistics.median(v), 2) for k, v in alone.items()}
    peak = bench.hbm_peak_measured(dev)
    rec["flat_gradient_floats"] = n
    rec["launch_us"] = us
    rec["launch_us_passes"] = {k: [round(x, 2) for x in v] for k, v in alone.items()}
    rec["peak_measured"] = peak
    rec["launches"] = {}
    for name, (_, bpe) in launches.items():
        gbps = bpe * n / (us[name] * 1e-6) / 1e9
        rec["launches"][name] = {"bytes_per_element": bpe, "achieved_GBps": round(gbps, 1),
                                 "frac_of_measured_peak": round(gbps / peak, 4) if peak else None,
                                 "time_over_ema_step": round(us[name] / us["ema_step"], 4)}
    rec["what"] = ("launch-to-launch time of back-to-back launches between HIP events (includes the launch gap); peak_measured = GB/s of "
                   "this box's 16-byte-per-lane streaming copy (bytes read + written); the bar for add and last is 1.10 x ema_step's time")
    rec["within_1.10x_of_ema_step"] = {k: bool(us[k] <= 1.10 * us["ema_step"]) for k in ("add", "last")}
    print(json.dumps(rec))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
