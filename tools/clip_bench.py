#!/usr/bin/env python
"""What gradient clipping costs the training step: cfg2 (run.sh's model), batch 32, bf16, dropout 0.1, captured graphs, three steps in ONE
process — the plain (fused-optimiser) step, the fuse_optimizer=False step, the clipped step — timed in alternated passes, medians over
the passes.  The difference plain -> separate is what losing the optimiser epilogue costs (the gradient's HBM round trip), separate ->
clipped is the norm.  Then the two new launches on their own over the model's flat gradient buffer, between HIP events, and
mtn_grad_sumsq's achieved GB/s (4 n bytes read; the partials it writes are noise) against this box's own streaming-copy rate
(bench.py's hbm_peak_measured: mtn_measure_hbm_peak, 1 GiB read + 1 GiB written).

    python tools/clip_bench.py [--steps 30] [--warmup 5] [--passes 5] [--out profiles/clip_train_bench.json]
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
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--clip", type=float, default=1.0)
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

    steps = {}
    for name, kw in (("plain", {}), ("separate_optimizer", dict(fuse_optimizer=False)), ("clipped", dict(clip_grad_norm=args.clip))):
        torch.manual_seed(2)
        model = make_model(V, V, N=6, d_model=512, d_ff=2048, h=8, dropout=0.1, ft_sizes=fts, diff_encoder=True, auto_encoder_ft="query",
                           compute_dtype="bf16").to(dev).train()
        model.prepare()
        steps[name] = TrainStep(model, batch, V, pad=1, **kw)
        for _ in range(args.warmup):
            steps[name]()
    torch.cuda.synchronize()
    passes = {k: [] for k in steps}
    for _ in range(args.passes):
        for name, step in steps.items():
            passes[name].append(timed(step, args.steps))
    adam = steps["clipped"].opt.optimizer
    st = adam.clip_stats()
    rec = {"workload": "cfg2", "batch": args.batch, "dtype": "bf16", "steps": args.steps, "warmup": args.warmup, "passes": args.passes,
           "clip_grad_norm": args.clip,
           "ms_per_step": {k: round(statistics.median(v), 4) for k, v in passes.items()},
           "ms_per_step_passes": {k: [round(x, 4) for x in v] for k, v in passes.items()},
           "fused_optimizer": {k: bool(s._fused()) for k, s in steps.items()},
           "clip_stats": st}
    p = rec["ms_per_step"]
    rec["ms_losing_the_fusion"] = round(p["separate_optimizer"] - p["plain"], 4)
    rec["ms_the_norm"] = round(p["clipped"] - p["separate_optimizer"], 4)
    rec["ratio_to_plain"] = {k: round(p[k] / p["plain"], 4) for k in ("separate_optimizer", "clipped")}

    # the two launches alone over the model's flat gradient buffer (as the last step left it)
    lib = L.load()
    grad = steps["clipped"].model.flat_buffers()[2]
    n = grad.numel()
    npart = lib.mtn_grad_sumsq_partials(n)
    partial = torch.zeros(npart, device=dev, dtype=torch.float64)
    out = torch.zeros(1, device=dev, dtype=torch.float64)
    scale = torch.ones(1, device=dev)
    sp = L.stream_ptr()
    launches = {"grad_sumsq": lambda: L.check(lib.mtn_grad_sumsq(n, grad.data_ptr(), partial.data_ptr(), sp)),
                "clip_scale": lambda: L.check(lib.mtn_clip_scale(npart, partial.data_ptr(), args.clip, None, scale.data_ptr(), out.data_ptr(), None, sp))}
    for fn in launches.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    alone = {k: [] for k in launches}
    for _ in range(args.passes):
        for name, fn in launches.items():
            alone[name].append(timed(fn, args.steps) * 1e3)
    us = {k: round(statistics.median(v), 2) for k, v in alone.items()}
    peak = bench.hbm_peak_measured(dev)
    gbps = 4.0 * n / (us["grad_sumsq"] * 1e-6) / 1e9
    rec["launch_us"] = us
    rec["flat_gradient_floats"] = n
    rec["partials"] = npart
    rec["grad_sumsq"] = {"bytes_read": 4 * n, "achieved_GBps": round(gbps, 1), "peak_measured": peak,
                         "frac_of_measured_peak": round(gbps / peak, 4) if peak else None,
                         "what": "launch-to-launch time of back-to-back launches between HIP events (includes the launch gap); bytes = 4 n read; "
                                 "peak_measured = GB/s of this box's 16-byte-per-lane streaming copy (bytes read + written)"}
    print(json.dumps(rec))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
