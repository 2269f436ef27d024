#!/usr/bin/env python
"""ms/step of the training step with unlikelihood training next to the plain one: cfg2 (run.sh's model), batch 32, bf16, dropout 0.1,
captured graphs, both steps in ONE process, timed in alternated passes, medians over the passes.  Then the two head launches on their
own, on the step's shapes (the response stream with its sequence length, the auto-encoder stream without), between HIP events: the plain
pair and the unlikelihood pair.  The expectation it confirms or refutes: unlikelihood costs one more pass over at most T gathered logits
per row, small next to the 12 KB the row already streams.

    python tools/unlikelihood_bench.py [--steps 30] [--warmup 5] [--passes 5] [--out profiles/unlikelihood_train_bench.json]
"""
import argparse
import ctypes as C
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
    ap.add_argument("--alpha", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
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
    for name, alpha in (("plain", 0.0), ("unlikelihood", args.alpha)):
        torch.manual_seed(2)
        model = make_model(V, V, N=6, d_model=512, d_ff=2048, h=8, dropout=0.1, ft_sizes=fts, diff_encoder=True, auto_encoder_ft="query",
                           compute_dtype="bf16").to(dev).train()
        model.prepare()
        steps[name] = TrainStep(model, batch, V, pad=1, unlikelihood=alpha)
        for _ in range(args.warmup):
            steps[name]()
    torch.cuda.synchronize()
    passes = {k: [] for k in steps}
    for _ in range(args.passes):
        for name, step in steps.items():
            passes[name].append(timed(step, args.steps))
    rec = {"workload": "cfg2", "batch": args.batch, "dtype": "bf16", "steps": args.steps, "warmup": args.warmup, "passes": args.passes,
           "ul_alpha": args.alpha,
           "ms_per_step": {k: round(statistics.median(v), 4) for k, v in passes.items()},
           "ms_per_step_passes": {k: [round(x, 4) for x in v] for k, v in passes.items()},
           "ul_per_token": round(float(steps["unlikelihood"].last_ul), 5)}
    p = rec["ms_per_step"]
    rec["ratio_to_plain"] = round(p["unlikelihood"] / p["plain"], 4)

    # the head launches alone, on the step's rows: stream 0 = the response (B x T rows, seq_len T), stream 1 = the auto-encoder's
    lib = L.load()
    y, ae_y = batch.trg_y.contiguous(), batch.query.contiguous()
    rows = [y.numel(), ae_y.numel()]
    R = sum(rows)
    g = torch.Generator(device=dev).manual_seed(3)
    logits = torch.randn(R, V, device=dev, generator=g)
    lse, rowloss, rowul = (torch.empty(R, device=dev) for _ in range(3))
    norm = torch.tensor([float((y != 1).sum()), float((ae_y != 1).sum())], device=dev)
    gloss = torch.ones(1, device=dev)
    dz = torch.empty(R, V, device=dev, dtype=torch.bfloat16)
    targets = [y.view(-1), ae_y.view(-1)]

    def block(cls):
        A = cls()
        A.n_seg = 2
        for s in range(2):
            A.rows[s], A.target[s], A.norm[s], A.coef[s] = rows[s], targets[s].data_ptr(), norm.data_ptr() + 4 * s, 1.0
        A.V, A.ldz, A.pad, A.smoothing, A.ldd = V, V, 1, 0.1, V
        A.logits, A.lse, A.rowloss, A.gloss, A.dlogits = logits.data_ptr(), lse.data_ptr(), rowloss.data_ptr(), gloss.data_ptr(), dz.data_ptr()
        return A

    H, U = block(L.LossHeadArgs), block(L.ULossHeadArgs)
    U.seq_len[0], U.ul_alpha, U.rowul = y.size(1), args.alpha, rowul.data_ptr()
    st = L.stream_ptr()
    code = L.dtype_code(torch.bfloat16)
    launches = {"plain_fwd": lambda: L.check(lib.mtn_losshead_fwd(C.byref(H), st)),
                "unlikelihood_fwd": lambda: L.check(lib.mtn_ulosshead_fwd(C.byref(U), st)),
                "plain_bwd": lambda: L.check(lib.mtn_losshead_bwd(code, C.byref(H), st)),
                "unlikelihood_bwd": lambda: L.check(lib.mtn_ulosshead_bwd(code, C.byref(U), st))}
    for fn in launches.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    head = {k: [] for k in launches}
    for _ in range(args.passes):
        for name, fn in launches.items():
            head[name].append(timed(fn, args.steps) * 1e3)
    rec["head_us_per_launch"] = {k: round(statistics.median(v), 2) for k, v in head.items()}
    rec["head_rows"] = {"response": rows[0], "auto_encoder": rows[1], "T": int(y.size(1))}
    print(json.dumps(rec))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
