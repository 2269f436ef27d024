#!/usr/bin/env python
"""ms/step of the training step with R-Drop next to the plain one: cfg2 (run.sh's model), bf16, dropout 0.1, captured graphs, the three
steps in ONE process, timed in alternated passes, medians over the passes:
    plain32   the plain step on 32 dialogues
    plain64   the plain step on 64 rows: the SAME rows as the doubled batch (the 32 dialogues twice)
    rdrop32   the R-Drop step from the 32 dialogues (it runs 64 rows: the refill copies, the paired loss head)
The comparison that matters is rdrop32 against plain64: the two differ by the refill and the head alone.  Then the two head launches on
their own, on the R-Drop step's rows (the response stream paired at distance B * T, the auto-encoder stream unpaired), between HIP events:
the plain pair and the paired pair.  The paired forward reads two rows per wave (three sweeps over both) where the plain one reads one
(two sweeps), the backward two rows in one sweep: about 2x the plain launches is what the design predicts.

    python tools/rdrop_bench.py [--steps 30] [--warmup 5] [--passes 5] [--out profiles/rdrop_train_bench.json]
                                [--parent-ms A B C --change-ms D E F]      bench.py's ms_per_step of the flag-off step, recorded next to it
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
    ap.add_argument("--parent-ms", type=float, nargs="*", default=None, help="bench.py's ms_per_step at the parent commit, one per fresh process")
    ap.add_argument("--change-ms", type=float, nargs="*", default=None, help="the same with this change, alternated with them: recorded as given")
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

    def fresh():
        torch.manual_seed(2)
        model = make_model(V, V, N=6, d_model=512, d_ff=2048, h=8, dropout=0.1, ft_sizes=fts, diff_encoder=True, auto_encoder_ft="query",
                           compute_dtype="bf16").to(dev).train()
        model.prepare()
        return model

    steps = {"rdrop32": TrainStep(fresh(), batch, V, pad=1, rdrop=args.alpha)}
    doubled = steps["rdrop32"].batch                               # 64 rows: the 32 dialogues twice (filled by the first step)
    steps["rdrop32"]()
    torch.cuda.synchronize()
    steps["plain32"] = TrainStep(fresh(), batch, V, pad=1)
    steps["plain64"] = TrainStep(fresh(), doubled, V, pad=1)
    for step in steps.values():
        for _ in range(args.warmup):
            step()
    torch.cuda.synchronize()
    names = ("plain32", "plain64", "rdrop32")
    passes = {k: [] for k in names}
    for _ in range(args.passes):
        for name in names:
            passes[name].append(timed(steps[name], args.steps))
    rec = {"workload": "cfg2", "batch": args.batch, "dtype": "bf16", "dropout": 0.1, "steps": args.steps, "warmup": args.warmup,
           "passes": args.passes, "rd_alpha": args.alpha,
           "ms_per_step": {k: round(statistics.median(v), 4) for k, v in passes.items()},
           "ms_per_step_passes": {k: [round(x, 4) for x in v] for k, v in passes.items()},
           "rd_per_token": round(float(steps["rdrop32"].last_rd), 6)}
    p = rec["ms_per_step"]
    rec["rdrop32_to_plain64"] = round(p["rdrop32"] / p["plain64"], 4)
    rec["rdrop32_to_plain32"] = round(p["rdrop32"] / p["plain32"], 4)

    # the head launches alone, on the R-Drop step's rows: stream 0 = the response (2 B x T rows, pair distance B T), stream 1 = the auto-encoder's
    lib = L.load()
    y, ae_y = doubled.trg_y.contiguous(), doubled.query.contiguous()
    rows = [y.numel(), ae_y.numel()]
    R = sum(rows)
    g = torch.Generator(device=dev).manual_seed(3)
    half = torch.randn(rows[0] // 2, V, device=dev, generator=g)
    logits = torch.cat([half, half + 0.1 * torch.randn(rows[0] // 2, V, device=dev, generator=g), torch.randn(rows[1], V, device=dev, generator=g)])
    lse, rowloss, rowrd, rowkl = (torch.empty(R, device=dev) for _ in range(4))
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

    H, P = block(L.LossHeadArgs), block(L.RLossHeadArgs)
    P.pair[0], P.rd_alpha, P.rowrd, P.rowkl = rows[0] // 2, args.alpha, rowrd.data_ptr(), rowkl.data_ptr()
    st = L.stream_ptr()
    code = L.dtype_code(torch.bfloat16)
    launches = {"plain_fwd": lambda: L.check(lib.mtn_losshead_fwd(C.byref(H), st)),
                "paired_fwd": lambda: L.check(lib.mtn_rlosshead_fwd(C.byref(P), st)),
                "plain_bwd": lambda: L.check(lib.mtn_losshead_bwd(code, C.byref(H), st)),
                "paired_bwd": lambda: L.check(lib.mtn_rlosshead_bwd(code, C.byref(P), st))}
    for fn in launches.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    head = {k: [] for k in launches}
    for _ in range(args.passes):
        for name, fn in launches.items():
            head[name].append(timed(fn, args.steps) * 1e3)
    rec["head_us_per_launch"] = {k: round(statistics.median(v), 2) for k, v in head.items()}
    rec["head_rows"] = {"response": rows[0], "auto_encoder": rows[1], "pair_distance": rows[0] // 2}
    if args.parent_ms and args.change_ms:                          # the flag-off step: bench.py, measured outside this process
        pm, cm = statistics.median(args.parent_ms), statistics.median(args.change_ms)
        rec["flag_off_bench_ms_per_step"] = {"parent": args.parent_ms, "change": args.change_ms, "median_parent": pm, "median_change": cm,
                                             "change_to_parent": round(cm / pm, 4)}
    rec["not_measured"] = ["any effect on validation loss or generated quality", "two ranks on two GPUs"]
    print(json.dumps(rec))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
