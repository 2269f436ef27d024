#!/usr/bin/env python
"""What the weight average costs: cfg2 (run.sh's model), batch 32, bf16, dropout 0.1.

  * the captured step with and without the EMA (TrainStep(ema_decay=...)), alternated in one process, median of --passes passes;
  * the EMA kernel alone over the model's flat buffer: median of 5 passes between HIP events on the launch stream, 12 bytes per element
    (average read + written, masters read), next to this box's streaming-copy rate (bench.py --full's peak_measured);
  * the one-rank RCCL schedule (a fresh process each, as bench.py's secondary.dp_schedule_one_rank) with and without the EMA: there the
    update is one launch per slice;
  * --parent-bench PATH/bench.py: this tree's bench.py (EMA off) and another checkout's, ALTERNATED in fresh processes — the EMA-off step
    against the parent commit (profiles/riders_ab.txt did the same by hand).  The other checkout must be built.

    python tools/ema_bench.py [--steps 30] [--warmup 5] [--passes 3] [--parent-bench ../parent/bench.py] [--out profiles/ema_train_bench.json]
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
DECAY = 0.999
V, FTS = 3000, [2048, 128]                                     # cfg2: run.sh's model, bench.py's flagship shapes


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
    """ms of one launch: median of 5 passes, each between its own pair of HIP events on the launch stream (bench.py's dominant kernel)"""
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


def hbm_peak(dev):
    import ctypes as C
    from mtn_amd import lib as L
    n = 1 << 30
    src = torch.empty(n, device=dev, dtype=torch.uint8)
    dst = torch.empty(n, device=dev, dtype=torch.uint8)
    src.zero_()
    g = C.c_double(0.0)
    L.check(L.load().mtn_measure_hbm_peak(src.data_ptr(), dst.data_ptr(), n, torch.cuda.current_stream().cuda_stream, C.byref(g)))
    return round(g.value, 1)


def dp_probe(args):
    """Child process: the data-parallel schedule on one rank, every collective through a one-rank RCCL group.  Prints one JSON object."""
    import time
    import torch.distributed as dist
    from mtn_amd import dp, lib
    from mtn_amd.synthetic import synthetic_batch
    from mtn_amd.train_step import TrainStep
    dp.init_distributed(force=True)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    lib.load()
    torch.manual_seed(0)
    model = make(dev).train()
    model.prepare()
    sync = dp.GradSync(lambda: model.flat_buffers()[2], force=True)
    sync.broadcast_(model._flat)
    batch = synthetic_batch(V, args.batch, 20, 128, 40, 20, [32, 32], FTS, device=dev, seed=1)
    st = TrainStep(model, batch, V, pad=1, warmup=4000, grad_sync=sync, ema_decay=args.dp_probe_decay)
    for _ in range(3):
        st()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        st()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / args.steps * 1e3
    print(json.dumps({"ms_per_step": round(ms, 4), "ema_decay": args.dp_probe_decay, "slices_per_step": len(st._slices()),
                      "segmented": bool(st.overlap), "dist_backend": dist.get_backend()}), flush=True)
    dist.destroy_process_group()


def last_json(text):
    for ln in reversed(text.strip().splitlines()):
        if ln.startswith("{"):
            return json.loads(ln)
    return None


def dp_one_rank(args, decay):
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ, MTN_FORCE_DIST="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--dp-probe", "--dp-probe-decay", str(decay), "--steps", str(args.steps),
                          "--batch", str(args.batch)], env=env, capture_output=True, text=True, timeout=240)
    return last_json(out.stdout) or {"error": (out.stderr or out.stdout)[-400:]}


def bench_ms(bench_py, steps, warmup):
    out = subprocess.run([sys.executable, bench_py, "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)], cwd=os.path.dirname(bench_py),
                         capture_output=True, text=True, timeout=300)
    rec = last_json(out.stdout)
    if rec is None:
        raise RuntimeError("no result line from %s: %s" % (bench_py, (out.stderr or out.stdout)[-400:]))
    print("%s: %.4f ms/step" % (bench_py, rec["ms_per_step"]), file=sys.stderr, flush=True)
    return rec["ms_per_step"]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--parent-bench", default=None, metavar="PATH", help="bench.py of a built checkout of the parent commit")
    ap.add_argument("--no-dp", action="store_true", help="skip the one-rank RCCL schedule")
    ap.add_argument("--out", default=None)
    ap.add_argument("--dp-probe", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--dp-probe-decay", type=float, default=0.0, help=argparse.SUPPRESS)
    args = ap.parse_args(argv)
    if args.dp_probe:
        return dp_probe(args)
    rec = {"workload": "cfg2", "batch": args.batch, "dtype": "bf16", "steps": args.steps, "warmup": args.warmup, "passes": args.passes,
           "ema_decay": DECAY}
    # fresh processes first: nothing of this process is on the GPU yet
    if args.parent_bench:
        ours = os.path.join(ROOT, "bench.py")
        ab = {"parent": [], "this_tree_ema_off": []}
        for _ in range(args.passes):
            ab["parent"].append(bench_ms(os.path.abspath(args.parent_bench), args.steps, args.warmup))
            ab["this_tree_ema_off"].append(bench_ms(ours, args.steps, args.warmup))
        mp, mt = statistics.median(ab["parent"]), statistics.median(ab["this_tree_ema_off"])
        ab.update(median_parent=mp, median_this_tree=mt, this_tree_vs_parent_percent=round((mt / mp - 1) * 100, 2),
                  what="ms per step of `bench.py --gpus 1`, both checkouts alternated in fresh processes (order inside a pass: parent, this tree)")
        rec["ema_off_vs_parent"] = ab
    if not args.no_dp:
        off, on = dp_one_rank(args, 0.0), dp_one_rank(args, DECAY)
        print("one-rank RCCL schedule: %s / %s" % (off, on), file=sys.stderr, flush=True)
        rec["dp_schedule_one_rank"] = {"ema_off": off, "ema_on": on,
                                       "what": "the step of a data-parallel rank on one GPU, every collective through a one-rank RCCL group "
                                               "(a fresh process each): the EMA is one launch per slice there"}
        if "ms_per_step" in off and "ms_per_step" in on:
            rec["dp_schedule_one_rank"]["ema_cost_ms"] = round(on["ms_per_step"] - off["ms_per_step"], 4)

    from mtn_amd import lib as L
    from mtn_amd.synthetic import synthetic_batch
    from mtn_amd.train_step import TrainStep
    dev = torch.device("cuda:0")
    batch = synthetic_batch(V, args.batch, 20, 128, 40, 20, [32, 32], FTS, device=dev, seed=1)
    steps = {}
    for key, decay in (("ema_off", 0.0), ("ema_on", DECAY)):
        torch.manual_seed(2)
        model = make(dev).train()
        model.prepare()
        steps[key] = TrainStep(model, batch, V, pad=1, ema_decay=decay)
    ms = {"ema_off": [], "ema_on": []}
    for _ in range(args.passes):                                 # alternated: off, on, off, on, ...
        for key in ("ema_off", "ema_on"):
            ms[key].append(round(timed(steps[key], args.steps, args.warmup), 4))
    med = {k: statistics.median(v) for k, v in ms.items()}
    rec["ms_per_step"] = {"passes": ms, "median": med, "ema_cost_ms": round(med["ema_on"] - med["ema_off"], 4),
                          "ema_cost_percent": round((med["ema_on"] / med["ema_off"] - 1) * 100, 2)}
    # the kernel alone, over this model's flat buffer
    adam = steps["ema_on"].opt.optimizer
    flat = steps["ema_on"].model._flat
    n = flat.numel()
    lib = L.load()
    k_ms, k_all = median_of_5(lambda: L.check(lib.mtn_ema_step(n, adam.ema.data_ptr(), flat.data_ptr(), adam.state.data_ptr(), DECAY, None, L.stream_ptr())))
    scratch = torch.empty_like(flat)
    s_ms, _ = median_of_5(lambda: L.check(lib.mtn_swap_f32(n, scratch.data_ptr(), adam.ema.data_ptr(), L.stream_ptr())))
    del steps, scratch
    peak = hbm_peak(dev)
    gbs = 12.0 * n / (k_ms * 1e-3) / 1e9
    rec["ema_kernel"] = {"elements": n, "bytes": 12 * n, "ms": round(k_ms, 4), "ms_passes": [round(x, 4) for x in k_all], "GB_per_s": round(gbs, 1),
                         "peak_measured_GB_per_s": peak, "frac_of_peak_measured": round(gbs / peak, 3),
                         "table_launch_frac_of_peak_measured": "0.77-0.93 (README)",
                         "swap_ms": round(s_ms, 4), "swap_GB_per_s": round(16.0 * n / (s_ms * 1e-3) / 1e9, 1),
                         "what": "mtn_ema_step over the model's whole flat fp32 buffer: 4 B read + 4 B written of the average, 4 B read of the "
                                 "masters per element; peak_measured = this box's 16-byte-per-lane streaming copy (bench.py --full)"}
    print(json.dumps(rec))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
