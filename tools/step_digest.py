"""Bit-level fingerprint of the training step, for A/B runs of two checkouts that must compute the same thing (a refactor of the
Python that feeds the kernels): one process, fixed seeds, atomic-free embedding gradients, a fixed list of cases.

  python tools/step_digest.py --out a.json        # in checkout A;  likewise b.json in checkout B (same libmtn_hip.so sources)
  python tools/step_digest.py --compare a.json b.json      # exit status 1 and the differing cases if any digest differs

A case = golden config x compute dtype x lockstep on/off x schedule (eager step, captured step, layer-segmented captured step),
three optimiser steps with every fused dropout site at 0.1 (the feature streams' torch dropout, which has an RNG of its own, is
off, as in the suite's bitwise tests).  Per case: SHA-256 of the three losses, of the flat parameter buffer, of both Adam
moments, and of the launch census of everything Python enqueued (variant, workgroups, count, M/N/K per launch); beside them the
library's group counters (fused / per-stage kernels, LayerNorm-fold epilogues), which say what paths the case took.  `wide` is
wide_n1 with two layers at batch 4: d_model 512 / 8 heads, where the LayerNorm-fold epilogue and the transposed-weight dX paths
engage."""
import os, sys, json, hashlib, argparse, struct, ctypes as C
os.environ["MTN_EMBED_DETERMINISTIC"] = "1"
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

STEPS = 3


class NoSync:
    """dp.GradSync's call surface on one rank (no exchange): what turns the layer-segmented schedule on."""
    world = 1

    def all_reduce_scalars(self, t):
        return t

    def reduce_range(self, lo, hi):
        return None

    def wait(self, handles):
        pass

    def __call__(self):
        pass


def cases():
    import torch
    from oracle import fixtures as fx
    configs = {k: fx.GOLDEN_CONFIGS[k] for k in ("cfg1_query", "small_shared", "small_diffall")}
    configs["wide"] = dict(fx.GOLDEN_CONFIGS["wide_n1"], N=2, B=4)
    for name, c in configs.items():
        for dtype in (torch.bfloat16,) if name == "wide" else (torch.bfloat16, torch.float32):
            for lockstep in (True, False):
                for schedule in ("eager", "graph", "segmented-graph"):
                    yield f"{name}/{str(dtype)[6:]}/{'lockstep' if lockstep else 'sequential'}/{schedule}", c, dtype, lockstep, schedule


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def run_case(c, dtype, lockstep, schedule, dev):
    import torch
    from mtn_amd import Batch, make_model, lib as L
    from mtn_amd.train_step import TrainStep
    from oracle import fixtures as fx
    torch.manual_seed(0)
    model = make_model(c["vocab"], c["vocab"], N=c["N"], d_model=c["d_model"], d_ff=c["d_ff"], h=c["h"], dropout=0.1,
                       ft_sizes=c["ft_sizes"], diff_encoder=c["diff_encoder"], diff_embed=c["diff_embed"], diff_gen=c["diff_gen"],
                       auto_encoder_ft=c["auto_encoder_ft"], compute_dtype=dtype, attn_dropout=0.1)
    model.load_state_dict(fx.det_state_dict(fx.state_shapes(**c), 0), strict=False)
    model.to(dev).train()
    for mod in model.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    model.lockstep = lockstep
    raw = fx.det_batch(c["vocab"], c["B"], c["Q"], c["H"], c["C"], c["T"], c["frames"], c["ft_sizes"], seed=1)
    t = torch.from_numpy
    b = Batch(t(raw["query"]), t(raw["his"]), None, [t(f) for f in raw["fts"]], t(raw["cap"]), t(raw["trg"]), t(raw["trg_y"]),
              pad=fx.PAD, device=dev)
    seg = schedule == "segmented-graph"
    ts = TrainStep(model, b, c["vocab"], pad=fx.PAD, warmup=20, grad_sync=NoSync() if seg else None, use_graph=schedule != "eager",
                   overlap=seg)
    model.prepare()
    model._seed.fill_(4242)
    lib = L.load()
    fused0, epi0 = L.fused_counters(), lib.mtn_ln_epilogue_groups()
    lib.mtn_census_begin()
    losses = [float(ts()) for _ in range(STEPS)]
    torch.cuda.synchronize()
    n = lib.mtn_census_end()
    census = hashlib.sha256()
    for i in range(n):
        info = L.CensusLaunch()
        lib.mtn_census_info(i, C.byref(info))
        k = min(4, info.count)
        census.update(struct.pack("<4i", info.dtype, info.variant, info.workgroups, info.count))
        census.update(struct.pack(f"<{3 * k}i", *info.M[:k], *info.N[:k], *info.K[:k]))
    adam = ts.opt.optimizer
    return dict(loss=hashlib.sha256(struct.pack(f"<{STEPS}d", *losses)).hexdigest(), losses=[x.hex() for x in losses],
                params=sha(model._flat), exp_avg=sha(adam.m), exp_avg_sq=sha(adam.v), census=census.hexdigest(), launches=n,
                segmented=bool(ts.overlap),
                # groups on the fused forward / per-stage forward / fused backward / per-stage backward kernels, and backward groups
                # with a LayerNorm-fold epilogue: which paths the case took
                fused_groups=[b - a for a, b in zip(fused0, L.fused_counters())], ln_epilogue_groups=lib.mtn_ln_epilogue_groups() - epi0)


def compare(pa, pb):
    a, b = (json.load(open(p)) for p in (pa, pb))
    bad = [k for k in sorted(set(a) | set(b)) if a.get(k) != b.get(k)]
    for k in bad:
        fields = [f for f in (a.get(k) or b.get(k)) if (a.get(k) or {}).get(f) != (b.get(k) or {}).get(f)]
        print(f"DIFFERENT {k}: {' '.join(fields)}")
    print(f"{len(a)} / {len(b)} cases, {len(bad)} differ")
    return 1 if bad or not a else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--only", help="substring of the case names to run")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    import torch
    dev = torch.device("cuda:0")
    out = {}
    for name, c, dtype, lockstep, schedule in cases():
        if args.only and args.only not in name:
            continue
        try:
            out[name] = run_case(c, dtype, lockstep, schedule, dev)
        except (ValueError, AssertionError, NotImplementedError) as e:      # a combination the step refuses: recorded as such
            out[name] = dict(refused=f"{type(e).__name__}: {e}")
            torch.cuda.synchronize()                                        # (anything else, a device error included, ends the run)
        print(name, json.dumps(out[name]), flush=True)
        if args.out:
            with open(args.out, "w") as f:
                json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
