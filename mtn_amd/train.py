#!/usr/bin/env python
"""Training entry point with the reference's model/optimiser flags (train.py:57-96), so that the `python train.py ...`
line of run.sh:109-140 can launch this implementation:  python -m mtn_amd.train --nb-blocks 6 --d-model 512 ...

Three modes:
  * ``--train-set <json> --train-path <.../<FeaType>/<ImageID>.npy>`` (what run.sh passes): the reference's pipeline —
    vocabulary from the training annotations, DSTC7-AVSD json + per-video .npy features loaded once and uploaded whole
    (mtn_amd.data_handler), length-bucketed batches, an epoch loop on captured graphs per padded shape (or ``--eager``),
    validation loss after every epoch, <model>.conf / <model>_params.txt / <model>_N.pth.tar / <model>_best.pth.tar written
    as train.py:166-225 does (checkpoints are state_dicts in the reference's key schema);
  * ``--corpus-videos N``: the same loop on a synthetic ragged corpus;
  * neither: one fixed-shape synthetic batch replayed (throughput runs).
One process per GPU under torchrun gives data parallelism (RCCL all-reduce of the flat gradient buffer).
"""
import argparse
import copy
import logging
import time

import torch

from . import dp, make_model
from .synthetic import synthetic_batch
from .train_step import TrainStep


def parse(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--gpu", "-g", default=0, type=int)
    # data flags of the reference (train.py:59-73); synthetic data is used when --train-set is empty
    for f in ("--fea-type",):
        p.add_argument(f, nargs="+", type=str, default=["i3d_rgb", "vggish"])
    for f in ("--train-path", "--train-set", "--valid-path", "--valid-set", "--model"):
        p.add_argument(f, default="", type=str)
    p.add_argument("--include-caption", default="none", type=str)
    p.add_argument("--separate-caption", default=1, type=int)
    p.add_argument("--cut-a", default=0, type=int,
                   help="1: randomly truncate answers as the reference's training recipe does (data_handler.py:255-260), training "
                        "and validation batches, draws from numpy RandomState(--rand-seed) — corpus mode only")
    p.add_argument("--merge-source", default=0, type=int)
    p.add_argument("--exclude-video", action="store_true")
    p.add_argument("--fixed-word-emb", default=0, type=int)
    # model (train.py:75-84)
    p.add_argument("--nb-blocks", default=6, type=int)
    p.add_argument("--d-model", default=512, type=int)
    p.add_argument("--d-ff", default=2048, type=int)
    p.add_argument("--att-h", default=8, type=int)
    p.add_argument("--dropout", default=0.1, type=float)
    p.add_argument("--separate-his-embed", default=0, type=int)
    p.add_argument("--separate-cap-embed", default=0, type=int)
    p.add_argument("--diff-encoder", default=1, type=int)
    p.add_argument("--diff-embed", default=0, type=int)
    p.add_argument("--diff-gen", default=0, type=int)
    p.add_argument("--auto-encoder-ft", default="query", type=str)
    # training (train.py:86-93)
    p.add_argument("--num-epochs", "-e", default=1, type=int)
    p.add_argument("--rand-seed", "-s", default=1, type=int)
    p.add_argument("--batch-size", "-b", default=32, type=int)
    p.add_argument("--max-length", default=20, type=int)
    p.add_argument("--max-history-length", default=-1, type=int)
    p.add_argument("--report-interval", default=100, type=int)
    p.add_argument("--warmup-steps", default=4000, type=int)
    p.add_argument("--loss-l", default=1.0, type=float)
    p.add_argument("--verbose", "-v", default=0, type=int)
    # this implementation
    p.add_argument("--compute-dtype", default="bf16", choices=["bf16", "fp32"])
    p.add_argument("--steps-per-epoch", default=200, type=int, help="synthetic mode: batches per epoch")
    p.add_argument("--vocab-size", default=3000, type=int, help="synthetic mode")
    p.add_argument("--ft-sizes", default=[2048, 128], nargs="+", type=int, help="synthetic mode: feature dims")
    p.add_argument("--lens", default=[20, 128, 40, 20, 32], nargs=5, type=int, help="synthetic mode: Q H C T frames")
    p.add_argument("--valid-videos", default=0, type=int,
                   help="corpus mode: a held-out synthetic corpus of that many videos; its mean loss per token is evaluated in eval() mode "
                        "after every epoch and the best model is kept as <model>_best (train.py:201-224)")
    p.add_argument("--resume", default="", type=str,
                   help="corpus mode: checkpoint prefix to continue from (<prefix>.pth.tar = model state_dict in the reference's key "
                        "schema, <prefix>_opt.pth.tar = optimiser moments + schedule state); the --cut-a draw stream restarts "
                        "from --rand-seed")
    p.add_argument("--eager", action="store_true", help="corpus mode: one eager step per batch instead of captured graphs per padded shape")
    p.add_argument("--bucket", default=8, type=int, help="corpus mode: batch lengths are rounded up to multiples of this")
    p.add_argument("--corpus-max-answer", default=18, type=int, help="synthetic corpus: longest answer (AVSD's reach 52 tokens)")
    p.add_argument("--corpus-max-question", default=20, type=int, help="synthetic corpus: longest question (AVSD's reach 42 tokens)")
    p.add_argument("--corpus-videos", default=0, type=int,
                   help="> 0: train on a synthetic ragged CORPUS of that many videos (10 turns each) through the reference's "
                        "epoch loop — batch planning, device-side batch assembly, one eager step per batch — instead of "
                        "replaying one fixed-shape batch")
    # knowledge distillation (word level): frozen teacher checkpoints whose next-token distribution the student is trained against
    p.add_argument("--distill-model", default=[], nargs="+", type=str, metavar="PREFIX",
                   help="teacher checkpoint prefix(es) (<prefix>.pth.tar, as generate.py's --model), at most 8; several form an ensemble teacher")
    p.add_argument("--distill-conf", default=[], nargs="+", type=str, metavar="CONF",
                   help="the teachers' <model>.conf: one per --distill-model entry, or one for all")
    p.add_argument("--distill-weights", default=None, nargs="+", type=float, help="one weight >= 0 per teacher (default: uniform)")
    p.add_argument("--distill-mode", default="prob", choices=["prob", "logprob"], help="how several teachers are combined (generate.py --ensemble-mode)")
    p.add_argument("--distill-alpha", default=0.5, type=float, help="loss = (1 - alpha) * label-smoothed KL + alpha * T^2 * KL(teacher || student)")
    p.add_argument("--distill-temperature", default=1.0, type=float, help="T: both distributions are softmax(. / T) in the soft term")
    # averaging in weight space: an exponential moving average of the weights kept by the optimiser inside the step
    p.add_argument("--ema-decay", default=0.0, type=float, metavar="D",
                   help="0 < D < 1: keep ema += max(1 - D, 9 / (10 + step)) * (weights - ema) after every optimiser step; with --model every epoch "
                        "also writes <model>_N_ema, validation runs a second time under the averaged weights and its best is kept as "
                        "<model>_best_ema (0: off)")
    # self-critical sequence training: sampled responses scored against the corpus' answers, row weight -(reward - baseline)
    p.add_argument("--scst-samples", default=0, type=int, metavar="S",
                   help="2..16: corpus mode trains on S sampled responses per dialogue, scored on the device against the corpus' answers "
                        "(Rennie et al. 2017); responses have min(--max-length, 129) positions (0: off)")
    p.add_argument("--scst-reward", default="cider", choices=["cider", "rouge"], help="the metric a sample is rewarded with")
    p.add_argument("--scst-baseline", default="mean", choices=["mean", "greedy"],
                   help="mean: the leave-one-out mean of the dialogue's other samples; greedy: the reward of the greedy response")
    p.add_argument("--scst-temperature", default=1.0, type=float)
    p.add_argument("--scst-top-k", default=0, type=int)
    p.add_argument("--scst-top-p", default=1.0, type=float)
    p.add_argument("--scst-xe-weight", default=0.0, type=float, metavar="W",
                   help="> 0: the gold answer is one more row per dialogue with the constant weight W (smoothing 0)")
    # unlikelihood training: the training-time repetition penalty (generate.py's --no-repeat-ngram / --repetition-penalty act at decode time)
    p.add_argument("--unlikelihood-alpha", default=0.0, type=float, metavar="A",
                   help="> 0: the response stream's loss gains A * sum over each target position of -log(1 - p(c)) over the response's "
                        "earlier tokens c (Welleck et al. 2019); validation stays the plain loss (0: off)")
    # gradient clipping by global norm, as torch.nn.utils.clip_grad_norm_: the cap every Transformer recipe carries next to Adam
    p.add_argument("--clip-grad-norm", default=0.0, type=float, metavar="C",
                   help="C > 0: every step's gradient is multiplied by min(1, C / (its global L2 norm + 1e-6)) on the device before Adam "
                        "reads it (inf: measure the norm, never clip); the step then takes the separate optimiser pass; every epoch logs "
                        "the mean and largest norm and how many steps were clipped (0: off)")
    # gradient accumulation: an effective batch of K assembled batches per optimiser update, without holding one padded batch of that size
    p.add_argument("--accum-steps", default=1, type=int, metavar="K",
                   help="K > 1: the optimiser updates once per window of K consecutive batches, from the token-weighted mean of their "
                        "gradients, accumulated on the device (an epoch's last window may be shorter); under several ranks the gradient "
                        "exchange runs once per window; every epoch logs its updates (1: off)")
    # scheduled sampling: the decoder is fed a mix of gold tokens and the model's own predictions from one extra eval() forward per step
    p.add_argument("--sched-sample-prob", default=0.0, type=float, metavar="P",
                   help="0 < P <= 1: before every training forward the model runs once over the gold prefix and a fraction P of the "
                        "decoder's input tokens is replaced by its predictions (two-pass scheduled sampling: Mihaylova & Martins 2019, "
                        "Duckworth et al. 2019); targets, validation and checkpoints are unchanged; every epoch logs the replaced "
                        "tokens (0: off)")
    p.add_argument("--sched-sample-start", default=0, type=int, metavar="S", help="optimiser updates before any token is replaced")
    p.add_argument("--sched-sample-ramp", default=0, type=int, metavar="R",
                   help="the fraction grows linearly from 0 to P over R updates after --sched-sample-start (0: P at once)")
    p.add_argument("--sched-sample-pick", default="argmax", choices=["argmax", "sample"],
                   help="argmax: the most likely token; sample: a draw from softmax(logits / --sched-sample-temperature)")
    p.add_argument("--sched-sample-temperature", default=1.0, type=float)
    p.add_argument("--sched-sample-seed", default=0, type=int, help="seed of the coins and draws (the update count is added on the device)")
    # R-Drop: every dialogue runs through the model twice under independent dropout masks, in one doubled batch
    p.add_argument("--rdrop-alpha", default=0.0, type=float, metavar="A",
                   help="> 0: every batch is trained on twice in one step, rows b and B + b the same dialogue under two dropout masks, and "
                        "the response stream's loss gains A / 4 * (KL(p || q) + KL(q || p)) between the two passes' next-token distributions "
                        "per target token (R-Drop: Liang et al. 2021); --batch-size B keeps meaning B dialogues: the step runs 2 B rows and "
                        "needs that much activation memory; validation stays the plain loss on the undoubled batch; every epoch logs the "
                        "mean divergence (0: off)")
    args = p.parse_args(argv)
    err = (distill_flag_error(args) or ema_flag_error(args) or scst_flag_error(args) or unlikelihood_flag_error(args) or clip_flag_error(args)
           or accum_flag_error(args) or sched_flag_error(args) or rdrop_flag_error(args))
    if err:
        p.error(err)
    return args


DISTILL_MAX_TEACHERS = 8


def distill_flag_error(args):
    """What is wrong with the --distill-* flags, as one line (None: nothing)."""
    import math
    n = len(args.distill_model)
    if args.distill_conf and not n:
        return "--distill-conf needs --distill-model"
    if not (0.0 <= args.distill_alpha <= 1.0):
        return "--distill-alpha must lie in [0, 1] (got %r)" % args.distill_alpha
    if not (args.distill_temperature > 0.0 and math.isfinite(args.distill_temperature)):
        return "--distill-temperature must be finite and > 0 (got %r)" % args.distill_temperature
    if not n:
        if args.distill_weights is not None:
            return "--distill-weights needs --distill-model"
        return None
    if n > DISTILL_MAX_TEACHERS:
        return "--distill-model takes at most %d teachers (%d given)" % (DISTILL_MAX_TEACHERS, n)
    if not args.distill_conf:
        return "--distill-model needs --distill-conf (the teachers' <model>.conf)"
    if len(args.distill_conf) not in (1, n):
        return "--distill-conf takes one conf per --distill-model entry or one for all (%d given for %d)" % (len(args.distill_conf), n)
    w = args.distill_weights
    if w is not None:
        if len(w) != n:
            return "--distill-weights takes one weight per --distill-model entry (%d given for %d)" % (len(w), n)
        if not all(math.isfinite(x) and x >= 0 for x in w) or not any(x > 0 for x in w):
            return "--distill-weights must be finite and >= 0, and not all 0"
    return None


def scst_flag_error(args, world=None):
    """What is wrong with the --scst-* flags, or what they conflict with, as one line (None: nothing).  ``world``: the number of ranks
    (None: what the launcher's WORLD_SIZE says)."""
    import math
    import os
    S = args.scst_samples
    if S == 0:
        return None
    if not 2 <= S <= 16:
        return "--scst-samples must be 0 (off) or lie in 2..16 (got %r)" % S
    if not (args.scst_temperature >= 0.0 and math.isfinite(args.scst_temperature)):
        return "--scst-temperature must be finite and >= 0 (got %r)" % args.scst_temperature
    if args.scst_top_k < 0:
        return "--scst-top-k must be >= 0 (got %r)" % args.scst_top_k
    if not 0.0 < args.scst_top_p <= 1.0:
        return "--scst-top-p must lie in (0, 1] (got %r)" % args.scst_top_p
    if not (args.scst_xe_weight >= 0.0 and math.isfinite(args.scst_xe_weight)):
        return "--scst-xe-weight must be finite and >= 0 (got %r)" % args.scst_xe_weight
    if args.max_length < 2:
        return "--scst-samples needs --max-length >= 2, the positions of a sampled response (got %r)" % args.max_length
    if args.distill_model:
        return "--scst-samples does not combine with --distill-model: distillation under self-critical training is out of scope"
    if world is None:
        world = int(os.environ.get("WORLD_SIZE", "1") or 1)
    if world > 1:
        return "--scst-samples does not combine with more than one rank (%d): data parallelism under self-critical training is out of scope" % world
    if not args.train_set and args.corpus_videos <= 0:
        return ("--scst-samples does not combine with the fixed synthetic batch: rewards need a corpus of answers "
                "(--train-set or --corpus-videos)")
    return None


def unlikelihood_flag_error(args):
    """What is wrong with --unlikelihood-alpha, or what it conflicts with, as one line (None: nothing).  0 = off."""
    import math
    a = args.unlikelihood_alpha
    if not (a >= 0.0 and math.isfinite(a)):        # (nan fails the comparison)
        return "--unlikelihood-alpha must be finite and >= 0 (got %r)" % a
    if a > 0.0 and args.distill_model:
        return "--unlikelihood-alpha does not combine with --distill-model: unlikelihood under distillation is out of scope"
    if a > 0.0 and args.scst_samples:
        return "--unlikelihood-alpha does not combine with --scst-samples: unlikelihood under self-critical training is out of scope"
    return None


def rdrop_flag_error(args):
    """What is wrong with --rdrop-alpha, or what it conflicts with, as one line (None: nothing).  0 = off."""
    import math
    a = args.rdrop_alpha
    if not (a >= 0.0 and math.isfinite(a)):        # (nan fails the comparison)
        return "--rdrop-alpha must be finite and >= 0 (got %r)" % a
    if a == 0.0:
        return None
    if args.distill_model:
        return "--rdrop-alpha does not combine with --distill-model: R-Drop under distillation would be a combined loss head, out of scope"
    if args.scst_samples:
        return "--rdrop-alpha does not combine with --scst-samples: R-Drop under self-critical training is out of scope"
    if args.unlikelihood_alpha > 0.0:
        return "--rdrop-alpha does not combine with --unlikelihood-alpha: R-Drop with unlikelihood would be a combined loss head, out of scope"
    if args.sched_sample_prob > 0.0:
        return ("--rdrop-alpha does not combine with --sched-sample-prob: the mix keys rows by batch index, so the two passes of a dialogue "
                "would see different inputs")
    return None


def clip_flag_error(args, world=None):
    """What is wrong with --clip-grad-norm, or what it conflicts with, as one line (None: nothing).  0 = off; inf is allowed.  ``world``:
    the number of ranks (None: what the launcher's WORLD_SIZE says)."""
    import os
    c = args.clip_grad_norm
    if not c >= 0.0:                               # (nan fails the comparison)
        return "--clip-grad-norm must be 0 (off) or > 0, inf allowed (got %r)" % c
    if c == 0.0:
        return None
    if world is None:
        world = int(os.environ.get("WORLD_SIZE", "1") or 1)
    if world > 1 and os.environ.get("MTN_DP_SHARDED", "0") != "0":
        return ("--clip-grad-norm does not combine with the sharded data-parallel optimiser (MTN_DP_SHARDED=%s): clipping under it is out "
                "of scope; leave MTN_DP_SHARDED unset or 0" % os.environ["MTN_DP_SHARDED"])
    return None


def accum_flag_error(args, world=None):
    """What is wrong with --accum-steps, or what it conflicts with, as one line (None: nothing).  1 = off.  ``world``: the number of ranks
    (None: what the launcher's WORLD_SIZE says)."""
    import os
    k = args.accum_steps
    if k < 1:
        return "--accum-steps must be an integer >= 1 (got %r)" % k
    if k == 1:
        return None
    if args.scst_samples:
        return ("--accum-steps does not combine with --scst-samples: accumulation under self-critical training is out of scope "
                "(a self-critical step is one update per call)")
    if world is None:
        world = int(os.environ.get("WORLD_SIZE", "1") or 1)
    if world > 1 and os.environ.get("MTN_DP_SHARDED", "0") != "0":
        return ("--accum-steps does not combine with the sharded data-parallel optimiser (MTN_DP_SHARDED=%s): accumulation under it is out "
                "of scope; leave MTN_DP_SHARDED unset or 0" % os.environ["MTN_DP_SHARDED"])
    return None


def sched_flag_error(args, world=None):
    """What is wrong with the --sched-sample-* flags, or what they conflict with, as one line (None: nothing).  0 = off.  ``world``: the
    number of ranks (scheduled sampling runs under any number; the argument keeps the siblings' signature)."""
    import math
    pr = args.sched_sample_prob
    if not 0.0 <= pr <= 1.0:                       # (nan fails the comparison)
        return "--sched-sample-prob must be 0 (off) or lie in (0, 1] (got %r)" % pr
    if args.sched_sample_start < 0:
        return "--sched-sample-start must be >= 0 (got %r)" % args.sched_sample_start
    if args.sched_sample_ramp < 0:
        return "--sched-sample-ramp must be >= 0 (got %r)" % args.sched_sample_ramp
    if not (args.sched_sample_temperature > 0.0 and math.isfinite(args.sched_sample_temperature)):
        return "--sched-sample-temperature must be finite and > 0 (got %r)" % args.sched_sample_temperature
    if not 0 <= args.sched_sample_seed < 2 ** 62:
        return "--sched-sample-seed must lie in [0, 2^62) (got %r)" % args.sched_sample_seed
    if pr == 0.0:
        return None
    if args.distill_model:
        return ("--sched-sample-prob does not combine with --distill-model: the teacher would have to see the mixed inputs; scheduled "
                "sampling under distillation is out of scope")
    if args.scst_samples:
        return "--sched-sample-prob does not combine with --scst-samples: scheduled sampling under self-critical training is out of scope"
    return None


def sched_config(args):
    """The --sched-sample-* flags as a train_step.SchedConfig (None: off).  <sos> = 2 is never picked (nor is <pad>)."""
    if args.sched_sample_prob == 0.0:
        return None
    from .train_step import SchedConfig
    return SchedConfig(args.sched_sample_prob, start=args.sched_sample_start, ramp=args.sched_sample_ramp, pick=args.sched_sample_pick,
                       temperature=args.sched_sample_temperature, seed=args.sched_sample_seed, banned=(2,))


def sched_epoch_report(cfg, stats, step_count, epoch, rank):
    """The epoch's scheduled-sampling line from the device counter block (one small D2H copy; the block is reset; the ranks' counts are
    summed).  ``step_count``: the optimiser's update count, at which p is quoted."""
    st = stats.clone()
    stats.zero_()
    if torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1:
        torch.distributed.all_reduce(st)
    n, k, d = (int(v) for v in st.tolist())
    if rank == 0:
        print("epoch %d scheduled sampling: p %f replaced %d of %d target tokens, %d differ from gold" % (epoch + 1, cfg.prob_at(step_count), k, n, d))


def clip_epoch_report(adam, epoch, rank):
    """The epoch's gradient-norm line from the optimiser's stats block (one small D2H copy; the block is reset).  A step whose norm
    was not finite wrote NaN into the weights: the run ends here, before anything of this epoch is saved."""
    st = adam.clip_stats(reset=True)
    if rank == 0:
        print("epoch %d gradient norm: mean %f max %f clipped %d of %d steps" % (epoch + 1, st["mean"], st["max"], st["clipped"], st["steps"]))
    if st["nonfinite"] > 0:
        raise SystemExit("mtn_amd.train: epoch %d: the gradient norm was not finite in %d of %d steps; the weights are NaN, no checkpoint "
                         "of this epoch is written" % (epoch + 1, st["nonfinite"], st["steps"]))


def ema_flag_error(args):
    """What is wrong with --ema-decay, as one line (None: nothing).  0 = off."""
    d = args.ema_decay
    if d != 0.0 and not (0.0 < d < 1.0):           # (nan fails both comparisons)
        return "--ema-decay must be 0 (off) or lie in (0, 1) (got %r)" % d
    return None


def vocab_difference(student, teacher):
    """The first word (in the student's id order, then the teacher's) whose id differs between two word -> id maps, as a phrase; None
    when the maps are equal."""
    for w, i in sorted(student.items(), key=lambda kv: kv[1]):
        if w not in teacher:
            return "word %r (id %d) is missing from it" % (w, i)
        if teacher[w] != i:
            return "word %r has id %d there and %d here" % (w, teacher[w], i)
    for w, i in sorted(teacher.items(), key=lambda kv: kv[1]):
        if w not in student:
            return "its word %r (id %d) is not in the student's vocabulary" % (w, i)
    return None


def check_distill_confs(confs, names, vocab, args):
    """A teacher scores the student's batches: its word -> id map must be the student's (``vocab``; None on synthetic data, where only
    the size can be compared) and, when the student reads a data set, the data-shaping fields generate.check_ensemble_confs compares
    must equal the student's arguments.  SystemExit naming the first teacher and the first difference."""
    from .generate import ENSEMBLE_DATA_FIELDS
    for (tv, ta), name in zip(confs, names):
        if vocab is not None:
            diff = vocab_difference(dict(vocab), dict(tv))
            if diff is not None:
                raise SystemExit("distillation: the vocabulary of %s differs from the student's: %s" % (name, diff))
            for f in ENSEMBLE_DATA_FIELDS:
                if getattr(ta, f) != getattr(args, f):
                    raise SystemExit("distillation: %s of %s is %r, the student's is %r: teacher and student read the same data"
                                     % (f, name, getattr(ta, f), getattr(args, f)))
        elif len(tv) != args.vocab_size:
            raise SystemExit("distillation: the vocabulary of %s has %d words, the student's %d" % (name, len(tv), args.vocab_size))


def load_teacher(args, vocab, dev):
    """The --distill-model checkpoints as one frozen teacher: a model, or a decode.Ensemble of them (None without the flag).  Loaded as
    generate.py loads --model / --ensemble-model; a teacher at weight 0 is not loaded."""
    if not args.distill_model:
        return None
    from . import generate as gen
    n = len(args.distill_model)
    paths = list(args.distill_conf) * (n if len(args.distill_conf) == 1 else 1)
    confs = [gen.load_conf(c) for c in paths]
    check_distill_confs(confs, ["%s (teacher %d)" % (c, i) for i, c in enumerate(paths)], vocab, args)
    weights = list(args.distill_weights) if args.distill_weights is not None else [1.0] * n
    members = []
    for prefix, (tv, ta), w in zip(args.distill_model, confs, weights):
        if w == 0:
            logging.info("distillation: %s has weight 0 and is not loaded", prefix)
            continue
        logging.info("Loading teacher params from " + prefix)
        members.append(gen.build_model(tv, ta, args.ft_sizes, gen.load_state_dict(prefix + ".pth.tar"), args.compute_dtype, dev))
    for m in members:
        for q in m.parameters():
            q.requires_grad_(False)
    if len(members) == 1:
        teacher = members[0]
    else:
        from .decode import Ensemble
        teacher = Ensemble(members, [w for w in weights if w != 0], args.distill_mode)
    logging.info("distillation: %d teacher(s), mode %s, alpha %g, temperature %g", len(members), args.distill_mode, args.distill_alpha,
                 args.distill_temperature)
    return teacher


def synthetic_corpus(n_videos, vocab, ft_sizes, seed, turns=10, max_answer=18, max_question=20):
    """A ragged corpus in the layout data_handler.load returns (dialogs + per-video feature arrays), lengths in the ranges
    of the AVSD data: questions/answers 3-20 tokens, captions 10-40, 20-40 frames per video."""
    import numpy as np
    rs = np.random.RandomState(seed)
    tok = lambda lo, hi: rs.randint(4, vocab, size=rs.randint(lo, hi + 1)).astype(np.int64)
    dialogs, qa = [], 0
    vids = [f"v{v:05d}" for v in range(n_videos)]
    for v in vids:
        cap, hist = tok(10, 40), np.zeros(0, np.int64)
        for _ in range(turns):
            q, a = tok(3, max_question), tok(3, max_answer)
            ans = np.concatenate([[2], a, [3]]).astype(np.int64)                     # <sos> ... <eos>
            dialogs.append([v, qa, hist.copy() if len(hist) else np.array([1], np.int64), q, ans[:-1], ans[1:], cap])
            hist = np.concatenate([hist, q, a])
            qa += 1
    feats = [{v: rs.randn(rs.randint(20, 41), F).astype(np.float32) for v in vids} for F in ft_sizes]
    return {"dialogs": dialogs, "features": feats, "vocab": {"<blank>": 1}}


def cut_a_applies(args) -> bool:
    """--cut-a truncates the answers of corpus-mode batches (--train-set or --corpus-videos); the fixed synthetic batch of
    throughput runs is never truncated, which a warning says."""
    corpus_mode = bool(args.train_set) or args.corpus_videos > 0
    if args.cut_a and not corpus_mode:
        logging.warning("--cut-a %d is ignored: answer truncation applies to corpus mode only (--train-set or --corpus-videos), "
                        "not to the fixed synthetic batch", args.cut_a)
    return bool(args.cut_a) and corpus_mode


def run_epoch_graphed(trainer, indices, epoch, report_interval, rank, rng, cut=None, stats=None):
    """The same epoch on captured graphs (train_step.BucketedTrainer): lengths rounded up to the bucket, one graph per padded
    shape, batches assembled in place on the device; the host only syncs at the report interval.  ``cut``: the --cut-a
    RandomState (None = no truncation).  Returns (mean loss per token, target tokens of the epoch over all ranks).  ``stats``: a dict
    that receives "kd", the epoch's mean distillation KL per token, when the trainer has a teacher, "ul", the epoch's mean unlikelihood per
    token, when it trains with unlikelihood, "rd", the epoch's mean R-Drop divergence per token, when it trains with R-Drop (the token
    counts are then the doubled batches': both passes), and "reward" / "baseline", the
    mean over the epoch's steps of the steps' mean reward and mean baseline, when it trains self-critically."""
    order = list(range(len(indices)))
    rng.shuffle(order)
    dev = trainer.corpus.device
    loss_sum = torch.zeros((), device=dev)
    scst = getattr(trainer, "scst", None) is not None
    rl_sum = torch.zeros(2, device=dev, dtype=torch.float64)
    kd_sum = torch.zeros((), device=dev) if trainer.teacher is not None else None
    ul_sum = torch.zeros((), device=dev) if getattr(trainer, "unlikelihood", 0.0) > 0.0 else None
    rd_sum = torch.zeros((), device=dev) if getattr(trainer, "rdrop", 0.0) > 0.0 else None
    tok_sum = torch.zeros((), device=dev, dtype=torch.int64)
    t0, tok0 = time.time(), 0
    accum = getattr(trainer, "accum_steps", 1) > 1
    for j, k in enumerate(order):
        if accum:           # the trainer closes a window at every accum_steps-th batch; the epoch's last batch closes a short one
            loss, b = trainer.step(indices[k], cut_a=cut is not None, rng=cut, last=True if j == len(order) - 1 else None)
        else:
            loss, b = trainer.step(indices[k], cut_a=cut is not None, rng=cut)
        # the step's loss is already divided by the token count of the step over ALL ranks (train.py:36; dp.py): weight it
        # with that same count; the ranks' sums add up to the epoch mean of the global batches
        n_glob = b._norms_global[0].to(torch.int64)
        loss_sum += loss * n_glob
        tok_sum += n_glob
        if kd_sum is not None:
            kd_sum += trainer.last_kd * n_glob
        if ul_sum is not None:
            ul_sum += trainer.last_ul * n_glob
        if rd_sum is not None:
            rd_sum += trainer.last_rd * n_glob
        if scst:
            rl_sum += torch.stack([trainer.last_reward, trainer.last_baseline])
        if (j + 1) % report_interval == 0 and rank == 0:
            ntok = int(tok_sum)
            dt = time.time() - t0
            print("Epoch: %d Step: %d Loss: %f Tokens per Sec: %f" % (epoch + 1, j + 1, float(loss), (ntok - tok0) / dt))
            t0, tok0 = time.time(), ntok
    if torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1:
        torch.distributed.all_reduce(loss_sum)
        if kd_sum is not None:
            torch.distributed.all_reduce(kd_sum)
        if ul_sum is not None:
            torch.distributed.all_reduce(ul_sum)
        if rd_sum is not None:
            torch.distributed.all_reduce(rd_sum)
    ntok = int(tok_sum)
    if rd_sum is not None and stats is not None:
        stats["rd"] = float(rd_sum) / max(1, ntok)
    if ul_sum is not None and stats is not None:
        stats["ul"] = float(ul_sum) / max(1, ntok)
    if kd_sum is not None and stats is not None:
        stats["kd"] = float(kd_sum) / max(1, ntok)
    if scst and stats is not None:
        stats["reward"], stats["baseline"] = (float(v) / max(1, len(order)) for v in rl_sum)
    return float(loss_sum) / max(1, ntok), ntok


def validate(corpus, indices, model, criterion, ae_ft, lam, cut=None):
    """train.py:201-210: the epoch loop with the model in eval() mode and no optimiser — mean loss per target token.  ``cut``:
    the --cut-a RandomState; the reference truncates validation answers too (train.py:30 passes cut_a to every run_epoch)."""
    from .data_handler import make_batch
    from .data_utils import SimpleLossCompute
    lc = SimpleLossCompute(model.generator, model.auto_encoder_generator, criterion, opt=None, l=lam, sync=False)
    was_training = model.training
    model.eval()
    total = torch.zeros((), device=corpus.device)
    tokens = torch.zeros((), device=corpus.device, dtype=torch.int64)
    with torch.no_grad():
        for ix in indices:
            b = make_batch(corpus, ix, 1, separate_caption=True, cut_a=cut is not None, rng=cut)
            out, ae_out = model.forward(b)
            ae_y = b.cap if ae_ft in ("caption", "summary") else b.query
            total += lc(out, b.trg_y, b.ntokens, ae_out, ae_y, (ae_y != 1).sum())
            tokens += b.ntokens
    model.train(was_training)
    return float(total) / max(1, int(tokens))


def global_norms(b, ae_y, sync):
    """[target tokens, auto-encoder tokens] of this step over ALL ranks (device tensor), and this rank's target tokens."""
    norms = torch.stack([b.ntokens, (ae_y != 1).sum()]).float()
    local_ntok = float(norms[0])
    if sync is not None and getattr(sync, "world", 1) > 1:
        sync.all_reduce_scalars(norms)
    return norms, local_ntok


def run_epoch(corpus, indices, model, loss_compute, ae_ft, epoch, report_interval, rank, rng, cut=None, distill=None, stats=None,
              unlikelihood=0.0):
    """train.py:23-50: shuffle the planned batches, assemble each on the device, forward, loss + backward + optimiser.
    Data parallel: the loss normalisers are the GLOBAL token counts of the step (all ranks' batches), so that the summed
    gradients are those of one rank on the concatenated batch (dp.py) — as the captured schedule does (TrainStep._norms).
    ``cut``: the --cut-a RandomState (None = no truncation).  Returns (mean loss per token, target tokens over all ranks).
    ``distill``: (teacher, alpha, temperature) — the teacher's rows are computed before the student's forward (train_step.teacher_rows);
    ``stats`` then receives "kd", this rank's mean distillation KL per token.  ``unlikelihood``: alpha of SimpleLossCompute.loss;
    ``stats`` then receives "ul", this rank's mean unlikelihood per token."""
    from .data_handler import make_batch
    from .train_step import teacher_rows
    order = list(range(len(indices)))
    rng.shuffle(order)
    t0, tokens, total_loss, total_tokens, global_tokens = time.time(), 0, 0.0, 0, 0
    sync = loss_compute.grad_sync
    kd_total = ul_total = 0.0
    for j, k in enumerate(order):
        b = make_batch(corpus, indices[k], 1, separate_caption=True, cut_a=cut is not None, rng=cut)
        kw = {}
        if distill is not None:
            kw = dict(teacher_logp=teacher_rows(distill[0], b), alpha=distill[1], temperature=distill[2])
        if unlikelihood > 0.0:
            kw = dict(unlikelihood=unlikelihood)
        out, ae_out = model.forward(b)
        ae_y = b.cap if ae_ft in ("caption", "summary") else b.query
        norms, local_ntok = global_norms(b, ae_y, sync)
        loss = loss_compute(out, b.trg_y, norms[0], ae_out, ae_y, norms[1], **kw)     # = normalised loss x global target tokens
        if distill is not None and loss_compute.last_kd_sum is not None:
            kd_total += float(loss_compute.last_kd_sum)
        if loss_compute.last_ul_sum is not None:
            ul_total += float(loss_compute.last_ul_sum)
        n_glob = float(norms[0])
        loss = loss * local_ntok / n_glob                                       # this rank's share, for the epoch mean below
        total_loss += loss
        total_tokens += int(b.ntokens)
        global_tokens += int(round(n_glob))
        tokens += int(b.ntokens)
        if (j + 1) % report_interval == 0 and rank == 0:
            dt = time.time() - t0
            print("Epoch: %d Step: %d Loss: %f Tokens per Sec: %f" % (epoch + 1, j + 1, loss / float(b.ntokens), tokens / dt))
            t0, tokens = time.time(), 0
    if distill is not None and stats is not None:
        stats["kd"] = kd_total / max(1, total_tokens)
    if unlikelihood > 0.0 and stats is not None:
        stats["ul"] = ul_total / max(1, total_tokens)
    return total_loss / max(1, total_tokens), global_tokens


def main(argv=None):
    args = parse(argv)
    logging.basicConfig(level=logging.DEBUG if args.verbose else logging.INFO, format="%(asctime)s %(levelname)s: %(message)s")
    cut_a = cut_a_applies(args)
    rank, world, local = dp.init_distributed()
    err = scst_flag_error(args, world) or clip_flag_error(args, world) or accum_flag_error(args, world) or sched_flag_error(args, world)
    if err:
        raise SystemExit("mtn_amd.train: " + err)
    local = local % torch.cuda.device_count()      # (several ranks may share a GPU in a gloo dry run)
    dev = torch.device("cuda", local)
    torch.cuda.set_device(dev)
    train_data = valid_data = vocab = None
    if args.train_set:
        from . import data_handler as dh
        sep_cap = bool(args.separate_caption) and args.include_caption != "none"
        logging.info("Extracting words from " + args.train_set)
        vocab = dh.get_vocabulary(args.train_set, include_caption=args.include_caption)
        kw = dict(include_caption=args.include_caption, separate_caption=bool(args.separate_caption), vocab=vocab,
                  max_history_length=args.max_history_length, merge_source=bool(args.merge_source))
        logging.info("Loading training data from " + args.train_set)
        train_data = dh.load(args.fea_type, args.train_path, args.train_set, **kw)
        if args.valid_set:
            logging.info("Loading validation data from " + args.valid_set)
            valid_data = dh.load(args.fea_type, args.valid_path or args.train_path, args.valid_set, **kw)
        if not sep_cap:
            raise SystemExit("mtn_amd.train: the model needs the caption as its own stream (--separate-caption 1 with "
                             "--include-caption caption|summary|caption,summary), as run.sh sets it; the reference crashes "
                             "without it too (mtn.py:52)")
        args.vocab_size = len(vocab)
        args.ft_sizes = dh.feature_shape(train_data)
        logging.info("Detected feature dims: %s  #vocab = %d", args.ft_sizes, len(vocab))
        if args.model and rank == 0:                                  # train.py:166-172
            import os
            import pickle
            os.makedirs(os.path.dirname(args.model) or ".", exist_ok=True)
            with open(args.model + ".conf", "wb") as f:
                pickle.dump((vocab, args), f, -1)
            with open(args.model + "_params.txt", "w") as f:
                for arg in vars(args):
                    f.write("{}={}\n".format(arg, getattr(args, arg)))
    torch.manual_seed(args.rand_seed)
    model = make_model(args.vocab_size, args.vocab_size, N=args.nb_blocks, d_model=args.d_model, d_ff=args.d_ff, h=args.att_h,
                       dropout=args.dropout, separate_his_embed=bool(args.separate_his_embed), separate_cap_embed=bool(args.separate_cap_embed),
                       ft_sizes=args.ft_sizes, diff_encoder=bool(args.diff_encoder), diff_embed=bool(args.diff_embed),
                       diff_gen=bool(args.diff_gen), auto_encoder_ft=args.auto_encoder_ft, compute_dtype=args.compute_dtype)
    model.to(dev).train()
    model.prepare()
    teacher = load_teacher(args, vocab, dev)
    distill = dict(teacher=teacher, distill_alpha=args.distill_alpha, distill_temperature=args.distill_temperature) if teacher is not None else {}
    sync = None
    if world > 1:
        sync = dp.GradSync(lambda: model.flat_buffers()[2])
        sync.broadcast_(model._flat)
        model._flat_version = -1
        model.prepare()
    if args.corpus_videos > 0 or train_data is not None:
        import random
        from .data_handler import DeviceCorpus, cut_a_stream, make_batch_indices
        from .data_utils import FusedAdam, LabelSmoothing, NoamOpt, SimpleLossCompute
        synthetic = train_data is None
        max_len = 256 if synthetic else args.max_length         # (run.sh passes 256, the parser's default is the reference's 20)
        data = (synthetic_corpus(args.corpus_videos, args.vocab_size, args.ft_sizes, args.rand_seed, max_answer=args.corpus_max_answer,
                                 max_question=args.corpus_max_question) if synthetic else train_data)
        indices, n_samples = make_batch_indices(data, batchsize=args.batch_size, max_length=max_len, separate_caption=True)  # train.py:126
        indices = indices[:len(indices) // world * world][rank::world]   # data parallel: equal shares of the planned batches (every
                                                                         # rank must issue the same number of gradient exchanges)
        corpus = DeviceCorpus(data, dev)
        logging.info("corpus: %d dialogs in %d batches, %.1f MB resident on the device", n_samples, len(indices), corpus.nbytes() / 1e6)
        rng = random.Random(args.rand_seed)
        # --cut-a: ONE stream for the run's training batches (in visiting order) and then each epoch's validation batches (in
        # plan order), as the reference's global np.random after np.random.seed(--rand-seed) (train.py:109); per rank
        cut = cut_a_stream(args.rand_seed, rank) if cut_a else None
        means = []
        scst = None
        if args.scst_samples:
            # the corpus' tokenised answers, uploaded once, are the reference corpus: rewards are on model token ids, item = QA id
            from .train_step import ScstConfig, corpus_reference
            longest = -(-int(corpus.host_tok["trg"][2].max()) // args.bucket) * args.bucket if args.scst_xe_weight > 0 else 0
            T = min(args.max_length, 129)                   # the metric kernels score sentences of at most 128 tokens
            scst = ScstConfig(samples=args.scst_samples, reward=args.scst_reward, baseline=args.scst_baseline, temperature=args.scst_temperature,
                              top_k=args.scst_top_k, top_p=args.scst_top_p, xe_weight=args.scst_xe_weight, max_length=T, sos=2, eos=3,
                              seed=args.rand_seed, refs=corpus_reference(corpus, min_len=max(T, longest)))
            if longest > 129:
                raise SystemExit("mtn_amd.train: --scst-xe-weight needs answers of at most 128 tokens (the metric kernels' longest sentence)")
            logging.info("self-critical training: %d samples per dialogue, reward %s, baseline %s, %d reference answers on the device",
                         scst.samples, scst.reward, scst.baseline, corpus.n_dialogs)
        accum = args.accum_steps > 1                          # (--eager then runs the trainer's steps eagerly, as under scst)
        sched = sched_config(args)                            # (likewise: the first pass and the mix belong to the trainer's step)
        rdrop = args.rdrop_alpha > 0.0                        # (likewise: the doubled batch belongs to the trainer's step)
        if args.eager and scst is None and not accum and sched is None and not rdrop:
            opt = NoamOpt(args.d_model, 1, args.warmup_steps, FusedAdam(model))
            if args.ema_decay:
                opt.optimizer.enable_ema(args.ema_decay)
            if args.clip_grad_norm:
                opt.optimizer.enable_clip(args.clip_grad_norm)
            lc = SimpleLossCompute(model.generator, model.auto_encoder_generator, LabelSmoothing(args.vocab_size, 1, 0.1), opt=opt,
                                   l=args.loss_l, grad_sync=sync)
        else:
            from .train_step import BucketedTrainer
            trainer = BucketedTrainer(model, corpus, args.vocab_size, pad=1, warmup=args.warmup_steps, lam=args.loss_l,
                                      bucket=args.bucket, grad_sync=sync, ema_decay=args.ema_decay, scst=scst,
                                      use_graph=not (args.eager and (scst is not None or accum or sched is not None or rdrop)),
                                      unlikelihood=args.unlikelihood_alpha, clip_grad_norm=args.clip_grad_norm, accum_steps=args.accum_steps,
                                      sched=sched, rdrop=args.rdrop_alpha, **distill)
        valid = None
        if args.valid_videos > 0 or valid_data is not None:
            vdata = valid_data if valid_data is not None else synthetic_corpus(args.valid_videos, args.vocab_size, args.ft_sizes, args.rand_seed + 1000)
            vidx, vn = make_batch_indices(vdata, batchsize=args.batch_size, max_length=max_len, separate_caption=True)
            valid = (DeviceCorpus(vdata, dev), vidx)
            logging.info("#validation sample = %d  #validation batch = %d", vn, len(vidx))
        min_valid = min_valid_ema = 1.0e10
        graphed = not args.eager or scst is not None or accum or sched is not None or rdrop  # (then --eager: the trainer's steps, run eagerly)
        the_opt = trainer.opt if graphed else opt
        if args.resume:
            model.load_state_dict(torch.load(args.resume + ".pth.tar", map_location=dev), strict=False)
            model.prepare()
            the_opt.load_state_dict(torch.load(args.resume + "_opt.pth.tar"))
            logging.info("resumed from %s at optimiser step %d", args.resume, the_opt.step_count())
            if scst is not None:
                trainer.rl_steps = the_opt.step_count()        # the draws go on where the resumed run's would
        for epoch in range(args.num_epochs):
            stats = {}
            if not graphed:
                mean, ntok = run_epoch(corpus, indices, model, lc, args.auto_encoder_ft, epoch, args.report_interval, rank, rng, cut,
                                       distill=(teacher, args.distill_alpha, args.distill_temperature) if teacher is not None else None, stats=stats,
                                       unlikelihood=args.unlikelihood_alpha)
            else:
                seen = (trainer.updates, trainer.micro_steps)
                mean, ntok = run_epoch_graphed(trainer, indices, epoch, args.report_interval, rank, rng, cut, stats=stats)
                if accum and rank == 0:
                    print("epoch %d optimiser updates: %d over %d batches" % (epoch + 1, trainer.updates - seen[0], trainer.micro_steps - seen[1]))
            means.append(mean)
            if rank == 0:
                logging.info("epoch %d: %d target tokens trained%s", epoch + 1, ntok, " (answers cut at random)" if cut_a else "")
            if rank == 0:
                print("epoch %d mean train loss per token: %f" % (epoch + 1, mean))
                if "kd" in stats:
                    print("epoch %d mean distillation KL per token: %f" % (epoch + 1, stats["kd"]))
                if "ul" in stats:
                    print("epoch %d mean unlikelihood per token: %f" % (epoch + 1, stats["ul"]))
                if "rd" in stats:
                    print("epoch %d mean R-Drop divergence per token: %f" % (epoch + 1, stats["rd"]))
                if "reward" in stats:
                    print("epoch %d mean reward: %f mean baseline: %f" % (epoch + 1, stats["reward"], stats["baseline"]))
            if args.clip_grad_norm:
                clip_epoch_report(the_opt.optimizer, epoch, rank)
            if sched is not None and trainer.sched_stats is not None:
                sched_epoch_report(sched, trainer.sched_stats, the_opt.step_count(), epoch, rank)
            if args.model:
                # EVERY rank builds the optimiser state: with the sharded optimiser (dp.ShardedOptimizerSync) a rank holds the
                # Adam moments of its shards only (and, with the compute-dtype gather, the current fp32 masters of its shards
                # only) and state_dict() gathers them with collectives; rank 0 alone writes the files
                opt_state = the_opt.state_dict()
                model_state = model.state_dict()              # (collective under the compute-dtype gather: fp32 masters)
                if rank == 0:
                    torch.save(model_state, f"{args.model}_{epoch + 1}.pth.tar")
                    torch.save(opt_state, f"{args.model}_{epoch + 1}_opt.pth.tar")
                del opt_state, model_state
                if args.ema_decay:
                    ema_state = the_opt.optimizer.ema_state_dict()       # (collective: every rank)
                    if rank == 0:
                        torch.save(ema_state, f"{args.model}_{epoch + 1}_ema.pth.tar")
                    del ema_state
            if valid is not None:
                best_state = model.state_dict() if args.model else None    # (collective) written by rank 0 alone if validation improves
                from .data_utils import LabelSmoothing as _LS
                # --cut-a: the second validation sees the truncations of the first and takes no draw from the run's stream
                cut_ema = copy.deepcopy(cut) if args.ema_decay else None
                vloss = validate(valid[0], valid[1], model, _LS(args.vocab_size, 1, 0.1), args.auto_encoder_ft, args.loss_l, cut)
                if rank == 0:
                    print("epoch: %d validation loss: %f" % (epoch + 1, vloss))          # train.py:210
                    if vloss < min_valid:
                        print("validation loss reduced %.4f -> %.4f" % (min_valid, vloss))
                        min_valid = vloss
                        if args.model:
                            torch.save(best_state, f"{args.model}_best.pth.tar")
                del best_state
                if args.ema_decay:
                    # the same validation under the averaged weights, with a minimum of its own; <model>_best stays chosen by the raw weights
                    best_ema = the_opt.optimizer.ema_state_dict() if args.model else None      # (collective)
                    with the_opt.optimizer.averaged_weights():
                        vloss_ema = validate(valid[0], valid[1], model, _LS(args.vocab_size, 1, 0.1), args.auto_encoder_ft, args.loss_l, cut_ema)
                    if rank == 0:
                        print("epoch: %d validation loss (averaged weights): %f" % (epoch + 1, vloss_ema))
                        if vloss_ema < min_valid_ema:
                            print("validation loss (averaged weights) reduced %.4f -> %.4f" % (min_valid_ema, vloss_ema))
                            min_valid_ema = vloss_ema
                            if args.model:
                                torch.save(best_ema, f"{args.model}_best_ema.pth.tar")
                    del best_ema
        if world > 1:
            torch.distributed.destroy_process_group()
        return means
    Q, H, C, T, V = args.lens
    batch = synthetic_batch(args.vocab_size, args.batch_size, Q, H, C, T, [V] * len(args.ft_sizes), args.ft_sizes, device=dev, seed=1 + rank)
    step = TrainStep(model, batch, args.vocab_size, pad=1, warmup=args.warmup_steps, lam=args.loss_l, grad_sync=sync, ema_decay=args.ema_decay,
                     unlikelihood=args.unlikelihood_alpha, clip_grad_norm=args.clip_grad_norm, accumulate=args.accum_steps > 1,
                     sched=sched_config(args), rdrop=args.rdrop_alpha, **distill)
    ntok = int(step.batch.ntokens) * world             # (R-Drop: the step's own doubled batch, both passes' tokens)
    K = args.accum_steps
    for epoch in range(args.num_epochs):
        t0, tokens = time.time(), 0
        kd_sum = torch.zeros((), device=dev) if teacher is not None else None
        ul_sum = torch.zeros((), device=dev) if args.unlikelihood_alpha > 0.0 else None
        rd_sum = torch.zeros((), device=dev) if args.rdrop_alpha > 0.0 else None
        for j in range(args.steps_per_epoch):
            # --accum-steps K: a call is one micro-step on the batch; every K-th one, and the epoch's last, closes the window and updates
            loss = step() if K == 1 else step((j + 1) % K == 0 or j == args.steps_per_epoch - 1)
            tokens += ntok
            if ul_sum is not None:
                ul_sum += step.last_ul
            if rd_sum is not None:
                rd_sum += step.last_rd
            if kd_sum is not None:
                kd_sum += step.last_kd
            if (j + 1) % args.report_interval == 0 and rank == 0:
                torch.cuda.synchronize()
                dt = time.time() - t0
                print("Epoch: %d Step: %d Loss: %f Tokens per Sec: %f" % (epoch + 1, j + 1, float(loss), tokens / dt))   # train.py:46
                t0, tokens = time.time(), 0
        if kd_sum is not None:
            if world > 1:
                torch.distributed.all_reduce(kd_sum)
            if rank == 0:
                print("epoch %d mean distillation KL per token: %f" % (epoch + 1, float(kd_sum) / max(1, args.steps_per_epoch)))
        if ul_sum is not None:
            if world > 1:
                torch.distributed.all_reduce(ul_sum)
            if rank == 0:
                print("epoch %d mean unlikelihood per token: %f" % (epoch + 1, float(ul_sum) / max(1, args.steps_per_epoch)))
        if rd_sum is not None:
            if world > 1:
                torch.distributed.all_reduce(rd_sum)
            if rank == 0:
                print("epoch %d mean R-Drop divergence per token: %f" % (epoch + 1, float(rd_sum) / max(1, args.steps_per_epoch)))
        if K > 1 and rank == 0:
            print("epoch %d optimiser updates: %d over %d batches" % (epoch + 1, -(-args.steps_per_epoch // K), args.steps_per_epoch))
        if args.clip_grad_norm:
            clip_epoch_report(step.opt.optimizer, epoch, rank)
        if step.sched is not None:
            sched_epoch_report(step.sched, step.sched_stats, step.opt.step_count(), epoch, rank)
        if args.model:
            model_state = model.state_dict()      # every rank: under the sharded optimiser's compute-dtype gather this gathers the fp32
            if rank == 0:                         # masters of the other ranks' shards (a collective) — rank 0 alone writes
                torch.save(model_state, f"{args.model}_{epoch + 1}.pth.tar")      # reference key schema
            del model_state
            if args.ema_decay:
                ema_state = step.opt.optimizer.ema_state_dict()
                if rank == 0:
                    torch.save(ema_state, f"{args.model}_{epoch + 1}_ema.pth.tar")
                del ema_state
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
