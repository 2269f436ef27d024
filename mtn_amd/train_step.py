"""One training step of the reference's batch loop (train.py:29-40 + data_utils.py:123-156) as a replayable unit:
zero glue grads -> forward -> generator + label-smoothed loss -> backward -> [gradient all-reduce] -> fused Noam/Adam.

On one GPU the whole step is captured into a single hipGraph (≈460 short kernels: launch-bound if driven from
Python).  With data parallelism the backward pass is cut at the decoder-layer boundaries (model.forward_segmented) and
the step becomes N+3 hipGraphs — [forward + loss + top layer] [layer N-2] … [layer 0] [encoder side] [Adam] — with the RCCL
all-reduce of each finished gradient slice (one layer = 17 M floats = 67 MB at cfg2) launched eagerly, asynchronously,
right after the graph that produced it: the exchange of layer k runs on RCCL's stream while layer k-1's backward runs.
Collectives stay out of graph capture on purpose.  ``overlap=False`` (or MTN_DP_OVERLAP=0) keeps
the simpler schedule: one graph for forward+backward, the whole-buffer all-reduce, one graph for Adam.
"""
from __future__ import annotations

import math
import os
from typing import Callable, NamedTuple, Optional

import torch

from . import lib as L
from .data_utils import FusedAdam, LabelSmoothing, NoamOpt, SimpleLossCompute

# Stream capture checks "potentially unsafe" runtime calls; in the default (global) mode a call from ANY thread invalidates the
# capture — and ProcessGroupNCCL's watchdog thread polls its work events (hipEventQuery) for a while after every collective, so a
# step captured right after an exchange (a new batch shape in BucketedTrainer, the fallback schedule, a second TrainStep) died
# with hipErrorStreamCaptureInvalidated (seen on hardware: tools/dp_rccl_probe.py, round 3).  Only this thread's calls matter here:
# the kernels come from this thread and from autograd's device thread, both onto the capturing stream.
CAPTURE_MODE = os.environ.get("MTN_CAPTURE_MODE", "thread_local")
_CUT_GACC = True      # gradients across a layer cut meet in the memory-gradient buffer (no autograd add)


def teacher_members(teacher):
    """(active members, weights or None, mode) of a teacher: a model is an ensemble of one (the combining kernel normalises)."""
    from .decode import Ensemble
    if isinstance(teacher, Ensemble):
        return list(teacher.active), list(teacher.active_weights), teacher.mode
    if isinstance(teacher, torch.nn.Module) and hasattr(teacher, "generator") and hasattr(teacher, "forward"):
        return [teacher], None, "prob"
    raise ValueError("distillation: teacher is a model or a decode.Ensemble")


def teacher_rows(teacher, batch, out=None):
    """The teacher's next-token log-probabilities for every target position of ``batch``, (rows, V) fp32: each active member's eval()
    forward under no_grad, its generator logits, then ONE ops.ensemble_rows launch over the members.  Nothing is left behind:
    no dropout stream is advanced, nothing enters a parameter-gradient queue, every forward flushes its rider work."""
    from . import ops
    members, weights, mode = teacher_members(teacher)
    rows = []
    with torch.no_grad():
        for m in members:
            if m.training:
                m.eval()
            o, _ = m.forward(batch)
            z = m.generator.logits(o)
            rows.append(z.reshape(-1, z.size(-1)))
        return ops.ensemble_rows(rows, weights, mode, out=out)


class ScstConfig:
    """Self-critical sequence training (Rennie et al. 2017) for TrainStep(scst=...): ``samples`` S responses per dialogue are drawn from
    the current weights (temperature / top_k / top_p as decode.sample_decode_many takes them), scored against the reference corpus
    ``refs`` = (ref (Qc, R, L) int32, ref_len (Qc, R) int32, n_ref (Qc,) int32) on the device by ``reward`` ("cider" | "rouge"), and
    trained on with the row weight -(reward - baseline): ``baseline`` "mean" = the leave-one-out mean of the dialogue's other samples
    (Luo 2020), "greedy" = the reward of the greedy response.  ``xe_weight`` > 0 adds the gold answer as one more row per dialogue with
    that constant weight.  Every target row has ``max_length`` positions; sampled and gold rows are -log p(target) (smoothing 0).
    ``sos`` / ``eos``: the start and end symbols; ``seed``: of the first step's draws, advanced by one per step."""

    def __init__(self, samples: int = 2, reward: str = "cider", baseline: str = "mean", temperature: float = 1.0, top_k: int = 0,
                 top_p: float = 1.0, xe_weight: float = 0.0, max_length: int = 20, sos: int = 2, eos: int = 3, seed: int = 0, refs=None):
        if not 2 <= int(samples) <= 16:
            raise ValueError("scst: 2 to 16 samples per dialogue")
        if reward not in ("cider", "rouge") or baseline not in ("mean", "greedy"):
            raise ValueError("scst: reward is cider or rouge, baseline is mean or greedy")
        if not (float(temperature) >= 0.0 and 0.0 < float(top_p) <= 1.0 and int(top_k) >= 0 and float(xe_weight) >= 0.0 and int(max_length) >= 2):
            raise ValueError("scst: temperature >= 0, top_k >= 0, 0 < top_p <= 1, xe_weight >= 0, max_length >= 2")
        self.samples, self.reward, self.baseline = int(samples), reward, baseline
        self.temperature, self.top_k, self.top_p = float(temperature), int(top_k), float(top_p)
        self.xe_weight, self.max_length, self.sos, self.eos, self.seed, self.refs = float(xe_weight), int(max_length), int(sos), int(eos), int(seed), refs
        self._table = None               # the corpus' document-frequency table, built once and shared by every step over this config

    def with_max_length(self, max_length: int):
        """A copy for another number of target positions; the reference corpus and its table are shared."""
        import copy
        c = copy.copy(self)
        c.max_length = int(max_length)
        return c


class SchedConfig:
    """Scheduled sampling in its two-pass, parallel form (Mihaylova & Martins 2019; Duckworth et al. 2019) for TrainStep(sched=...):
    ahead of every training forward the model runs once under eval() / no_grad over the gold decoder inputs, and one mtn_sched_mix
    launch (include/mtn_hip.h gives the formulas) replaces a fraction p of the decoder's INPUT tokens by that pass's predictions; the
    step then trains on the mixed inputs against the gold targets.  p = ``prob`` * min(1, max(0, step - ``start``) / ``ramp``) with step
    the optimiser's update count, read on the device (``ramp`` 0: ``prob`` from ``start`` on).  ``pick``: "argmax", or "sample" (a
    Gumbel-max draw from softmax(logits / ``temperature``)).  ``banned``: up to 4 ids never picked (<sos>; <pad> is always excluded).
    ``seed``: of the counter hash, to which the device adds the step."""

    def __init__(self, prob: float, start: int = 0, ramp: int = 0, pick: str = "argmax", temperature: float = 1.0, seed: int = 0,
                 banned=(2,)):
        prob, temperature = float(prob), float(temperature)
        if not 0.0 < prob <= 1.0:
            raise ValueError("sched: 0 < prob <= 1")
        if int(start) != start or int(ramp) != ramp or not (0 <= int(start) < 2 ** 31 and 0 <= int(ramp) < 2 ** 31):
            raise ValueError("sched: start and ramp are integers >= 0 (update counts)")
        if pick not in ("argmax", "sample"):
            raise ValueError("sched: pick is argmax or sample")
        if not (0.0 < temperature < float("inf")):
            raise ValueError("sched: temperature is finite and > 0")
        if int(seed) != seed or not 0 <= int(seed) < 2 ** 62:
            raise ValueError("sched: seed is an integer in [0, 2^62)")
        banned = tuple(int(b) for b in banned)
        if len(banned) > 4 or any(b < 0 for b in banned):
            raise ValueError("sched: at most 4 banned token ids, none negative")
        self.prob, self.start, self.ramp, self.pick = prob, int(start), int(ramp), pick
        self.temperature, self.seed, self.banned = temperature, int(seed), banned

    def prob_at(self, step: int) -> float:
        """p at update count ``step``, in the kernel's fp32 arithmetic."""
        import numpy as np
        f = np.float32
        if self.ramp == 0:
            return float(f(self.prob)) if step >= self.start else 0.0
        d = max(f(0.0), f(step) - f(self.start))
        return float(f(self.prob) * min(f(1.0), f(d / f(self.ramp))))


_NAMES = {"teacher": "a teacher (distillation)", "scst": "scst", "unlikelihood": "unlikelihood", "sched": "sched (scheduled sampling)",
          "rdrop": "rdrop"}


def check_objectives(who, *, teacher=None, distill_alpha=0.5, distill_temperature=1.0, scst=None, unlikelihood=0.0, rdrop=0.0, sched=None,
                     clip_grad_norm=0.0, clipping=False, accumulating=False, grad_sync=None):
    """What a step's keywords may hold and which of them combine, for TrainStep and BucketedTrainer (``who``: the message's prefix).
    Conflicts are reported in the order of the lines below.  ``clipping`` / ``accumulating``: what the step's optimiser has enabled."""
    def fail(msg):
        raise ValueError("%s: %s" % (who, msg))

    def alpha(name, a):
        if not (a >= 0.0 and math.isfinite(a)):
            fail("%s is finite and >= 0" % name)
        return a > 0.0

    on = dict(teacher=teacher is not None, scst=scst is not None, sched=sched is not None, unlikelihood=float(unlikelihood) > 0.0)

    def alone(name, *others):
        for o in others:
            if on[o]:
                fail("%s does not combine with %s" % (_NAMES[name], _NAMES[o]))

    if alpha("rdrop", float(rdrop)):
        alone("rdrop", "teacher", "scst", "unlikelihood", "sched")      # (sched keys rows by batch index: the halves would see different inputs)
    if on["sched"]:
        alone("sched", "teacher", "scst")                               # (a teacher would have to see the mixed inputs)
    if not float(clip_grad_norm) >= 0.0:                                # (nan fails the comparison)
        fail("clip_grad_norm is 0 (off) or > 0 (inf allowed)")
    if alpha("unlikelihood", float(unlikelihood)):
        alone("unlikelihood", "teacher", "scst")
    if on["teacher"]:
        if not (0.0 <= float(distill_alpha) <= 1.0):
            fail("distill_alpha in [0, 1]")
        if not (0.0 < float(distill_temperature) < float("inf")):
            fail("distill_temperature is finite and > 0")
    if on["scst"] and accumulating:
        fail("scst does not combine with gradient accumulation: rl_step is one update per call")
    if on["scst"] and (on["teacher"] or grad_sync is not None):
        fail("scst does not combine with a teacher (distillation) or with data parallelism")
    if grad_sync is not None and os.environ.get("MTN_DP_SHARDED", "0") != "0":      # asked for explicitly: the default gives way instead
        for flag, what, why in ((clipping, "gradient clipping", "the norm needs every slice reduced before any shard is updated"),
                                (accumulating, "gradient accumulation", "the update runs once per window, from the whole window gradient")):
            if flag:
                fail("%s does not combine with the sharded data-parallel optimiser (MTN_DP_SHARDED): %s; leave MTN_DP_SHARDED unset or 0"
                     % (what, why))


class _Stage(NamedTuple):
    """One stage of a step's schedule.  ``unit``: a callable whose launches are ONE graph of the captured step (None: nothing to capture);
    ``after``: what runs eagerly behind it, captured or not — the accumulate launch, a gradient exchange; ``closing``: the stage runs
    only in the call that closes an accumulation window."""
    unit: Optional[Callable] = None
    after: Optional[Callable] = None
    closing: bool = False


class TrainStep:
    def __init__(self, model, batch, vocab: int, pad: int = 1, warmup: int = 4000, factor: float = 1.0, lam: float = 1.0,
                 smoothing: float = 0.1, grad_sync=None, use_graph: bool = True, overlap: Optional[bool] = None, opt=None,
                 dynamic_norms: bool = False, fuse_optimizer: Optional[bool] = None, teacher=None, distill_alpha: float = 0.5,
                 distill_temperature: float = 1.0, ema_decay: float = 0.0, scst: Optional[ScstConfig] = None, unlikelihood: float = 0.0,
                 clip_grad_norm: float = 0.0, accumulate: bool = False, sched: Optional[SchedConfig] = None, rdrop: float = 0.0,
                 rdrop_paired: bool = False):
        """Which of the keywords below combine, and what they may hold, is check_objectives' to say.
        ``opt``: share an existing NoamOpt (several TrainSteps over one model, e.g. one per batch shape).
        ``dynamic_norms``: the batch tensors are refilled in place between steps, so the loss normalisers (token counts,
        train.py:35-39) are recomputed from them inside the step instead of once at construction.
        ``fuse_optimizer``: None = on one rank, apply Adam to the sublayer weight matrices inside their parameter-gradient
        GEMMs (FusedAdam.fuse_into_backward; those gradients are then never written to ``.grad``); False = always the
        separate optimiser pass (gradients of every parameter are left in ``.grad`` after the step).
        ``teacher``: word-level knowledge distillation — a frozen model, or a decode.Ensemble of them, on the student's device and
        with its vocabulary size.  Inside the step (and its captured graph) every active member runs an eval() forward on the step's
        batch under no_grad, the members' generator logits are combined by ops.ensemble_rows into one row of log-probabilities
        per target position, and the MAIN decoder stream's loss becomes (1 - distill_alpha) * label-smoothed KL + distill_alpha *
        T^2 * KL(teacher_T || student_T) (csrc/losshead.hip; the auto-encoder streams keep the plain loss).  The teacher pass runs
        to completion before the student's forward starts and leaves nothing behind, so with distill_alpha == 0 the step is the
        undistilled step bit for bit.  ``last_kd``: device scalar, the step's summed row KL over its target-token normaliser.
        ``ema_decay``: > 0 = the optimiser built here keeps an exponential moving average of the weights (FusedAdam.enable_ema); a
        shared ``opt`` keeps whatever its owner enabled.
        ``scst``: self-critical sequence training (ScstConfig) on ONE rank, without a teacher.  ``batch`` is then the SOURCE of B
        dialogues (its answers are the gold rows); the step trains on a static batch of its own (``self.batch``: B * S sampled rows
        d * S + s, then B gold rows when xe_weight > 0, max_length target positions each).  ``rl_step(items)`` is one step: the
        sampling search under eval() / no_grad on the current weights, the assemble, reward and advantage launches (csrc/scst.hip),
        the source's encoder-side tensors replicated into the static batch, then the (captured) forward, weighted loss head
        (mtn_wlosshead_fwd / _bwd), backward and optimiser.  The search reads the drawn tokens once per position, as
        decode.sample_decode_many does on the launch-per-sublayer pass; from its last token to the optimiser nothing is read on the
        host.  The sampling pass reads the COMPUTE-DTYPE copies of the weights (the matrices' bf16 images and the generator's): the
        optimiser of the previous step rewrites them with the masters (FusedAdam writes p_lp next to p), and rl_step calls
        model.prepare() before the search, which casts whatever a load_state_dict / EMA swap changed behind the optimiser's back.
        The main stream's normaliser is the count of non-<pad> SAMPLED targets, recomputed inside the step (``dynamic_norms``), so the
        learning-rate scale is cross-entropy's; the auto-encoder streams keep the plain loss, at ``smoothing``, which the main stream
        does not use under scst (its rows are -log p(target): smoothing 0).  ``last_reward`` / ``last_baseline``:
        device scalars (float64), the step's mean reward and mean baseline.  ``load_rows(trg, trg_y, weights)``: the test entry that
        puts fixed rows in the place of the samples.
        ``unlikelihood``: alpha of token-level unlikelihood training (Welleck et al. 2019) on the MAIN decoder stream: its loss becomes
        label-smoothed KL + alpha * sum over each target row of -log(clamp(1 - p_c, 1e-5)) over the set of its sequence's earlier targets
        (mtn_ulosshead_fwd / _bwd in the place of the two loss-head launches, inside the captured graph; the head is local to the rank, so
        data parallelism needs nothing new).  0 = the plain step, launch for launch and bit for bit.  ``last_ul``: device scalar, the
        step's summed ul over its target-token normaliser.
        ``clip_grad_norm``: C > 0 (inf allowed: measure, never clip) = the optimiser built here clips the gradient's global L2 norm at C
        as torch.nn.utils.clip_grad_norm_ does (FusedAdam.enable_clip: mtn_grad_sumsq + mtn_clip_scale ahead of mtn_adam_step, the
        coefficient never leaves the device); a shared ``opt`` keeps whatever its owner enabled.  0 = off: the step is what it is
        without the keyword, launch for launch.  Adam is not linear in g, so a clipped step takes the separate-optimiser path
        (``fuse_optimizer`` = False) in every schedule — eager, the one-graph capture, rl_step under scst — and pays for the gradient's
        HBM round trip.  Data parallelism uses the all-reduce scheme with clipping on (the layer-segmented overlap stays): after the
        exchange every rank holds the whole reduced gradient and computes the same norm bits with no further collective.
        ``last_grad_norm``: device double, the norm of the step just run (None when clipping is off).
        ``accumulate``: gradient accumulation over a window of micro-batches — the optimiser built here keeps a second flat fp32 buffer
        (FusedAdam.enable_accumulation; a shared ``opt`` keeps whatever its owner enabled) and ``__call__(last)`` is one MICRO-step:
        today's forward, loss and backward, normalised by its own token counts, then one mtn_grad_accum launch weighted by the
        micro-step's target-token count over all ranks (``_norms[0]``, a device float).  Weights do not move inside a window; the call
        with ``last`` true closes it: the window's gradient G = (sum_k w_k g_k) / (sum_k w_k) is then in the gradient buffer and the
        exchange, Noam tick, clipping, Adam and EMA run once, on G (the step count counts windows).  G is the gradient of the
        token-weighted mean of the micro-steps' losses: the concatenated batch's gradient for the main stream, and for the
        auto-encoder streams too when the micro-batches share their query-to-target token ratio (otherwise a micro-batch's
        auto-encoder term carries w_k / sum w, not its share of the query tokens).  A window of one launches nothing new: it is the
        ``fuse_optimizer`` = False step bit for bit.  The captured form is a forward/backward graph and an optimiser graph with the
        accumulate launch (and the exchange) between the replays; nothing in a window synchronises with the host.  The returned
        loss is the micro-step's own.  Data parallelism: the whole-buffer, non-overlapped all-reduce, once per window, after the
        closing launch.  With clipping on one rank the closing launch also writes the partials of G's sum of squares and the update
        skips its mtn_grad_sumsq launch.
        ``sched``: scheduled sampling (SchedConfig).  Inside the step (and its captured graph), before the training forward, the student
        itself runs an eval() forward on the gold batch under no_grad, its generator logits go through one mtn_sched_mix launch into
        ``sched_mixed`` (allocated once), and the training forward reads a shallow copy of the batch whose ``trg`` is that buffer:
        ``trg_y``, the masks and the normalisers are the gold batch's (the mix never writes <pad> and never changes a <pad> position).
        The first pass leaves nothing behind and no gradient flows through it.  ``sched_keys`` (B,) int64 name the rows to the counter
        hash: rank * B + b unless the caller refills them (BucketedTrainer: the batch's QA ids); the step word is the optimiser's
        update count on the device, so every replay draws anew, a resumed run continues the stream, and the micro-steps of an
        accumulation window share it (on a fixed batch they repeat their draws).  ``sched_stats`` (3,) int64 on the device counts
        [eligible, replaced, replaced with another token than gold] until the caller zeroes it.  None = off: nothing is allocated or
        launched.
        ``rdrop``: alpha of R-Drop (Liang et al. 2021) on the MAIN decoder stream.  ``batch`` is then the SOURCE of B dialogues and the
        step trains on a static batch of its own (``self.batch``) of 2 B rows, rows b and B + b the same dialogue: a dropout site's
        keep-mask is a counter hash of (seed, salt, flat element index), so the two copies draw different masks in ONE forward pass.
        The refill is device copies at the head of the step (one copy per tensor that writes both halves, the masks' kernel images included), captured
        with it, with no host read: a caller that refills the source in place (``dynamic_norms``) keeps working.  The loss head is
        mtn_rlosshead_fwd / _bwd (csrc/losshead.hip; include/mtn_hip.h gives the formulas) in the place of the two loss-head launches:
        loss = the plain loss of the doubled batch (the mean of the two passes' label-smoothed losses: the normaliser counts both
        passes' tokens) + rdrop * ``last_rd``, ``last_rd`` = the device scalar sum_rows rd / ``_norms[0]`` = (KL(p || q) + KL(q || p)) / 4
        per original target token; the auto-encoder streams keep the plain loss.  The head is local to the rank, so data
        parallelism needs nothing new.  ``rdrop_paired``: ``batch`` already holds 2 N rows in pair layout and is used as it is (checked
        once: trg_y[:N] == trg_y[N:]).  0 = off: nothing is allocated or launched, the step is the plain step launch for launch and bit
        for bit.  Combines with clip_grad_norm, ema_decay, accumulate, both optimiser paths, graph and eager and both data-parallel
        schedules."""
        shared = None if opt is None else opt.optimizer
        check_objectives("TrainStep", teacher=teacher, distill_alpha=distill_alpha, distill_temperature=distill_temperature, scst=scst,
                         unlikelihood=unlikelihood, rdrop=rdrop, sched=sched, clip_grad_norm=clip_grad_norm, grad_sync=grad_sync,
                         clipping=bool(clip_grad_norm) if shared is None else getattr(shared, "clip_max_norm", None) is not None,
                         accumulating=bool(accumulate) or getattr(shared, "accum", None) is not None)
        self.model, self.batch = model, batch
        self.rdrop, self.last_rd, self._rd_src = float(rdrop), None, None
        if self.rdrop > 0.0:
            if rdrop_paired:
                self._check_paired(batch)
            else:
                self._init_rdrop(batch, pad)
                batch = self.batch
        self.sched, self.scst = sched, scst
        self.unlikelihood, self.last_ul = float(unlikelihood), None
        self._init_teacher(teacher, distill_alpha, distill_temperature, vocab)
        if scst is not None:
            self._init_scst(batch, pad)
            batch, dynamic_norms = self.batch, True
        if opt is None:
            opt = NoamOpt(model.decoder.layers[0].size, factor, warmup, FusedAdam(model))
            if ema_decay:
                opt.optimizer.enable_ema(ema_decay)
            if clip_grad_norm:
                opt.optimizer.enable_clip(clip_grad_norm)
            if accumulate:
                opt.optimizer.enable_accumulation()
        self.opt = opt
        self.clipping = getattr(opt.optimizer, "clip_max_norm", None) is not None
        self.accumulating = getattr(opt.optimizer, "accum", None) is not None
        self.dynamic_norms = dynamic_norms
        self.crit = LabelSmoothing(vocab, pad, smoothing)
        self.lc = SimpleLossCompute(model.generator, model.auto_encoder_generator, self.crit, opt=None, l=lam, sync=False)
        self.grad_sync = grad_sync
        self.pad = pad
        self.use_graph = use_graph
        self._g_fb = self._g_opt = self._replays = None
        self._loss = None
        self._closing = True
        # the main stream's objective as SimpleLossCompute.loss keywords (the teacher's rows join them per step), and the pair
        # (attribute here, the loss computer's row sum) behind last_kd / last_ul / last_rd
        if scst is not None:
            self._loss_kw, self._last = dict(row_weights=self._roww, smoothing=0.0), None
        elif self.rdrop > 0.0:
            self._loss_kw, self._last = dict(rdrop=self.rdrop), ("last_rd", "last_rd_sum")
        elif self.unlikelihood > 0.0:
            self._loss_kw, self._last = dict(unlikelihood=self.unlikelihood), ("last_ul", "last_ul_sum")
        elif teacher is not None:
            self._loss_kw, self._last = dict(alpha=self.distill_alpha, temperature=self.distill_temperature), ("last_kd", "last_kd_sum")
        else:
            self._loss_kw, self._last = {}, None
        if overlap is None:
            overlap = os.environ.get("MTN_DP_OVERLAP", "1") != "0"
        self.overlap = bool(overlap) and grad_sync is not None and not self.accumulating     # (accumulation: the whole-buffer exchange)
        # data parallel: reduce-scatter + optimiser on this rank's shard + all-gather of the master weights
        # (dp.ShardedOptimizerSync) instead of all-reduce + the full optimiser pass on every rank; MTN_DP_SHARDED=0 = the latter
        self.sharded = None
        if (grad_sync is not None and not self.clipping and not self.accumulating and os.environ.get("MTN_DP_SHARDED", "1") != "0"
                and hasattr(self.opt.optimizer, "step_range")):
            from .dp import ShardedOptimizerSync
            if getattr(grad_sync, "compress", False):
                raise ValueError("bf16 gradient compression applies to the all-reduce scheme only (MTN_DP_SHARDED=0): the sharded "
                                 "optimiser reduce-scatters the fp32 gradient in place")
            adam = self.opt.optimizer
            group = getattr(grad_sync, "group", None)
            sh = getattr(adam, "_sharded", None)          # ONE exchange object per optimiser: every TrainStep over it (one per
            if sh is None or sh.group is not group:       # batch shape, BucketedTrainer) shares the shard ownership and the
                sh = ShardedOptimizerSync(lambda: model.flat_buffers()[0], lambda: model.flat_buffers()[2], adam.step_range, group=group,
                                          force=getattr(grad_sync, "force", None),
                                          lp_fn=lambda: model.flat_buffers()[1], update_lp=getattr(adam, "step_range_lp", None))
                adam._sharded = sh                        # slice set that state_dict()'s gather walks
                # nobody may read the fp32 masters whole while foreign shards are stale (compute-dtype gather):
                # model.state_dict() and model.prepare() bring them up to date through this hook (a collective)
                model._master_sync = adam.gather_masters
            self.sharded = sh
        self._g_seg = None
        self._st = None
        self._g_opt_sumsq = None                 # accumulation with clipping: the optimiser graph that reads the closing launch's partials
        self._fuse_opt = False if fuse_optimizer is False or self.accumulating else None
        ae_y = batch.cap if model.auto_encoder_ft in ("caption", "summary") else batch.query
        self._ae_y = ae_y
        # loss normalisers (train.py:35-39).  Under DP they are all-reduced ONCE here for a static batch so that
        # N ranks x local batch == one rank x concatenated batch.
        self._norms = torch.stack([batch.ntokens, (ae_y != pad).sum()]).float()
        if grad_sync is not None:
            grad_sync.all_reduce_scalars(self._norms)
        self._init_sched()

    @property
    def last_grad_norm(self):
        return self.opt.optimizer.clip_norm if self.clipping else None

    # ---- pieces
    def local_norms(self):
        b = self.batch
        if self._rd_src is not None:         # the doubled batch's counts, from the source: right before the step's refill too
            src = self._rd_src
            ae_y = src.cap if self.model.auto_encoder_ft in ("caption", "summary") else src.query
            return 2.0 * torch.stack([(src.trg_y != self.pad).sum(), (ae_y != self.pad).sum()]).float()
        if self.scst is not None:            # the sampled rows alone: gold rows ride on the same normaliser
            return torch.stack([(b.trg_y[:self._n_sampled] != self.pad).sum(), (self._ae_y != self.pad).sum()]).float()
        return torch.stack([(b.trg_y != self.pad).sum(), (self._ae_y != self.pad).sum()]).float()

    def _refresh_norms(self):
        """dynamic_norms on ONE rank: recomputed inside the (captured) step.  Under data parallelism the global counts need a
        collective, which stays out of graph capture: the caller refreshes them eagerly (refresh_norms_eager) before the step."""
        if self.dynamic_norms and self.grad_sync is None:
            self._norms.copy_(self.local_norms())

    def refresh_norms_eager(self):
        if self.dynamic_norms and self.grad_sync is not None:
            n = self.local_norms()
            self.grad_sync.all_reduce_scalars(n)
            self._norms.copy_(n)

    # ---- knowledge distillation
    def _init_teacher(self, teacher, alpha, temperature, vocab):
        self.teacher, self._teacher_rows, self.last_kd = teacher, None, None
        self.distill_alpha, self.distill_temperature = float(alpha), float(temperature)
        if teacher is None:
            return
        members, _, _ = teacher_members(teacher)
        dev = next(self.model.parameters()).device
        for m in members:
            if m is self.model:
                raise ValueError("TrainStep: the teacher is the student itself (pass a frozen copy)")
            if int(m.generator.proj.weight.size(0)) != int(vocab):
                raise ValueError(f"TrainStep: a teacher's vocabulary size ({int(m.generator.proj.weight.size(0))}) is not the student's ({vocab})")
            if next(m.parameters()).device != dev:
                raise ValueError("TrainStep: the teacher is not on the student's device")
            m.eval()
            m.prepare()
        self._teacher_rows = torch.empty(self.batch.trg_y.numel(), int(vocab), device=dev, dtype=torch.float32)
        self.last_kd = torch.zeros((), device=dev)

    def _teacher_pass(self):
        """The teacher's rows for this batch, into the buffer allocated once; returns it (None without a teacher).  eval() forwards
        under no_grad: no dropout stream is advanced, nothing enters a parameter-gradient queue, and every forward ends by flushing
        its rider work (EncoderDecoder.forward), so the student's launches that follow are those of the undistilled step.
        Scheduled sampling's first pass is such a forward too, by the student itself: it runs here."""
        if self.sched is not None:
            self._sched_pass()
        if self._teacher_rows is None:
            return None
        return teacher_rows(self.teacher, self.batch, out=self._teacher_rows)

    # ---- scheduled sampling
    def _init_sched(self):
        """``_fwd_batch``: what the training forward reads.  The gold batch itself without scheduled sampling."""
        self._fwd_batch, self.sched_mixed, self.sched_keys, self.sched_stats = self.batch, None, None, None
        if self.sched is None:
            return
        import copy
        b = self.batch
        if b.trg.size(1) >= 4096 or not b.trg.is_contiguous():
            raise ValueError("TrainStep: sched needs contiguous decoder inputs of fewer than 4096 target positions")
        rank = 0
        if self.grad_sync is not None and torch.distributed.is_available() and torch.distributed.is_initialized():
            rank = torch.distributed.get_rank(getattr(self.grad_sync, "group", None))
        B, dev = b.trg.size(0), b.trg.device
        self.sched_keys = torch.arange(rank * B, rank * B + B, dtype=torch.int64, device=dev)
        self.sched_stats = torch.zeros(3, dtype=torch.int64, device=dev)
        self.sched_mixed = b.trg.detach().clone().contiguous()
        self._fwd_batch = copy.copy(b)
        self._fwd_batch.trg = self.sched_mixed

    def _sched_pass(self):
        """The first pass: the student's eval() forward over the GOLD batch under no_grad, its generator logits, one mtn_sched_mix
        launch into ``sched_mixed``."""
        from . import ops
        cfg, m, b = self.sched, self.model, self.batch
        training = m.training
        m.eval()
        try:
            with torch.no_grad():
                state = self.opt.optimizer.state
                if self.overlap and self.sharded is not None:
                    # the one schedule that advances the optimiser state BEFORE the forward (begin_sharded_step ahead of the segment
                    # graphs): the draws are those of the update count every other schedule reads, so no schedule changes the stream
                    state = (state[:1] - 1.0).clamp_(min=0.0)
                o, _ = m.forward(b)
                z = m.generator.logits(o)
                ops.sched_mix(z.reshape(-1, z.size(-1)), b.trg, self.sched_keys, state, pad=self.pad, prob=cfg.prob,
                              start=cfg.start, ramp=cfg.ramp, pick=cfg.pick, temperature=cfg.temperature, seed=cfg.seed,
                              banned=cfg.banned, out=self.sched_mixed, stats=self.sched_stats)
        finally:
            if training:
                m.train()

    # ---- R-Drop
    @staticmethod
    def _check_paired(batch):
        """A pre-paired batch: 2 N rows, row N + b the second pass of row b.  One host read, at construction."""
        y = batch.trg_y
        if y.size(0) < 2 or y.size(0) % 2 != 0:
            raise ValueError("TrainStep: rdrop_paired needs a batch of 2 N rows (got %d)" % y.size(0))
        N = y.size(0) // 2
        differ = (y[:N] != y[N:]).any(1).nonzero()
        if differ.numel() > 0:
            raise ValueError("TrainStep: rdrop_paired: the targets of row %d and of its partner, row %d, differ" % (int(differ[0]), int(differ[0]) + N))

    def _init_rdrop(self, src, pad):
        """The static batch of 2 B rows the step trains on, rows b and B + b both dialogue b of the source."""
        from .data_utils import Batch
        if getattr(src, "trg", None) is None:
            raise ValueError("TrainStep: rdrop needs the source batch's answers")
        two = lambda t: torch.cat([t, t]).contiguous()
        b = Batch(two(src.query), two(src.his), None, None, None if src.cap is None else two(src.cap), two(src.trg), two(src.trg_y), pad=pad,
                  device=src.query.device)
        if src.fts is not None:                                    # (already cleaned by the source's constructor: not through it again)
            b.fts, b.fts_mask = [two(f) for f in src.fts], [two(m) for m in src.fts_mask]
        self._rd_src, self.batch = src, b

    def _rdrop_refill(self):
        """The source batch into both halves of the static batch, in place: one copy per tensor that writes both halves, and the masks' kernel images
        (ops.prepare_masks).  Part of the (captured) step; nothing is read on the host."""
        src, b = self._rd_src, self.batch
        if src is None:
            return
        B = src.query.size(0)

        def both(dst, rows):                     # one broadcast copy into the two halves (two slice copies if dst cannot be viewed so)
            if dst.is_contiguous():
                dst.view((2,) + tuple(rows.shape)).copy_(rows.unsqueeze(0).expand((2,) + tuple(rows.shape)))
            else:
                dst[:B].copy_(rows)
                dst[B:].copy_(rows)

        def put(dst, rows):
            both(dst, rows)
            u8 = getattr(dst, "_mtn_u8", None)
            if u8 is not None and u8.data_ptr() != dst.data_ptr():
                both(u8, rows)

        for name in ("query", "his", "trg", "trg_y") + (("cap",) if src.cap is not None else ()):
            put(getattr(b, name), getattr(src, name))
        for name in ("query_mask", "his_mask", "trg_mask") + (("cap_mask",) if src.cap is not None else ()):
            put(getattr(b, name), getattr(src, name))
        if src.fts is not None:
            for f, m, sf, sm in zip(b.fts, b.fts_mask, src.fts, src.fts_mask):
                put(f, sf)
                put(m, sm)

    # ---- self-critical sequence training
    def _init_scst(self, src, pad):
        from .data_utils import Batch
        cfg = self.scst
        B, S, T = src.query.size(0), cfg.samples, cfg.max_length
        gold = cfg.xe_weight > 0
        if gold and (getattr(src, "trg", None) is None or src.trg.size(1) > T):
            raise ValueError("TrainStep: scst with xe_weight needs the source batch's answers, of at most max_length positions")
        dev = src.query.device
        self.src, self._n_sampled = src, B * S
        idx = torch.arange(B, device=dev).repeat_interleave(S)
        if gold:
            idx = torch.cat([idx, torch.arange(B, device=dev)])
        self._rep_idx = idx
        rows = idx.numel()
        trg = torch.full((rows, T), pad, dtype=torch.long, device=dev)
        trg_y = torch.full((rows, T), pad, dtype=torch.long, device=dev)
        trg[:, 0], trg_y[:, 0] = cfg.sos, cfg.eos                      # empty responses until rows are loaded or drawn
        b = Batch(src.query[idx], src.his[idx], None, None, None if src.cap is None else src.cap[idx], trg, trg_y, pad=pad, device=dev)
        if src.fts is not None:
            b.fts, b.fts_mask = [f[idx].contiguous() for f in src.fts], [m[idx].contiguous() for m in src.fts_mask]
        self.batch = b
        self._roww = torch.zeros(rows, T, dtype=torch.float32, device=dev)
        self._means = torch.zeros(2, dtype=torch.float64, device=dev)
        self.last_reward, self.last_baseline = self._means[0], self._means[1]
        self._hyp_len = torch.zeros(B * S, dtype=torch.int32, device=dev)
        self._item = torch.zeros(B * S, dtype=torch.int32, device=dev)
        self._rl_steps = 0
        self._pad_scst = pad
        self._replicate()

    def _replicate(self):
        """The source batch's encoder-side tensors (and, with xe_weight, its answers as the gold rows) into the static batch, in place:
        the masks' kernel images (ops.prepare_masks) follow."""
        src, b, idx, n, pad = self.src, self.batch, self._rep_idx, self._n_sampled, self._pad_scst

        def put(dst, rows):
            dst.copy_(rows)
            u8 = getattr(dst, "_mtn_u8", None)
            if u8 is not None:
                u8.copy_(rows)

        for name in ("query", "his") + (("cap",) if src.cap is not None else ()):
            getattr(b, name).copy_(getattr(src, name)[idx])
            put(getattr(b, name + "_mask"), getattr(src, name + "_mask")[idx])
        if src.fts is not None:
            for f, m, sf, sm in zip(b.fts, b.fts_mask, src.fts, src.fts_mask):
                f.copy_(sf[idx])
                put(m, sm[idx])
        if idx.numel() > n:
            Tg = src.trg.size(1)
            b.trg[n:].fill_(pad)
            b.trg_y[n:].fill_(pad)
            b.trg[n:, :Tg].copy_(src.trg)
            b.trg_y[n:, :Tg].copy_(src.trg_y)
            self._roww[n:].fill_(self.scst.xe_weight)
        self._refresh_target_mask()

    def _refresh_target_mask(self):
        from .data_utils import Batch
        b = self.batch
        m = Batch.make_std_mask(b.trg, self._pad_scst)
        b.trg_mask.copy_(m)
        u8 = getattr(b.trg_mask, "_mtn_u8", None)
        if u8 is not None:
            u8.copy_(m)

    def load_rows(self, trg, trg_y, weights):
        """Test entry: fixed rows in the place of the samples.  ``trg`` / ``trg_y`` (n, max_length) int64 for the first n rows of the
        static batch (n = B * S, or every row), ``weights`` (n,) or (n, max_length) float: one weight per row or per target position."""
        b, n = self.batch, trg.size(0)
        if n not in (self._n_sampled, b.trg.size(0)) or tuple(trg.shape) != tuple(b.trg[:n].shape) or tuple(trg_y.shape) != tuple(trg.shape):
            raise ValueError("load_rows: (B * S, max_length) or (every row, max_length) int64 targets")
        b.trg[:n].copy_(trg)
        b.trg_y[:n].copy_(trg_y)
        w = torch.as_tensor(weights, dtype=torch.float32).to(self._roww.device)
        self._roww[:n].copy_(w.reshape(n, -1).expand(n, self._roww.size(1)))
        self._refresh_target_mask()

    def _sample_log(self, items, seed):
        """The token log (max_length, B * S) int32 of one sampling search over the source batch, left on the device."""
        from . import decode as dec
        cfg, S = self.scst, self.scst.samples
        T = cfg.max_length
        temperature, top_k = (1.0, 1) if cfg.temperature == 0.0 else (cfg.temperature, cfg.top_k)
        banned = (self._pad_scst, cfg.sos)                             # neither can stand inside a target row
        params = dict(temperature=temperature, top_k=top_k, top_p=cfg.top_p, banned=banned, eos=cfg.eos, min_len=0)
        row_keys = [int(k) * S + s for k in items for s in range(S)]
        log = dec._sample_search(self.model, self.src, T, cfg.sos, self._pad_scst, S, seed, row_keys, params, True,
                                 T > dec.KV_CACHE_FROM, False, on_device=True)
        return log[0]

    def _rewards(self, log_tok, item, trg=None, trg_y=None):
        """Assemble + reward launches for a (max_length, n) token log: the chosen reward, (n,) float64 on the device."""
        from . import ops
        cfg, T = self.scst, self.scst.max_length
        ref, ref_len, n_ref = cfg.refs
        n, dev = log_tok.size(1), log_tok.device
        if ref.stride(1) < T or ref.size(2) < T - 1:
            raise ValueError("TrainStep: scst needs reference rows of at least max_length - 1 tokens with a row stride >= max_length")
        if cfg._table is None:
            cfg._table = ops.eval_table_build(ref, ref_len, n_ref)
        hyp = torch.empty(n, ref.stride(1), dtype=torch.int32, device=dev)
        hyp_len = torch.empty(n, dtype=torch.int32, device=dev)
        if trg is None:
            trg, trg_y = torch.empty(n, T, dtype=torch.long, device=dev), torch.empty(n, T, dtype=torch.long, device=dev)
        ops.scst_assemble(log_tok, cfg.sos, cfg.eos, self._pad_scst, T=T, out=(trg, trg_y, hyp[:, :T], hyp_len), hyp_stride=ref.stride(1))
        _, rouge, cider = ops.eval_score_rows(hyp[:, :ref.size(2)], hyp_len, item, ref, ref_len, n_ref, cfg._table)
        return cider if cfg.reward == "cider" else rouge

    def rl_step(self, items, seed=None, timings=None):
        """One self-critical step on the source batch; ``items``: per dialogue its index in the reference corpus (also the sampling keys).
        ``seed``: of this step's draws (None: the config's seed + the steps this TrainStep has run).  With the greedy baseline the greedy
        search runs FIRST (it hands its tokens over the host), then the sampling search.  Returns the device tensor of the step's loss;
        ``last_reward`` / ``last_baseline`` hold the means.  ``timings``: a dict that accumulates the wall-clock ms of the step's three
        parts under "search", "reward" and "step" — a measuring aid (tools/scst_bench.py): the device is synchronised between them."""
        import time
        from . import decode as dec

        def lap(name, t0):
            if timings is None:
                return t0
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            timings[name] = timings.get(name, 0.0) + (t1 - t0) * 1e3
            return t1
        from . import ops
        cfg, m, b = self.scst, self.model, self.batch
        if cfg.refs is None:
            raise ValueError("TrainStep: rl_step needs ScstConfig.refs, the reference corpus on the device")
        B, S, T, n = self.src.query.size(0), cfg.samples, cfg.max_length, self._n_sampled
        if len(items) != B:
            raise ValueError("rl_step: one corpus item per dialogue of the source batch")
        dev = self._roww.device
        dlg_item = torch.tensor([int(i) for i in items], dtype=torch.int32).to(dev)
        self._item.copy_(dlg_item.repeat_interleave(S))
        t0 = lap("reward", time.perf_counter()) if timings is not None else 0.0
        training = m.training
        m.eval()
        m.prepare()                       # the compute-dtype copies the search reads are current (see __init__)
        try:
            with torch.no_grad():
                base = None
                if cfg.baseline == "greedy":
                    ys = dec.greedy_decode_many(m, self.src, T, cfg.sos, self._pad_scst)
                    glog = torch.cat([ys[:, 1:].to(torch.int32), torch.full((B, 1), cfg.eos, dtype=torch.int32, device=dev)], 1).t().contiguous()
                    base = self._rewards(glog, dlg_item)
                log_tok = self._sample_log(items, cfg.seed + self._rl_steps if seed is None else int(seed))
        finally:
            if training:
                m.train()
        t0 = lap("search", t0)
        reward = self._rewards(log_tok, self._item, b.trg[:n], b.trg_y[:n])
        ops.scst_advantage(reward.view(B, S), T, baseline=base, roww=self._roww, means=self._means)
        self._replicate()
        self._rl_steps += 1
        t0 = lap("reward", t0)
        loss = self()
        lap("step", t0)
        return loss

    def _loss_of(self, out, ae_out, teacher_rows):
        """The step's loss, for both schedules (monolithic _fwd_bwd, the segmented top())."""
        kw = self._loss_kw if teacher_rows is None else dict(self._loss_kw, teacher_logp=teacher_rows)
        loss = self.lc.loss(out, self.batch.trg_y, self._norms[0], ae_out, self._ae_y, self._norms[1], **kw)
        if self._last is not None:
            attr, of = self._last
            s = getattr(self.lc, of)             # (None: a teacher at alpha 0 on the composed path)
            setattr(self, attr, s / self._norms[0] if s is not None else torch.zeros_like(self._norms[0]))
        return loss

    def _begin_step(self):
        """The head of a step in every schedule: the R-Drop refill, the in-step normalisers, the scheduled-sampling and teacher passes,
        the glue gradients zeroed, and whatever a step that raised left queued or in exchange dropped (never mixed into this one; nothing
        happens on a clean state).  Returns the teacher's rows (None without a teacher)."""
        m, sh = self.model, self.sharded
        self._rdrop_refill()
        self._refresh_norms()
        teacher_rows = self._teacher_pass()
        m.zero_glue_grads()
        if m._queue is not None and (m._queue.gemm or m._queue.ln or m._queue._armed):
            m._queue.reset()
        if sh is not None and (sh._pending is not None or sh._works):
            sh.abort()
        return teacher_rows

    def _fwd_bwd(self, fuse: bool = False):
        m = self.model
        teacher_rows = self._begin_step()
        if fuse:
            self.opt.begin_fused_step()
        try:
            out, ae_out = m.forward(self._fwd_batch)
            loss = self._loss_of(out, ae_out, teacher_rows)
            loss.backward(self._unit_grad(loss))          # (a kept ones scalar: autograd would launch a fill for the implicit one)
        except BaseException:
            self._drop_step()
            raise
        return loss.detach()

    def _drop_step(self):
        """After a step that raised: its queued parameter-gradient work and its deferred shard update / gather never reach the next one."""
        if self.model._queue is not None:
            self.model._queue.reset()
        if self.sharded is not None:
            self.sharded.abort()

    def _unit_grad(self, loss):
        g = getattr(self, "_one", None)
        if g is None or g.device != loss.device or g.dtype != loss.dtype:
            g = self._one = torch.ones((), device=loss.device, dtype=loss.dtype)
        return g

    def _optim(self):
        self.opt.step()

    def _fused(self) -> bool:
        """One rank: the optimiser rides on the parameter-gradient GEMMs (no gradient exchange to wait for)."""
        if self._fuse_opt is None:
            self._fuse_opt = self.grad_sync is None and hasattr(self.opt, "begin_fused_step") and self.opt.optimizer.can_fuse()
        return self._fuse_opt

    def _step_fused(self):
        loss = self._fwd_bwd(fuse=True)
        self.opt.finish_fused_step()
        return loss

    # ---- layer-segmented backward (data parallel, overlapped exchange)
    def _segments(self):
        """[(callable, the (lo, hi, mat_hi) slice of _slices() that is final once the callable has run)]"""
        m = self.model
        slices = self._slices()
        N = len(m._layer_slices)

        def bwd(outs, leaves):
            # An auto-encoder output is BOTH the next layer's chain input (across the cut: its gradient arrives as leaf.grad) and the
            # memory of x's attention inside this layer.  In the monolithic graph the two gradients meet in one buffer (ops.py, the
            # ops.GradMeet: first writer = the chain input's dx, the memory-gradient GEMM accumulates into it); across a cut
            # autograd would ADD them (12 torch add launches per step, 112 us at batch 64: profiles/r04_x_*).  Here the leaf's gradient
            # seeds that meeting point instead of going to autograd: same summation order as the monolithic step, no add launch.
            roots, grads = [], []
            for o, l in zip(outs, leaves):
                if l.grad is None:
                    continue
                ga = getattr(o, "_mtn_gacc", None)
                if _CUT_GACC and ga is not None and ga.seed(l.grad, o.shape):
                    # the next layer offered THIS tensor (its dx, through the producer's output dropout, compute dtype) to the producer
                    # of `o` as a ready-made dy (ops.HandOff), valid while the tensor is untouched — it is about to be accumulated into:
                    # withdraw it (in bf16 mode the memory-gradient GEMM's epilogue hands the full sum over again; fp32 mode casts it)
                    h = getattr(o, "_mtn_next", None)
                    if h is not None:
                        h.withdraw(l.grad.data_ptr())
                    continue
                roots.append(o); grads.append(l.grad)
            if roots:
                torch.autograd.backward(roots, grads)

        def top():
            teacher_rows = self._begin_step()
            st = m.forward_segmented(self._fwd_batch)
            self._st = st
            loss = self._loss_of(st["out"], st["ae_out"], teacher_rows)
            loss.backward(self._unit_grad(loss))                # loss head + final LayerNorms
            ins, outs = st["layers"][N - 1]
            bwd(outs, st["top_in"])                             # top decoder layer
            self._loss = self._loss_t = loss.detach()

        def layer(k):
            def run():
                st = self._st
                ins, outs = st["layers"][k]
                bwd(outs, st["layers"][k + 1][0])
            return run

        def enc():
            st = self._st
            bwd(st["enc_out"], st["enc_leaf"])                  # embeddings, feature Linears, Encoder LayerNorms
            self._st = None

        return list(zip([top] + [layer(k) for k in range(N - 2, -1, -1)] + [enc], slices))

    def _exchanged(self, runners):
        """Segment runners [(callable, (lo, hi, mat_hi))] as stages: each slice's exchange goes out eagerly, asynchronously, right behind
        the callable (or graph) that finished it, and the step waits for them after the last."""
        sh, gs = self.sharded, self.grad_sync
        if sh is None:
            works = []
            reduce = lambda lo, hi: lambda: works.append(gs.reduce_range(lo, hi))
            return ([_Stage(after=works.clear)] + [_Stage(run, reduce(lo, hi)) for run, (lo, hi, _) in runners]
                    + [_Stage(after=lambda: gs.wait(works))])

        def begin():
            if sh._pending is not None or sh._works:
                sh.abort()                              # left over from a step that raised between reduce_update() and finish()
            self.opt.begin_sharded_step()

        def finish():
            if sh.timeline is not None and torch.cuda.is_available():
                e = torch.cuda.Event(enable_timing=True)
                e.record()                              # the compute chain (every segment graph) ends here; what follows is exposed exchange
                sh.timeline.append({"chain_end": e})
            sh.finish()

        return [_Stage(after=begin)] + [_Stage(run, lambda rng=rng: sh.reduce_update(*rng)) for run, rng in runners] + [_Stage(after=finish)]

    def _run_segmented(self, runners):
        """The layer-segmented forward / backward with its exchanges (no optimiser): ``runners`` = _segments(), or their graphs' replays."""
        self._run(self._exchanged(runners))

    def _stages(self):
        """The step as a list of _Stage in launch order, from (accumulating, overlap, sharded, grad_sync, _fused()).  Eager steps run it
        as it is; a captured step is the same list with every unit replaced by its graph's replay (_capture_schedule)."""
        update = self._refresh_after_exchange if self.sharded is not None else self._optim    # (sharded: the updates ran shard by shard)
        if self.accumulating:            # the accumulate launch (and, closing the window, the exchange) sit between the two graphs
            adam, sync = self.opt.optimizer, self.grad_sync
            return ([_Stage(self._unit_fwd_bwd, lambda: adam.accumulate(self._norms[0], self._closing, sumsq=sync is None))]
                    + ([_Stage(after=sync, closing=True)] if sync is not None else []) + [_Stage(self._optim, closing=True)])
        if self.overlap:
            return self._exchanged(self._segments()) + [_Stage(update)]
        if self.grad_sync is None:
            return [_Stage(self._unit_step)]
        return [_Stage(self._unit_fwd_bwd, self._whole_buffer_sharded if self.sharded is not None else self.grad_sync), _Stage(update)]

    def _unit_fwd_bwd(self):
        self._loss = self._fwd_bwd()

    def _unit_step(self):
        """One rank: the whole step is one unit."""
        if self._fused():
            self._loss = self._step_fused()
        else:
            self._loss = self._fwd_bwd()
            self._optim()

    def _run(self, stages):
        try:
            for st in stages:
                if st.closing and not self._closing:
                    break
                if st.unit is not None:
                    st.unit()
                if st.after is not None:
                    st.after()
        except BaseException:
            self._drop_step()
            raise

    def _capture(self):
        """Warm-up and capture.  The warm-up passes launch scheduled sampling's mix like any step: its counters are put back after."""
        keep = None if self.sched_stats is None else self.sched_stats.clone()
        try:
            self._capture_schedule()
        finally:
            if keep is not None:
                self.sched_stats.copy_(keep)

    def _capture_schedule(self):
        m = self.model
        m.prepare()
        self._fused()                               # decides (and builds its device-side tables) outside the capture
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):               # allocator / autograd warm-up off the capture stream
            for _ in range(2):
                self._fwd_bwd()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        if self.overlap:
            err = None
            try:
                stages = self._stages()
                with torch.cuda.stream(side):
                    for st in stages[:-1]:          # warm-up of the segmented schedule (no exchange: gradients are discarded)
                        if st.unit is not None:
                            st.unit()
                torch.cuda.current_stream().wait_stream(side)
                torch.cuda.synchronize()
                self._capture_stages(stages)
            except Exception as e:      # never lose the run to the more elaborate schedule: fall back to the simple one
                err = e
            # the decision is COLLECTIVE: a rank that fell back alone would issue a different sequence of collectives
            failed = torch.tensor([1.0 if err is not None else 0.0], device=self.model._flat.device)
            self.grad_sync.all_reduce_scalars(failed)
            if float(failed.item()) == 0.0:
                return
            import logging
            logging.getLogger("mtn_amd").warning("layer-segmented capture failed on %d rank(s) (%s); using the two-graph schedule",
                                                 int(failed.item()), err)
            self.overlap, self._g_seg, self._st, self._replays = False, None, None, None
            torch.cuda.synchronize()
        if self.accumulating:
            self.opt.optimizer._accum_sumsq = False       # (read by FusedAdam._clip inside the capture: this graph holds the norm launch)
        self._capture_stages(self._stages())
        if self.accumulating:                             # the optimiser stage picks between two graphs: see _replay_optim
            self._replays[-1] = self._replays[-1]._replace(unit=self._replay_optim)
        # the warm-up/capture passes did not run the optimiser outside capture: parameters are untouched

    def _capture_stages(self, stages):
        """One graph per unit, in order, all in the first one's memory pool; ``_replays`` = the stages with the replays for units."""
        graphs, replays, pool = [], [], None
        for st in stages:
            if st.unit is not None:
                g = torch.cuda.CUDAGraph()
                with L.capturing(g, pool=pool, capture_error_mode=CAPTURE_MODE):
                    st.unit()
                pool = g.pool()
                graphs.append(g)
                st = st._replace(unit=g.replay)
            replays.append(st)
        self._g_fb, self._g_opt = graphs[0], graphs[-1] if len(graphs) > 1 else None
        if self.overlap:                # [(replay, slice)] of the segment graphs, as _run_segmented takes them
            self._g_seg = [(g.replay, rng) for g, rng in zip(graphs[:-1], self._slices())]
        self._replays = replays

    def _capture_optim(self, have_sumsq: bool):
        """The optimiser graph of the accumulating step.  ``have_sumsq``: clipping reads the partials the closing mtn_grad_accum launch
        wrote (no mtn_grad_sumsq in this graph); False: the norm launch is part of it (a window of one, a gradient exchange, no clipping)."""
        self.opt.optimizer._accum_sumsq = bool(have_sumsq)       # (consumed by FusedAdam._clip inside the capture)
        g = torch.cuda.CUDAGraph()
        with L.capturing(g, pool=self._g_fb.pool(), capture_error_mode=CAPTURE_MODE):
            self._optim()
        return g

    def _replay_optim(self):
        """The accumulating step's optimiser graph: the one without the norm launch when the closing accumulate launch wrote its partials
        (captured the first time that happens)."""
        if not self.opt.optimizer._accum_sumsq:
            self._g_opt.replay()
            return
        if self._g_opt_sumsq is None:
            self._g_opt_sumsq = self._capture_optim(True)
        self._g_opt_sumsq.replay()

    def __call__(self, last: bool = True) -> torch.Tensor:
        """Runs one step; returns the device tensor of the NORMALISED loss (main KL / global target tokens + lambda * sum of the
        auto-encoder KLs / global query tokens: the `loss` of data_utils.py:135-144, before the `* norm` of :156), without
        synchronising.  ``last`` matters under accumulation only (``accumulate``): the call is one micro-step — forward + backward, the
        accumulate launch — and ``last`` closes the window: the exchange and the optimiser follow."""
        self._closing = bool(last) or not self.accumulating
        if self.use_graph and self._replays is None:
            self._capture()
        self._run(self._replays if self.use_graph else self._stages())
        return self._loss

    def _refresh_after_exchange(self):
        """After the sharded exchange: with the compute-dtype gather the matrices' bf16 copies arrived by all-gather, only the glue
        slice (generator, feature Linears: fp32 masters gathered) is cast; otherwise every weight is (the fp32 masters were gathered)."""
        lp_gather = self.sharded is not None and self.sharded.lp_mode()
        self.opt.optimizer.refresh_copies(self.model._layer_slices[0][0] if lp_gather else None)

    def _slices(self):
        """The (lo, hi) ranges of the flat buffers the exchange works in, last-finished-first: [top layer .. end], layers
        N-2 .. 0, [glue + encoder norms].  BOTH schedules use them, so which rank owns (and keeps the Adam moments of) an element
        never depends on the schedule a step ran under."""
        m = self.model
        m.prepare()
        sl = m._layer_slices
        total, N = m._flat_grad.numel(), len(sl)
        # a layer's slice is its weight matrices (mtn.py _ordered_params): mat_hi = hi -> they travel in the compute dtype; the last
        # slice = glue parameters + every vector (biases, all LayerNorms): fp32 throughout, complete once the last segment has run
        assert all(sl[k][1] == sl[k + 1][0] for k in range(N - 1)), "layer slices not contiguous"
        assert sl[N - 1][1] == total, "the last layer's matrices end the flat buffer"
        return [(sl[N - 1][0], total, total)] + [sl[k] + (sl[k][1],) for k in range(N - 2, -1, -1)] + [(0, sl[0][0], None)]

    def _whole_buffer_sharded(self):
        """The simple schedule (MTN_DP_OVERLAP=0, or the fallback) with the sharded optimiser: same slices as the segmented one."""
        self.opt.begin_sharded_step()
        for lo, hi, mat_hi in self._slices():
            self.sharded.reduce_update(lo, hi, mat_hi)
        self.sharded.finish()


class BucketedTrainer:
    """The reference's per-batch loop body (train.py:29-40) for batches of VARYING shape, on captured graphs: batch lengths
    are rounded up to multiples of ``bucket`` (padding is masked everywhere on the path, so the real tokens see the same
    arithmetic), one static Batch + one captured TrainStep is kept per padded shape, and every step refills that Batch in
    place on the device (data_handler.make_batch(out=...)) and replays its graph.  One optimiser state for all shapes."""

    def __init__(self, model, corpus, vocab_size: int, pad: int = 1, warmup: int = 4000, lam: float = 1.0, bucket: int = 8,
                 grad_sync=None, max_shapes: int = 64, teacher=None, distill_alpha: float = 0.5, distill_temperature: float = 1.0,
                 ema_decay: float = 0.0, scst: Optional[ScstConfig] = None, use_graph: bool = True, unlikelihood: float = 0.0,
                 clip_grad_norm: float = 0.0, accum_steps: int = 1, sched: Optional[SchedConfig] = None, rdrop: float = 0.0):
        """``scst``: self-critical sequence training — every padded shape keeps, next to its static source Batch, a TrainStep(scst=...)
        whose own static batch holds the drawn rows; a step refills the source in place and calls rl_step with the batch's QA ids as
        corpus items and sampling keys and the seed ``scst.seed + rl_steps`` (``rl_steps``: steps taken; set it after a resume).  With
        xe_weight the rows have max(scst.max_length, the shape's padded answer length) positions.  ``last_reward`` / ``last_baseline``:
        the last step's device scalars.  ``use_graph`` = False: the same steps run eagerly.
        ``unlikelihood``: TrainStep's alpha for every shape; ``last_ul``: the last step's device scalar (None at 0).
        ``clip_grad_norm``: > 0 = the one optimiser all shapes share clips the gradient's global norm (FusedAdam.enable_clip).
        ``accum_steps``: K > 1 = gradient accumulation (TrainStep's ``accumulate``): step() is one micro-step and every K-th one, or
        one called with ``last=True``, closes the window and updates.  The accumulator belongs to the shared optimiser, so the
        micro-steps of one window may fall into different padded shapes.  ``micro_steps`` / ``updates``: counted on the host.
        1 = off: today's step, launch for launch.
        ``sched``: scheduled sampling (TrainStep's ``sched``) for every shape: the rows' hash keys are the batch's QA ids, refilled
        before every step, and ``sched_stats`` is the one (3,) int64 device counter block all shapes add to (zero it to start a count).
        ``use_graph`` = False runs these steps eagerly.
        ``rdrop``: TrainStep's R-Drop alpha for every shape: each padded shape's static Batch is the source its step doubles inside the
        (captured) step; ``last_rd``: the last step's device scalar (None at 0).
        What combines with what: check_objectives."""
        if int(accum_steps) != accum_steps or int(accum_steps) < 1:
            raise ValueError("BucketedTrainer: accum_steps is an integer >= 1")
        check_objectives("BucketedTrainer", teacher=teacher, distill_alpha=distill_alpha, distill_temperature=distill_temperature, scst=scst,
                         unlikelihood=unlikelihood, rdrop=rdrop, sched=sched, clip_grad_norm=clip_grad_norm, grad_sync=grad_sync,
                         clipping=bool(clip_grad_norm), accumulating=int(accum_steps) > 1)
        self.rdrop, self.last_rd = float(rdrop), None
        self.sched, self.sched_stats = sched, None
        self.accum_steps, self.micro_steps, self.updates, self._in_window = int(accum_steps), 0, 0, 0
        self.unlikelihood, self.last_ul = float(unlikelihood), None
        self.scst, self.use_graph, self.rl_steps = scst, use_graph, 0
        self.last_reward = self.last_baseline = None
        self.model, self.corpus, self.vocab, self.pad, self.lam = model, corpus, vocab_size, pad, lam
        self.teacher, self.distill_alpha, self.distill_temperature = teacher, distill_alpha, distill_temperature
        self.bucket, self.grad_sync, self.max_shapes = bucket, grad_sync, max_shapes
        self.opt = NoamOpt(model.decoder.layers[0].size, 1.0, warmup, FusedAdam(model))
        if ema_decay:
            self.opt.optimizer.enable_ema(ema_decay)
        if clip_grad_norm:
            self.opt.optimizer.enable_clip(clip_grad_norm)
        if self.accum_steps > 1:
            self.opt.optimizer.enable_accumulation()
        self.steps = {}
        self.last_kd = None

    def _padded(self, index):
        up = lambda v: -(-int(v) // self.bucket) * self.bucket
        x_len, h_len, q_len, a_len, c_len, n = index[2:]
        return (index[0], index[1], [up(v) for v in x_len], up(h_len), up(q_len), up(a_len), up(c_len), n)

    def _key(self, index):
        """The padded shape an index entry falls into: the key of ``steps``."""
        pidx = self._padded(index)
        return (tuple(pidx[2]),) + tuple(pidx[3:])

    def step(self, index, cut_a: bool = False, rng=None, last: Optional[bool] = None):
        """One optimiser step on the batch described by ``index`` (an entry of data_handler.make_batch_indices with
        separate_caption=True).  Returns (device loss tensor, the static Batch that now holds this batch).  ``cut_a``: the
        reference's random answer truncation, drawn once per step from ``rng`` (data_handler.draw_cuts; None = np.random).
        ``last`` (accum_steps > 1: the call is one micro-step): None = the trainer counts and closes the window at accum_steps;
        True closes it now (an epoch's tail); False keeps it open, whatever the count."""
        from .data_handler import make_batch
        pidx = self._padded(index)
        key = (tuple(pidx[2]),) + tuple(pidx[3:])                    # (== self._key(index))
        hit = self.steps.get(key)
        if hit is None:
            if len(self.steps) >= self.max_shapes:
                self.steps.pop(next(iter(self.steps)))
            batch = make_batch(self.corpus, pidx, self.pad, separate_caption=True, cut_a=cut_a, rng=rng)
            cfg = self.scst
            if cfg is not None and cfg._table is None:           # once, before any per-shape copy of the config is made
                from . import ops
                cfg._table = ops.eval_table_build(*cfg.refs)
            if cfg is not None and cfg.xe_weight > 0 and batch.trg.size(1) > cfg.max_length:
                cfg = cfg.with_max_length(batch.trg.size(1))
            ts = TrainStep(self.model, batch, self.vocab, pad=self.pad, lam=self.lam, grad_sync=self.grad_sync, opt=self.opt,
                           dynamic_norms=True, teacher=self.teacher, distill_alpha=self.distill_alpha,
                           distill_temperature=self.distill_temperature, scst=cfg, use_graph=self.use_graph,
                           unlikelihood=self.unlikelihood, sched=self.sched, rdrop=self.rdrop)
            if self.sched is not None:                           # one counter block for every shape (read at launch: set before the capture)
                if self.sched_stats is None:
                    self.sched_stats = ts.sched_stats
                ts.sched_stats = self.sched_stats
            self.steps[key] = hit = (batch, ts)
        else:
            make_batch(self.corpus, pidx, self.pad, separate_caption=True, out=hit[0], cut_a=cut_a, rng=rng)
        hit[1].refresh_norms_eager()
        if self.sched is not None:
            hit[1].sched_keys.copy_(torch.tensor([int(q) for q in index[1]], dtype=torch.int64), non_blocking=False)
        if self.scst is not None:
            loss = hit[1].rl_step(list(index[1]), seed=self.scst.seed + self.rl_steps)
            self.rl_steps += 1
            self.last_reward, self.last_baseline = hit[1].last_reward, hit[1].last_baseline
            hit[1].batch._norms_global = hit[1]._norms
            return loss, hit[1].batch
        if self.accum_steps > 1:
            self._in_window += 1
            last = self._in_window >= self.accum_steps if last is None else bool(last)
            loss = hit[1](last)
            self.micro_steps += 1
            if last:
                self._in_window = 0
                self.updates += 1
        else:
            loss = hit[1]()
        self.last_kd = hit[1].last_kd               # (device scalar; None without a teacher)
        self.last_ul = hit[1].last_ul               # (device scalar; None without unlikelihood)
        self.last_rd = hit[1].last_rd               # (device scalar; None without R-Drop)
        hit[0]._norms_global = hit[1]._norms        # [target tokens, auto-encoder tokens] the step's loss is divided by (all ranks)
        return loss, hit[0]


def corpus_reference(corpus, min_len: int = 0, max_len: int = 128):
    """The corpus' tokenised answers as the reference corpus of ScstConfig.refs, uploaded once: item q = QA id q, one reference each, the
    answer's model token ids without <sos> / <eos> (cut at ``max_len`` = 128 tokens, the metric kernels' longest sentence).  Rows hold
    max(longest answer, ``min_len`` - 1) tokens with a row stride >= ``min_len``, what a step of ``min_len`` target positions needs.
    Returns (ref (Qc, 1, L) int32, ref_len (Qc, 1) int32, n_ref (Qc,) int32) on the corpus' device."""
    import numpy as np
    flat, start, lens = corpus.host_tok["trg_y"]                      # y.., <eos>
    n = np.minimum(np.maximum(lens.astype(np.int64) - 1, 0), max_len)
    Lr = int(min(max_len, max(int(n.max()) if len(n) else 1, min_len - 1, 1)))
    ld = -(-max(Lr, min_len) // 8) * 8
    ref = np.full((len(n), 1, ld), 1, dtype=np.int32)
    for q in range(len(n)):
        ref[q, 0, :n[q]] = flat[start[q]:start[q] + n[q]]
    dev = corpus.device
    return (torch.from_numpy(ref).to(dev)[:, :, :Lr], torch.from_numpy(n.astype(np.int32).reshape(-1, 1)).to(dev),
            torch.ones(len(n), dtype=torch.int32, device=dev))
