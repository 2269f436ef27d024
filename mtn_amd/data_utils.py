"""Batch / masks / optimiser / loss harness around the model — the surface of the reference's
data_utils.py + label_smoothing.py that train.py's batch loop drives (SURVEY.md §2 "IN as harness").

Differences that matter on MI355X: nothing here forces a host sync inside the step (the reference's
``loss.item()`` at data_utils.py:156 is optional), the optimiser is one fused Adam kernel over the flat
parameter buffer with the Noam rate computed on device (so a whole step can be captured in a hipGraph), and
tensors stay on whatever device they were created on (no hard-coded ``.cuda()``).
"""
from __future__ import annotations

import contextlib
import logging
import math
import os

from typing import List, NamedTuple, Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import lib as L


def subsequent_mask(size: int, device=None) -> torch.Tensor:
    """(1,size,size) bool, True where a position may be attended (data_utils.py:10-14)."""
    return torch.ones(1, size, size, dtype=torch.bool, device=device).tril_()


class Batch:
    """Holds one mini-batch with its masks (data_utils.py:21-54).  ``fts`` are (B,V,F) float tensors (already
    batch-first, on the target device) or (V,B,F) numpy arrays as data_handler.make_batch produces them."""

    def __init__(self, query, his, his_st=None, fts=None, cap=None, trg=None, trg_y=None, pad=0, device=None):
        dev = device if device is not None else query.device
        self.query, self.his, self.his_st = query.to(dev), his.to(dev), his_st
        if fts is not None:
            cleaned, masks = [], []
            for ft in fts:
                if not torch.is_tensor(ft):
                    ft = torch.from_numpy(ft).float().permute(1, 0, 2)          # data_utils.py:28
                ft = ft.to(dev)
                mask = ((ft != 1).sum(dim=2) != 0).unsqueeze(-2)                # frames padded with 1.0 (data_handler.py:236)
                cleaned.append(ft * mask.squeeze(-2).unsqueeze(-1).to(ft.dtype))
                masks.append(mask)
            self.fts, self.fts_mask = cleaned, masks
        else:
            self.fts = self.fts_mask = None
        self.query_mask = (self.query != pad).unsqueeze(-2)
        self.his_mask = (self.his != pad).unsqueeze(-2)
        if cap is not None:
            self.cap = cap.to(dev)
            self.cap_mask = (self.cap != pad).unsqueeze(-2)
        else:
            self.cap = self.cap_mask = None
        if trg is not None:
            self.trg, self.trg_y = trg.to(dev), trg_y.to(dev)
            self.trg_mask = self.make_std_mask(self.trg, pad)
            self.ntokens = (self.trg_y != pad).sum()

    @staticmethod
    def make_std_mask(tgt, pad):
        """pad mask AND causal mask (data_utils.py:48-54)."""
        return (tgt != pad).unsqueeze(-2) & subsequent_mask(tgt.size(-1), tgt.device)


class LabelSmoothing(nn.Module):
    """KLDivLoss(sum) against the smoothed target distribution (label_smoothing.py:9-32), computed in closed
    form without materialising the (rows, vocab) target matrix twice.  The reference's quirk is kept: rows
    whose target is <pad> are zeroed only if the SUM OF THEIR INDICES is > 0 (label_smoothing.py:29)."""

    def __init__(self, size: int, padding_idx: int, smoothing: float = 0.0):
        super().__init__()
        self.size, self.padding_idx, self.smoothing = size, padding_idx, smoothing
        self.confidence = 1.0 - smoothing

    def forward(self, x, target):
        assert x.size(1) == self.size
        eps = self.smoothing / (self.size - 2)
        true_dist = torch.full_like(x, eps)
        true_dist.scatter_(1, target.unsqueeze(1), self.confidence)
        true_dist[:, self.padding_idx] = 0
        pad_rows = target == self.padding_idx
        idx_sum = (torch.arange(target.numel(), device=target.device) * pad_rows).sum()
        zero_rows = pad_rows & (idx_sum > 0)                      # device-side form of the reference's host test
        true_dist = true_dist * (~zero_rows).unsqueeze(1).to(x.dtype)
        pos = true_dist > 0
        safe = torch.where(pos, true_dist, torch.ones_like(true_dist))
        return (true_dist * (safe.log() - x)).sum()


class FusedAdam:
    """Adam(betas=(0.9,0.98), eps=1e-9) (train.py:190) over the model's flat buffers in ONE kernel, with the Noam
    learning rate (data_utils.py:111-117) advanced on device.  Writes the compute-dtype weight copy in the same pass."""

    def __init__(self, model, betas=(0.9, 0.98), eps=1e-9):
        self.model = model
        self.betas, self.eps = betas, eps
        flat, _, _ = model.flat_buffers()
        self.m = torch.zeros_like(flat)
        self.v = torch.zeros_like(flat)
        self.state = torch.zeros(8, device=flat.device, dtype=torch.float32)   # step, lr, 1-b1^t, 1-b2^t
        self.param_groups = [{"lr": 0.0, "params": list(model.parameters())}]
        self.grad_scale: Optional[torch.Tensor] = None                        # device scalar multiplied into every gradient
        self._aux_cache = {}                      # host-side chunk lists of the table launch's front tiles (ops.ParamGradQueue._table_aux)
        self.ema: Optional[torch.Tensor] = None   # exponential moving average of the fp32 masters (enable_ema); None = off: nothing is launched
        self.ema_decay = 0.0
        self.clip_max_norm: Optional[float] = None   # gradient clipping by global norm (enable_clip); None = off: nothing is launched
        self.accum: Optional[torch.Tensor] = None    # gradient accumulation over a window of micro-batches (enable_accumulation); None = off

    def tick(self, factor: float, model_size: int, warmup: int):
        L.check(L.load().mtn_noam_tick(self.state.data_ptr(), factor, model_size, warmup, self.betas[0], self.betas[1], L.stream_ptr()))

    def _buffers(self):
        flat, flat_lp, grad = self.model.flat_buffers()
        self.model._ln_fold_stale = True          # every caller is about to change weights: the LayerNorm fold vectors go stale
        if self.m.data_ptr() == 0 or self.m.numel() != flat.numel() or self.m.device != flat.device:
            raise L.MtnHipError("model was re-flattened after the optimiser was built")
        return flat, flat_lp, grad, (None if flat_lp is flat else flat_lp.data_ptr())

    # ---- averaging in weight space: an EMA of the masters, a per-element buffer like the moments
    def enable_ema(self, decay: float):
        """Keep ema <- ema + c (p - ema) after every update of the masters, c = max(1 - decay, 9 / (10 + step)) computed on the device
        (include/mtn_hip.h mtn_ema_step), starting from a copy of the current masters.  The launches sit inside step() / step_rest() /
        step_range(), so they are captured with the step and every TrainStep that shares this optimiser updates the one buffer."""
        decay = float(decay)
        if not 0.0 < decay < 1.0:
            raise ValueError("FusedAdam.enable_ema: 0 < decay < 1, got %r" % (decay,))
        flat, _, _ = self.model.flat_buffers()
        if self.m.numel() != flat.numel() or self.m.device != flat.device:
            raise L.MtnHipError("model was re-flattened after the optimiser was built")
        self.ema, self.ema_decay = flat.detach().clone(), decay
        return self

    def _ema_update(self, flat, off: int, n: int):
        if self.ema is not None:
            L.check(L.load().mtn_ema_step(n, self.ema.data_ptr() + 4 * off, flat.data_ptr() + 4 * off, self.state.data_ptr(), self.ema_decay,
                                          None, L.stream_ptr()))

    # ---- gradient clipping by global norm: two launches ahead of the update, the coefficient stays on the device
    def enable_clip(self, max_norm: float):
        """Clip the gradient's global L2 norm at ``max_norm`` (> 0; inf measures the norm and never clips) as
        torch.nn.utils.clip_grad_norm_ does: from now on step() reduces the whole flat gradient buffer to its norm (mtn_grad_sumsq),
        turns it into scale = min(1, max_norm / (norm + 1e-6)) in device memory (mtn_clip_scale; times ``grad_scale`` if one is set,
        and the norm is then that of the scaled gradient) and hands that scalar to mtn_adam_step as its grad_scale: no host read, so the
        launches are captured with the step.  The reduction runs over the padding between parameters too: it is allocated as zeros and
        nothing on the separate-optimiser path writes there (tests/test_clip_step_gpu.py).  Adam is not linear in g, so the update
        cannot start before the whole gradient exists: can_fuse() is False while clipping is on and step_range() (the sharded
        data-parallel update) raises.  ``clip_norm``: device double, the norm of the step just run.  No optimiser state: nothing to
        checkpoint."""
        max_norm = float(max_norm)
        if not max_norm > 0.0:                     # (nan fails the comparison)
            raise ValueError("FusedAdam.enable_clip: max_norm > 0 (inf allowed), got %r" % (max_norm,))
        flat, _, grad = self.model.flat_buffers()
        if self.m.numel() != flat.numel() or self.m.device != flat.device:
            raise L.MtnHipError("model was re-flattened after the optimiser was built")
        if getattr(self, "_sharded", None) is not None:
            raise L.MtnHipError("gradient clipping does not combine with the sharded data-parallel optimiser")
        self._clip_np = int(L.load().mtn_grad_sumsq_partials(grad.numel()))
        self._clip_partial = torch.zeros(self._clip_np, device=flat.device, dtype=torch.float64)
        self._clip_f64 = torch.zeros(6, device=flat.device, dtype=torch.float64)      # [0] the norm, [1:6] the stats block
        self.clip_norm, self._clip_stats = self._clip_f64[0], self._clip_f64[1:]
        self.clip_scale = torch.ones(1, device=flat.device, dtype=torch.float32)
        self.clip_max_norm = max_norm
        return self

    def _clip(self, grad):
        """The two clipping launches; returns the device scalar the update multiplies every gradient by."""
        if self.clip_max_norm is None:
            return self.grad_scale
        if grad.numel() != self.model._flat_grad.numel() or int(L.load().mtn_grad_sumsq_partials(grad.numel())) != self._clip_np:
            raise L.MtnHipError("model was re-flattened after clipping was enabled")
        h, st = L.load(), L.stream_ptr()
        if getattr(self, "_accum_sumsq", False):   # the launch that closed the accumulation window wrote these partials (accumulate)
            self._accum_sumsq = False
        else:
            L.check(h.mtn_grad_sumsq(grad.numel(), grad.data_ptr(), self._clip_partial.data_ptr(), st))
        L.check(h.mtn_clip_scale(self._clip_np, self._clip_partial.data_ptr(), self.clip_max_norm, L.ptr(self.grad_scale),
                                 self.clip_scale.data_ptr(), self.clip_norm.data_ptr(), self._clip_stats.data_ptr(), st))
        return self.clip_scale

    def clip_stats(self, reset: bool = False):
        """Since the last reset: dict(mean, max: of the finite gradient norms; steps; clipped: steps whose coefficient was < 1;
        nonfinite: steps whose norm was inf or NaN — their update wrote NaN).  One small D2H copy (it synchronises)."""
        if self.clip_max_norm is None:
            raise L.MtnHipError("clip_stats(): clipping is off (enable_clip)")
        s = [float(x) for x in self._clip_stats.cpu()]
        if reset:
            self._clip_stats.zero_()
        fin = s[2] - s[4]
        return {"mean": s[0] / fin if fin > 0 else 0.0, "max": s[1], "steps": int(s[2]), "clipped": int(s[3]), "nonfinite": int(s[4])}

    # ---- gradient accumulation: one launch per micro-step over a second flat fp32 buffer, the window's gradient lands in the gradient buffer
    def enable_accumulation(self):
        """Accumulate the gradient over a window of micro-batches before every update: ``accum`` (zeros like the flat gradient buffer)
        collects w_k * g_k and the launch that closes the window writes G = (sum_k w_k g_k) / (sum_k w_k) over the gradient buffer in
        place (include/mtn_hip.h mtn_grad_accum states the arithmetic), where the exchange, clipping and the update already read it.
        ``accumulate(w, last)`` is one micro-step's launch; the caller runs tick / step once per window, so the step count counts
        windows.  The sublayer gradients are overwritten by every backward pass, so the optimiser epilogue of the dW GEMMs would update
        a weight before the window's gradient exists: can_fuse() is False while accumulation is on, fuse_into_backward() and
        step_range() (the sharded data-parallel update) raise.  Windows never span an epoch: no optimiser state, nothing to checkpoint."""
        flat, _, grad = self.model.flat_buffers()
        if self.m.numel() != flat.numel() or self.m.device != flat.device:
            raise L.MtnHipError("model was re-flattened after the optimiser was built")
        if getattr(self, "_sharded", None) is not None:
            raise L.MtnHipError("gradient accumulation does not combine with the sharded data-parallel optimiser")
        self.accum = torch.zeros_like(grad)
        self._accum_total = torch.zeros(2, device=grad.device, dtype=torch.float32)    # the two slots the launches alternate between
        self._accum_k = 0                          # micro-steps of the open window already accumulated (host side)
        self._accum_sumsq = False                  # the closing launch wrote clipping's partials: _clip skips its mtn_grad_sumsq once
        self.accum_windows = self.accum_micro = 0  # windows closed / micro-steps seen so far (host side)
        return self

    def accumulate(self, w, last: bool, sumsq: bool = True) -> bool:
        """One micro-step of the open window: its gradient is in the flat gradient buffer, ``w`` is its weight (a device float: the
        micro-step's target-token count over all ranks).  The window's first micro-step is MTN_ACCUM_FIRST, the one that closes it
        (``last``) MTN_ACCUM_LAST, the others MTN_ACCUM_ADD; a window of one launches nothing.  With clipping on and ``sumsq``, the
        closing launch writes the partials of the window gradient's sum of squares, and the update that follows skips its
        mtn_grad_sumsq launch; pass ``sumsq`` = False when a gradient exchange comes between (the norm is the reduced gradient's).
        Stream-ordered, no host read.  Returns ``last``."""
        if self.accum is None:
            raise L.MtnHipError("accumulate(): accumulation is off (enable_accumulation)")
        grad = self.model.flat_buffers()[2]
        if grad.numel() != self.accum.numel() or grad.device != self.accum.device:
            raise L.MtnHipError("model was re-flattened after accumulation was enabled")
        if not (torch.is_tensor(w) and w.dtype == torch.float32 and w.device == grad.device and w.numel() == 1):
            raise ValueError("accumulate(): w is one float32 on the gradient's device")
        k, last = self._accum_k, bool(last)
        self._accum_sumsq = False
        self.accum_micro += 1
        self._accum_k = 0 if last else k + 1
        self.accum_windows += int(last)
        if last and k == 0:                        # a window of one: the gradient buffer is the window's gradient already
            return last
        h = L.load()
        partial = None
        if last and sumsq and self.clip_max_norm is not None:
            if int(h.mtn_grad_sumsq_partials(grad.numel())) != self._clip_np:
                raise L.MtnHipError("model was re-flattened after clipping was enabled")
            partial, self._accum_sumsq = self._clip_partial, True
        mode = L.MTN_ACCUM_FIRST if k == 0 else (L.MTN_ACCUM_LAST if last else L.MTN_ACCUM_ADD)
        tot = self._accum_total
        L.check(h.mtn_grad_accum(mode, grad.numel(), self.accum.data_ptr(), grad.data_ptr(), w.data_ptr(),
                                 None if k == 0 else tot.data_ptr() + 4 * ((k - 1) & 1), tot.data_ptr() + 4 * (k & 1), L.ptr(partial),
                                 L.stream_ptr()))
        return last

    def step(self):
        flat, flat_lp, grad, lp_ptr = self._buffers()
        L.check(L.load().mtn_adam_step(L.dtype_code(self.model.compute_dtype), flat.numel(), flat.data_ptr(), grad.data_ptr(),
                                       self.m.data_ptr(), self.v.data_ptr(), lp_ptr, self.state.data_ptr(),
                                       L.ptr(self._clip(grad)), self.betas[0], self.betas[1], self.eps, L.stream_ptr()))
        self._ema_update(flat, 0, flat.numel())
        self.model.refresh_transposed()

    def step_range(self, off: int, n: int, write_lp: bool = False):
        """The update on flat elements [off, off+n) only (data parallel: this rank's shard of a gradient slice,
        dp.ShardedOptimizerSync).  write_lp = False: the compute-dtype copies are NOT written — the caller refreshes them once all
        shards of all ranks have arrived (refresh_copies); True: the shard's compute-dtype copy is written by the same pass (the
        compute-dtype gather: the other ranks receive THAT, not the fp32 master)."""
        if self.accum is not None:
            raise L.MtnHipError("FusedAdam.step_range: gradient accumulation updates once per window, from the whole window gradient; "
                                "the sharded data-parallel optimiser updates shard by shard (use the all-reduce scheme)")
        if self.clip_max_norm is not None:
            raise L.MtnHipError("FusedAdam.step_range: gradient clipping needs the whole reduced gradient before any element is updated; "
                                "the sharded data-parallel optimiser updates shard by shard (use the all-reduce scheme)")
        flat, flat_lp, grad, lp_ptr = self._buffers()
        assert off % 4 == 0 and n > 0
        lp = None
        if write_lp and lp_ptr is not None:
            lp = lp_ptr + flat_lp.element_size() * off
        L.check(L.load().mtn_adam_step(L.dtype_code(self.model.compute_dtype), n, flat.data_ptr() + 4 * off, grad.data_ptr() + 4 * off,
                                       self.m.data_ptr() + 4 * off, self.v.data_ptr() + 4 * off, lp, self.state.data_ptr(),
                                       L.ptr(self.grad_scale), self.betas[0], self.betas[1], self.eps, L.stream_ptr()))
        self._ema_update(flat, off, n)

    def step_range_lp(self, off: int, n: int):
        self.step_range(off, n, write_lp=True)

    def refresh_copies(self, hi: Optional[int] = None):
        """Compute-dtype weight copy + transposed copies from the fp32 master (after a sharded update + all-gather).  ``hi``:
        only flat elements [0, hi) are cast (compute-dtype gather: the matrices' copies arrived by all-gather already; what is left
        is the glue slice — generator / feature Linears — whose masters were gathered in fp32)."""
        m = self.model
        flat, flat_lp, _, lp_ptr = self._buffers()
        if lp_ptr is not None:
            n = flat.numel() if hi is None else min(int(hi), flat.numel())
            if n > 0:
                L.check(L.load().mtn_cast_f32_to_lp(L.dtype_code(m.compute_dtype), n, flat.data_ptr(), lp_ptr, L.stream_ptr()))
        m.refresh_transposed()

    # ---- optimiser epilogue: the update of the sublayer weight matrices rides on their parameter-gradient GEMMs
    def can_fuse(self) -> bool:
        m = self.model
        if self.clip_max_norm is not None:        # the epilogue updates a weight before the rest of the gradient exists
            return False
        if self.accum is not None:                # ... or, under accumulation, before the window's gradient exists
            return False
        m.prepare()
        ok = bool(getattr(m, "_fusable", None)) and m._flat.is_cuda and os.environ.get("MTN_NO_FUSED_ADAM") is None
        if ok:      # build the two expected "rest" tables now: they are device tensors and the step may be under graph capture later
            every = frozenset(t[0] for t in m._fusable)
            m.rest_tables(every)
            m.rest_tables(every - m._fusable_optional)
        return ok

    def fuse_into_backward(self, write_grad: bool = False):
        """Arm the model's parameter-gradient queue: its next flush (the end of the coming backward pass) applies THIS
        step's update to every sublayer weight matrix inside the dW GEMM that produces its gradient (include/mtn_hip.h
        mtn_adam_fuse) — no gradient round trip through HBM, no separate transpose pass.  The schedule must already have
        been advanced (tick) and ``step_rest()`` must follow the backward pass.  Single-rank only: with data parallelism
        the gradients are exchanged between backward and the update."""
        if self.accum is not None:
            raise L.MtnHipError("FusedAdam.fuse_into_backward: gradient accumulation needs the separate optimiser pass (can_fuse() is False)")
        if self.clip_max_norm is not None:
            raise L.MtnHipError("FusedAdam.fuse_into_backward: gradient clipping needs the separate optimiser pass (can_fuse() is False)")
        flat, flat_lp, grad, lp_ptr = self._buffers()
        m = self.model
        esz = flat_lp.element_size()
        self._armed = dict(fusable=m._fusable, starts=[t[0] for t in m._fusable], optional=m._fusable_optional, covered=frozenset(),
                           grad=grad.data_ptr(), p=flat.data_ptr(), m=self.m.data_ptr(), v=self.v.data_ptr(), lp=lp_ptr,
                           lpT=m._flat_lpT.data_ptr() if m._flat_lpT is not None else None,
                           t_map=dict(m._t_off), esz=esz, write_grad=write_grad,
                           state=self.state.data_ptr(), grad_scale=L.ptr(self.grad_scale), betas=self.betas, eps=self.eps, applied=False,
                           n_flat=flat.numel(), rest_done=False, aux_cache=self._aux_cache)
        m._queue.adam = self._armed

    def step_rest(self):
        """After a backward pass armed by fuse_into_backward(): the update of everything the GEMM epilogues did not touch."""
        m = self.model
        armed, m._queue.adam = m._queue.adam, None
        if armed is None or not armed["applied"]:
            raise L.MtnHipError("optimiser epilogue was armed but the backward pass did not run its parameter-gradient GEMMs")
        flat, flat_lp, grad, lp_ptr = self._buffers()
        (off, ln, n), trest = m.rest_tables(armed["covered"])
        if not armed["rest_done"]:                 # (round 5: normally the table launch's front tiles have done this — ops.ParamGradQueue._table_aux)
            L.check(L.load().mtn_adam_step_chunks(L.dtype_code(m.compute_dtype), n, off.data_ptr(), ln.data_ptr(), flat.data_ptr(),
                                                  grad.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), lp_ptr, self.state.data_ptr(),
                                                  L.ptr(self.grad_scale), self.betas[0], self.betas[1], self.eps, L.stream_ptr()))
        self._ema_update(flat, 0, flat.numel())    # by now the table launch and the GEMM epilogues have written every master
        if trest is not None:
            m.refresh_transposed(trest)

    def zero_grad(self, set_to_none: bool = False):
        self.model.zero_glue_grads()

    def state_dict(self):
        """Optimiser state for checkpoints (the reference saves none: train.py:215-217 pickles the model only).  Moments are
        stored per parameter NAME, so a checkpoint survives a different flat layout; ``schedule`` is the device-side Noam /
        bias-correction state [step, lr, 1-b1^t, 1-b2^t]."""
        off = 0
        sh = getattr(self, "_sharded", None)
        if sh is not None:          # data parallel with a sharded optimiser: every rank holds the moments of its shards only
            sh.gather(self.m)
            sh.gather(self.v)
            self.gather_masters()
            if self.ema is not None:
                sh.gather(self.ema)
        out = {"schedule": self.state.detach().cpu().clone(), "exp_avg": {}, "exp_avg_sq": {}}
        if self.ema is not None:
            out["ema"], out["ema_decay"] = {}, self.ema_decay
        names = {id(p): n for n, p in self.model.named_parameters()}
        for p, o in zip(self.model._flat_params, self.model._flat_offsets):
            n = names[id(p)]
            out["exp_avg"][n] = self.m[o:o + p.numel()].view(p.shape).detach().cpu().clone()
            out["exp_avg_sq"][n] = self.v[o:o + p.numel()].view(p.shape).detach().cpu().clone()
            if self.ema is not None:
                out["ema"][n] = self.ema[o:o + p.numel()].view(p.shape).detach().cpu().clone()
        return out

    def _gather_average(self):
        """Data parallel with the sharded optimiser: a rank updates the average of its own shards only, as it does the moments — make
        the masters and the average whole on every rank.  A collective."""
        sh = getattr(self, "_sharded", None)
        if sh is not None:
            self.gather_masters()
            sh.gather(self.ema)

    def ema_state_dict(self):
        """The model's state dict in the reference's key schema with every parameter replaced by its average (what generate.py
        loads); entries that are not parameters are the model's.  A collective under data parallelism: every rank calls it."""
        if self.ema is None:
            raise L.MtnHipError("ema_state_dict(): the average is off (enable_ema)")
        self._buffers()
        self._gather_average()
        out = self.model.state_dict()
        offs = {id(p): o for p, o in zip(self.model._flat_params, self.model._flat_offsets)}
        for n, p in self.model.named_parameters(remove_duplicate=False):
            if n in out:
                o = offs[id(p)]
                out[n] = self.ema[o:o + p.numel()].view(p.shape).detach().clone()
        return out

    @contextlib.contextmanager
    def averaged_weights(self):
        """Inside the block the model computes with the averaged weights: masters and average are exchanged in place (mtn_swap_f32, no
        third buffer) and the compute-dtype copy, the transposed copies and the LayerNorm fold vectors follow, as after
        load_state_dict; on exit they are exchanged back, every byte as it was.  A collective under data parallelism."""
        if self.ema is None:
            raise L.MtnHipError("averaged_weights(): the average is off (enable_ema)")
        self._buffers()
        self._gather_average()
        self._swap_average()
        try:
            yield self
        finally:
            self._swap_average()

    def _swap_average(self):
        m = self.model
        flat = m._flat
        L.check(L.load().mtn_swap_f32(flat.numel(), flat.data_ptr(), self.ema.data_ptr(), L.stream_ptr()))
        m._flat_version = -1               # the masters changed under the model: recast and re-transpose, as prepare() does after load_state_dict
        m._ln_fold_stale = True
        m.prepare()

    def gather_masters(self):
        """Data parallel with the compute-dtype gather (dp.ShardedOptimizerSync): a rank keeps the fp32 master of its own shard of
        every weight matrix current and receives the others' bf16 copies only — bring every rank's masters up to date before
        anything reads them whole (model.state_dict()).  A collective: every rank calls it."""
        sh = getattr(self, "_sharded", None)
        if sh is not None and sh.lp_slices and sh.masters_stale:
            sh.gather(self.model._flat)
            sh.masters_stale = False

    def load_state_dict(self, sd):
        names = {id(p): n for n, p in self.model.named_parameters()}
        self.state.copy_(sd["schedule"].to(self.state.device))
        for p, o in zip(self.model._flat_params, self.model._flat_offsets):
            n = names[id(p)]
            self.m[o:o + p.numel()].copy_(sd["exp_avg"][n].reshape(-1).to(self.m.device))
            self.v[o:o + p.numel()].copy_(sd["exp_avg_sq"][n].reshape(-1).to(self.v.device))
        if self.ema is None:                       # the average is off here: a file that carries one loads as any other
            return
        if sd.get("ema") is not None:
            for p, o in zip(self.model._flat_params, self.model._flat_offsets):
                self.ema[o:o + p.numel()].copy_(sd["ema"][names[id(p)]].reshape(-1).to(self.ema.device))
        else:
            logging.getLogger("mtn_amd").info("optimiser state carries no weight average: the average starts from the loaded weights")
            self.gather_masters()                  # (data parallel: foreign masters may be stale; every rank loads the same file)
            self.ema.copy_(self.model.flat_buffers()[0])


class NoamOpt:
    """Optimiser wrapper with the reference's interface (data_utils.py:92-117): ``step()``, ``rate()``,
    ``.optimizer.zero_grad()``.  The schedule itself runs on device inside FusedAdam.tick()."""

    def __init__(self, model_size, factor, warmup, optimizer: FusedAdam):
        self.optimizer = optimizer
        self._step = 0
        self.warmup, self.factor, self.model_size = warmup, factor, model_size
        self._rate = 0

    def step(self):
        self._step += 1
        self.optimizer.tick(self.factor, self.model_size, self.warmup)
        self.optimizer.step()

    def begin_fused_step(self, write_grad: bool = False):
        """step() split around the backward pass (FusedAdam.fuse_into_backward): advance the schedule and arm the epilogue
        before it, finish_fused_step() after it.  Same arithmetic as step(), element for element."""
        self._step += 1
        self.optimizer.tick(self.factor, self.model_size, self.warmup)
        self.optimizer.fuse_into_backward(write_grad)

    def finish_fused_step(self):
        self.optimizer.step_rest()

    def begin_sharded_step(self):
        """Data parallel with a sharded optimiser (dp.ShardedOptimizerSync): advance the schedule now; the per-shard updates
        (FusedAdam.step_range) follow slice by slice, refresh_copies() at the end."""
        self._step += 1
        self.optimizer.tick(self.factor, self.model_size, self.warmup)

    def step_count(self) -> int:
        """Optimiser steps taken so far.  The schedule lives on the device (FusedAdam.state[0]) and advances on every replay
        of a captured step, which the host-side counter does not see: read it there (one small D2H copy; checkpoints / logs only)."""
        st = getattr(self.optimizer, "state", None)
        if torch.is_tensor(st) and st.numel() > 0:
            self._step = int(round(float(st[0].item())))
        return self._step

    def state_dict(self):
        return {"step": self.step_count(), "optimizer": self.optimizer.state_dict()}

    def load_state_dict(self, sd):
        self._step = int(sd["step"])
        self.optimizer.load_state_dict(sd["optimizer"])

    def rate(self, step=None):
        if step is None:
            step = self.step_count()
        return self.factor * (self.model_size ** (-0.5) * min(step ** (-0.5), step * self.warmup ** (-1.5)))


UL_CLAMP = 9.999999747378752e-06            # MTN_UL_CLAMP (include/mtn_hip.h): the float 1e-5f, fairseq's clamp


def unlikelihood_rows(logp, y, pad):
    """Token-level unlikelihood (Welleck et al. 2019) composed from PyTorch ops, the definition include/mtn_hip.h states for
    mtn_ulosshead_args: ``logp`` (B, T, V) log-probabilities, ``y`` (B, T) targets -> (B, T) ul = sum over the set of the sequence's
    earlier targets, without the row's own target and <pad>, of -log(clamp(1 - p_c, min=MTN_UL_CLAMP)); 0 on <pad>-target rows."""
    B, T, V = logp.shape
    onehot = torch.zeros(B, T, V, dtype=torch.bool, device=logp.device).scatter_(2, y.unsqueeze(2), True)
    cand = (onehot.cumsum(1) - onehot.long()) > 0                      # seen at an earlier position
    cand &= ~onehot                                                     # not the row's own target
    cand[:, :, pad] = False
    cand &= (y != pad).unsqueeze(2)
    u = torch.clamp(1.0 - logp.exp(), min=UL_CLAMP)
    return -(torch.where(cand, u, torch.ones_like(u)).log()).sum(2)


def rdrop_rows(logp, y, pad):
    """R-Drop (Liang et al. 2021) composed from PyTorch ops, the definition include/mtn_hip.h states for mtn_rlosshead_args: ``logp``
    (2 N, V) log-probabilities whose rows i and i + N are two passes of one position, ``y`` (2 N,) targets -> (2 N,) rd =
    (KL(p || q) + KL(q || p)) / 4 with p the row's distribution and q its partner's; 0 on rows whose own target is <pad>."""
    N = logp.size(0) // 2
    other = torch.cat([logp[N:], logp[:N]])
    d = logp - other
    rd = 0.25 * ((logp.exp() - other.exp()) * d).sum(-1)
    return torch.where(y.reshape(-1) != pad, rd, torch.zeros_like(rd))


class Objective(NamedTuple):
    """The main decoder stream's objective: ``kind`` (a key of ops.LOSS_HEADS) and that kind's parameters.  ``alpha``: the weight of
    the kind's extra term (distill, unlikelihood, rdrop)."""
    kind: str = "plain"
    alpha: float = 0.0
    temperature: float = 1.0                      # distill
    teacher: Optional[torch.Tensor] = None        # distill: (rows, V) log-probabilities or logits
    row_weights: Optional[torch.Tensor] = None    # weighted: one weight per row, or None (all ones)
    smoothing: Optional[float] = None             # weighted: in the place of the criterion's, or None


def objective(y, teacher_logp=None, alpha=0.0, temperature=1.0, row_weights=None, smoothing=None, unlikelihood=0.0, rdrop=0.0) -> Objective:
    """The Objective that SimpleLossCompute.loss's keywords describe for targets ``y``: every value check, and the one "at most one
    kind" check (ops.one_loss_head).  unlikelihood == 0 and rdrop == 0 are the plain head; ``smoothing`` alone selects the weighted one;
    a teacher at alpha == 0 stays "distill", whose kernels and composed form then never read it."""
    from . import ops
    unlikelihood, rdrop = float(unlikelihood), float(rdrop)
    for name, a in (("rdrop", rdrop), ("unlikelihood", unlikelihood)):
        if not (a >= 0.0 and math.isfinite(a)):
            raise ValueError("%s: alpha is finite and >= 0" % name)
    asked = {"distill": teacher_logp is not None, "weighted": row_weights is not None or smoothing is not None,
             "unlikelihood": unlikelihood > 0.0, "rdrop": rdrop > 0.0}
    kind = ops.one_loss_head([k for k in ops.LOSS_HEADS if asked.get(k)])
    if kind == "rdrop" and (y.dim() != 2 or y.size(0) % 2 != 0):
        raise ValueError("rdrop: y is (2 B, T)")
    if kind == "unlikelihood" and y.dim() != 2:
        raise ValueError("unlikelihood: y is (B, T)")
    if kind == "distill" and not (0.0 <= float(alpha) <= 1.0 and 0.0 < float(temperature) < float("inf")):
        raise ValueError("distillation: alpha in [0, 1] and a finite temperature > 0")
    if smoothing is not None and not (0.0 <= float(smoothing) <= 1.0):
        raise ValueError("smoothing in [0, 1]")
    if row_weights is not None and row_weights.numel() != y.numel():
        raise ValueError("row_weights: one weight per target row")
    if kind == "distill":
        return Objective(kind, float(alpha), float(temperature), teacher=teacher_logp)
    if kind == "weighted":
        return Objective(kind, row_weights=row_weights, smoothing=None if smoothing is None else float(smoothing))
    return Objective(kind, {"unlikelihood": unlikelihood, "rdrop": rdrop}.get(kind, 0.0))


class SimpleLossCompute:
    """generator -> label-smoothed KL (+ lambda * auto-encoder losses) -> backward -> optimiser step
    (data_utils.py:123-156).  ``sync=False`` returns the device tensor instead of ``loss.item()*norm`` so that the
    step contains no host synchronisation; ``grad_sync`` (optional callable) runs between backward and the
    optimiser step — that is where data-parallel gradient all-reduce goes."""

    def __init__(self, generator, ae_generator, criterion, opt=None, l=1.0, sync=True, grad_sync=None, fused=True):
        self.generator, self.ae_generator, self.criterion = generator, ae_generator, criterion
        self.opt, self.l, self.sync, self.grad_sync, self.fused = opt, l, sync, grad_sync, fused
        self._extra = (None, None)         # (spec key, value) of the last loss' extra row sum: what last_kd_sum / _ul_sum / _rd_sum read

    last_kd_sum, last_ul_sum, last_rd_sum = (property(lambda self, key=key: self._extra[1] if self._extra[0] == key else None)
                                             for key in ("kd_sum", "ul_sum", "rd_sum"))

    def _fused_loss(self, x, y, norm, ae_x, ae_y, ae_norm, teacher_logp=None, alpha=0.0, temperature=1.0, row_weights=None, smoothing=None,
                    unlikelihood=0.0, rdrop=0.0):
        """_fused_head from ``loss``'s keywords."""
        return self._fused_head(objective(y, teacher_logp, alpha, temperature, row_weights, smoothing, unlikelihood, rdrop), x, y, norm,
                                ae_x, ae_y, ae_norm)[0]

    def _fused_head(self, obj: Objective, x, y, norm, ae_x, ae_y, ae_norm):
        """Generator + log-softmax + label-smoothed KL + weighted sum as the fused HIP loss head (ops.GeneratorLossFn): (loss, the
        objective's extra row sum or None).  (None, None) when the fused path does not apply (CPU tensors, un-flattened model, vocab
        not a multiple of 8, foreign criterion): the caller then composes the same value from PyTorch ops."""
        from . import ops
        gens = [self.generator]
        xs, ys, norms, coefs = [x], [y], [norm], [1.0]
        if ae_x is not None:
            lst = ae_x if isinstance(ae_x, (list, tuple)) else [ae_x]
            for i, a in enumerate(lst):
                if self.ae_generator is not None:
                    gens.append(self.ae_generator[i] if isinstance(ae_x, (list, tuple)) else self.ae_generator)
                else:
                    gens.append(self.generator)
                xs.append(a); ys.append(ae_y); norms.append(ae_norm); coefs.append(self.l)
        if not (isinstance(self.criterion, LabelSmoothing) and x.is_cuda and len(xs) <= 4):
            return None, None
        fused = [getattr(g, "_fused", None) for g in gens]
        if any(f is None for f in fused) or self.criterion.size % 8 != 0:
            return None, None
        spec = dict(targets=ys, norms=[n if torch.is_tensor(n) else torch.tensor(float(n), device=x.device) for n in norms], coefs=coefs,
                    gens=[(f["w_lp"], f["bias"], f["grad_w"], f["grad_b"], f.get("w_lpT")) for f in fused], vocab=self.criterion.size,
                    pad=self.criterion.padding_idx, smoothing=self.criterion.smoothing, lp_dtype=fused[0]["lp_dtype"],
                    queue=fused[0].get("queue"))
        spec["norms"] = [n.detach().float().reshape(1) for n in spec["norms"]]
        rest = [None] * (len(xs) - 1)           # the main stream only: the auto-encoder streams keep the plain loss
        if obj.kind == "distill":
            spec["teacher"] = [obj.teacher.reshape(-1, obj.teacher.size(-1))] + rest
            spec["alpha"], spec["temperature"] = obj.alpha, obj.temperature
        elif obj.kind == "weighted":
            spec["row_weights"] = [None if obj.row_weights is None else obj.row_weights.detach().reshape(-1)] + rest
            spec["smoothing_seg"] = [obj.smoothing] + rest
        elif obj.kind == "unlikelihood":
            spec["unlikelihood"] = (obj.alpha, [y.size(1)] + rest)
        elif obj.kind == "rdrop":               # rows b T + t and (B + b) T + t are a pair
            spec["rdrop"] = (obj.alpha, [y.numel() // 2] + rest)
        return ops.GeneratorLossFn.apply(spec, *xs), spec.get(ops.LOSS_HEADS[obj.kind].sum_key)

    def _weighted_rows(self, logp, y, row_weights, smoothing):
        """The composed form of the weighted loss head (include/mtn_hip.h mtn_wlosshead_args): sum_rows w KL_ls at ``smoothing``."""
        crit = self.criterion
        V, pad = logp.size(-1), crit.padding_idx
        sm = float(crit.smoothing if smoothing is None else smoothing)
        td = torch.full_like(logp, sm / (V - 2))
        td.scatter_(1, y.unsqueeze(1), 1.0 - sm)
        td[:, pad] = 0
        is_pad = y == pad
        if int((torch.arange(y.numel(), device=y.device) * is_pad).sum()) > 0:      # label_smoothing.py:29, the lone-<pad> quirk
            td[is_pad] = 0
        kl = (td * (torch.where(td > 0, td, torch.ones_like(td)).log() - logp)).sum(1)
        return kl.sum() if row_weights is None else (row_weights.detach().reshape(-1).to(kl.dtype) * kl).sum()

    def loss(self, x, y, norm, ae_x=None, ae_y=None, ae_norm=None, teacher_logp=None, alpha=0.0, temperature=1.0, row_weights=None,
             smoothing=None, unlikelihood=0.0, rdrop=0.0):
        """The main stream's objective is at most one of the following (``objective``); the auto-encoder streams keep the plain loss.
        ``teacher_logp``: (rows, V) fp32 teacher log-probabilities (or logits: they are normalised) for the main stream — word-level
        knowledge distillation, loss = (1 - alpha) KL_ls + alpha T^2 KL(softmax(q / T) || softmax(z / T)) over the rows whose target is
        not <pad>, both over ``norm`` (include/mtn_hip.h mtn_distill_args).  alpha == 0 is the plain loss.  ``last_kd_sum`` is left
        holding the sum of the rows' KL (None without a teacher).
        ``row_weights``: one fp32 weight per main-stream row (signed; no gradient flows into it), loss = sum_rows w KL_ls / norm — the
        policy-gradient loss of self-critical sequence training when w = -(reward - baseline); ``smoothing``: the main stream's label
        smoothing in the place of the criterion's (0: KL_ls = -log p(target)) (include/mtn_hip.h mtn_wlosshead_args).
        ``unlikelihood``: alpha >= 0 of token-level unlikelihood training on the main stream, ``y`` (B, T): loss = (KL_ls + alpha
        sum_rows ul) / norm with ul the row's sum over its sequence's earlier targets (a set, without the row's own target and <pad>) of
        -log(clamp(1 - p_c, 1e-5)) (include/mtn_hip.h mtn_ulosshead_args).  0 is the plain loss.  ``last_ul_sum`` is left holding
        sum_rows ul (None at 0).
        ``rdrop``: alpha >= 0 of R-Drop on the main stream, ``y`` (2 B, T) with sequences b and B + b two passes of one dialogue: loss =
        (KL_ls + alpha sum_rows rd) / norm, rd = (KL(p || q) + KL(q || p)) / 4 between a row and its partner, 0 on <pad>-target rows
        (include/mtn_hip.h mtn_rlosshead_args).  0 is the plain loss.  ``last_rd_sum`` is left holding sum_rows rd (None at 0)."""
        from . import ops
        obj = objective(y, teacher_logp, alpha, temperature, row_weights, smoothing, unlikelihood, rdrop)
        loss, extra = self._fused_head(obj, x, y, norm, ae_x, ae_y, ae_norm) if self.fused else (None, None)
        if loss is None:
            loss, extra = self._composed(obj, x, y, norm, ae_x, ae_y, ae_norm)
        self._extra = (ops.LOSS_HEADS[obj.kind].sum_key, extra)
        return loss

    def _composed(self, obj: Objective, x, y, norm, ae_x, ae_y, ae_norm):
        """The same (loss, extra row sum) from PyTorch ops."""
        pad, extra = self.criterion.padding_idx, None
        out = self.generator(x)
        logp = out.reshape(-1, out.size(-1))
        if obj.kind == "weighted":
            loss = self._weighted_rows(logp, y.reshape(-1), obj.row_weights, obj.smoothing) / norm.float()
        else:
            loss = self.criterion(logp, y.reshape(-1)) / norm.float()
        if obj.kind == "distill" and obj.alpha != 0.0:      # (0, as the fused head: the teacher is not read, nothing is multiplied by 1 - alpha)
            # the composed form of the fused head's soft term: the generator's output is log_softmax(z), and log_softmax(logp / T) ==
            # log_softmax(z / T) (the row's log-sum-exp is a common shift)
            T = obj.temperature
            q = obj.teacher.reshape(-1, obj.teacher.size(-1)).to(logp.dtype)
            kd = F.kl_div(torch.log_softmax(logp / T, dim=-1), torch.softmax(q / T, dim=-1), reduction="none").sum(-1)
            extra = torch.where(y.reshape(-1) != pad, kd, torch.zeros_like(kd)).sum()
            loss = (1.0 - obj.alpha) * loss + obj.alpha * T * T * extra / norm.float()
        elif obj.kind == "unlikelihood":
            extra = unlikelihood_rows(out.reshape(y.size(0), y.size(1), out.size(-1)), y, pad).sum()
            loss = loss + obj.alpha * extra / norm.float()
        elif obj.kind == "rdrop":
            extra = rdrop_rows(logp, y, pad).sum()
            loss = loss + obj.alpha * extra / norm.float()
        if ae_x is not None:
            xs = ae_x if isinstance(ae_x, (list, tuple)) else [ae_x]
            for i, ae_in in enumerate(xs):
                if self.ae_generator is not None:
                    gen = self.ae_generator[i] if isinstance(ae_x, (list, tuple)) else self.ae_generator
                else:
                    gen = self.generator
                ae_out = gen(ae_in)
                loss = loss + self.l * self.criterion(ae_out.reshape(-1, ae_out.size(-1)), ae_y.reshape(-1)) / ae_norm.float()
        return loss, None if extra is None else extra.detach()

    def __call__(self, x, y, norm, ae_x=None, ae_y=None, ae_norm=None, teacher_logp=None, alpha=0.0, temperature=1.0, unlikelihood=0.0):
        loss = self.loss(x, y, norm, ae_x, ae_y, ae_norm, teacher_logp, alpha, temperature, unlikelihood=unlikelihood)
        if self.opt is not None:
            loss.backward()
            if self.grad_sync is not None:
                self.grad_sync()
            self.opt.step()
            self.opt.optimizer.zero_grad()
        out = loss.detach() * norm.float()
        return out.item() if self.sync else out
