"""Operators of the MTN hot path, backed by libmtn_hip.so.

Mirrors the reference's operator surface (mtn.py): ``LayerNorm.forward`` (:111-114),
``SublayerConnection.forward`` ∘ ``MultiHeadedAttention.forward`` (:125-127, :248-267, :221-231) and
``SublayerConnection.forward`` ∘ ``PositionwiseFeedForward.forward`` (:125-127, :279-280), each as one
``torch.autograd.Function`` whose forward/backward enqueue the fused HIP kernel chains.  PyTorch is used
for device memory, streams and autograd bookkeeping only.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from dataclasses import dataclass
from typing import Callable, Optional

import torch

from . import lib as L


# ------------------------------------------------------------------------------------------ helpers
_XACC = True          # a tensor with several consumers collects its gradients in one buffer (no autograd add)
_HANDOFF_MEM = True   # a memory's final gradient also leaves its last dmem GEMM as the producer's masked dy


def _drop(p: float, salt: int, seed: Optional[torch.Tensor]) -> L.Dropout:
    if p > 0.0 and seed is not None:
        return L.Dropout(float(p), int(salt) & 0xFFFFFFFF, seed.data_ptr())
    return L.Dropout(0.0, 0, None)


def _require_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise L.MtnHipError("mtn_amd operators run on the GPU only (HIP kernels); got a CPU tensor")


def _mask_u8(mask: Optional[torch.Tensor], B: int, a: int, m: int):
    """Reference masks are bool (B|1, 1|a, m) (data_utils.py:34-53).  -> (uint8 tensor, batch stride, row stride).
    The uint8 image is cached on the mask object: the same mask serves every layer (and several streams)."""
    if mask is None:
        return None, 0, 0
    if mask.dim() != 3 or mask.size(-1) != m or mask.size(0) not in (1, B) or mask.size(1) not in (1, a):
        raise ValueError(f"mask {tuple(mask.shape)} does not broadcast to ({B},{a},{m})")
    cached = getattr(mask, "_mtn_u8", None)
    if cached is None:
        cached = mask.to(torch.uint8).contiguous()
        try:
            mask._mtn_u8 = cached
        except Exception:
            pass
    sb = 0 if cached.size(0) == 1 else cached.size(1) * m
    sq = 0 if cached.size(1) == 1 else m
    return cached, sb, sq


def prepare_masks(*masks):
    """Convert masks to their kernel form NOW (on the current stream), before other streams start using them."""
    for mk in masks:
        if isinstance(mk, (list, tuple)):
            prepare_masks(*mk)
        elif mk is not None and getattr(mk, "_mtn_u8", None) is None:
            mk._mtn_u8 = mk.to(torch.uint8).contiguous()


def gemm(dtype: int, problems):
    """problems: list of lib.GemmProblem -> one grouped launch."""
    arr = (L.GemmProblem * len(problems))(*problems)
    L.check(L.load().mtn_gemm(dtype, len(problems), arr, L.stream_ptr()))


def cast_to_lp(x: torch.Tensor, lp_dtype: torch.dtype) -> torch.Tensor:
    _require_cuda(x)
    if lp_dtype == torch.float32:
        return x.contiguous()
    x = x.contiguous()
    out = torch.empty_like(x, dtype=lp_dtype)
    L.check(L.load().mtn_cast_f32_to_lp(L.dtype_code(lp_dtype), x.numel(), x.data_ptr(), out.data_ptr(), L.stream_ptr()))
    return out


# ------------------------------------------------------------------------------------------ deferred parameter gradients
class ParamGradQueue:
    """dW/db GEMMs and LayerNorm gain/bias reductions are off the critical path of backward.  Sublayer backwards
    enqueue them here (problem structs built by the C side, nothing launched) and the queue launches them in a few
    large grouped kernels when the backward pass ends (autograd engine callback) — hundreds of workgroups per launch
    instead of ~250 small launches serialised behind the activation-gradient chain."""

    def __init__(self):
        self.gemm, self.ln, self.keep = [], [], []
        self.embed = []             # deferred embedding-table scatters (EmbedBwdDesc): every table of the step in ONE grouped launch
        self.dtype = None
        self._armed = False
        self.adam = None            # set by FusedAdam.fuse_into(): the next flush applies the optimiser in the GEMM epilogues

    def _attach_adam(self):
        """Optimiser epilogue (include/mtn_hip.h mtn_adam_fuse): every dW problem whose target is (a row block of) a fusable
        sublayer weight updates that weight, its moments and both compute-dtype copies in place instead of storing a gradient.
        Raises unless the fusable weights are covered exactly once — a silent partial update would corrupt training."""
        import bisect
        A = self.adam
        table, starts = A["fusable"], A["starts"]
        esz = A["esz"]
        keep = []
        got = {}                                     # offset of the fusable weight -> elements that received a gradient GEMM
        seen = set()
        for p in self.gemm:
            if not (p.a_trans and p.b_trans and p.out_f32):
                continue
            off = (p.out_f32 - A["grad"]) // 4
            i = bisect.bisect_right(starts, off) - 1
            if i < 0:
                continue
            o, rows, cols = table[i]
            if not (o <= off < o + rows * cols):
                continue
            rel = off - o
            ok = (not p.residual and p.ldc == cols and p.N == cols and rel % cols == 0 and rel // cols + p.M <= rows and off not in seen)
            if not ok:
                raise L.MtnHipError("optimiser epilogue: a parameter-gradient GEMM does not cover its weight block once and whole")
            seen.add(off)
            r0 = rel // cols
            f = L.AdamFuse()
            f.p, f.m, f.v = A["p"] + 4 * off, A["m"] + 4 * off, A["v"] + 4 * off
            f.p_lp = A["lp"] + esz * off if A["lp"] else None
            f.p_lpT = A["lpT"] + esz * (A["t_map"][o] + r0) if (A["lpT"] and o in A["t_map"]) else None     # (compact buffer of the kept copies)
            f.ldT = rows
            f.write_grad = 1 if A["write_grad"] else 0
            f.state, f.grad_scale = A["state"], A["grad_scale"]
            f.beta1, f.beta2, f.eps = A["betas"][0], A["betas"][1], A["eps"]
            p.adam = C.pointer(f)
            keep.append(f)
            got[o] = got.get(o, 0) + p.M * p.N
        covered = set()
        for o, rows, cols in table:
            n = got.get(o, 0)
            if n == rows * cols:
                covered.add(o)
            elif n != 0 or o not in A["optional"]:
                raise L.MtnHipError(f"optimiser epilogue: weight at offset {o} received gradient GEMMs for {n} of {rows * cols} elements")
        A["covered"] = frozenset(covered)
        A["applied"] = True
        return keep

    def _table_aux(self, tt):
        """The rest of the optimiser step as FRONT tiles of the table launch (include/mtn_hip.h mtn_tt_aux), when the optimiser
        epilogue is armed: LayerNorm gains / biases (finalize + Adam per 256 columns), the bias of every Linear whose weight
        gradient is one of the launch's problems (updated by the tile that sums it), and every other range of the flat buffers no dW
        epilogue covers — the embedding tables, whose gradient the scatter launch above has completed — as <= 4096-element chunks.
        Nothing is left behind the launch: FusedAdam.step_rest() then only refreshes transposed copies.  Returns (aux, keep-alive)
        or None (a gradient that does not live in the model's flat buffer)."""
        A = self.adam
        if A is None or not A.get("n_flat"):
            return None
        g0, n_flat = A["grad"], A["n_flat"]
        inside = lambda ptr, n: ptr is not None and g0 <= ptr and ptr + 4 * n <= g0 + 4 * n_flat and (ptr - g0) % 4 == 0
        ln_units, taken = [], []                    # taken: (offset, length) ranges updated inside the launch
        for d_ in self.ln:
            if not (inside(d_.da2, d_.d) and inside(d_.db2, d_.d)):
                return None
            a_off, b_off = (d_.da2 - g0) // 4, (d_.db2 - g0) // 4
            ln_units.append((d_.partial, d_.nparts, d_.d, a_off, b_off))
            taken += [(a_off, d_.d), (b_off, d_.d)]
        for p in tt:
            if p.rowsum_out and inside(p.rowsum_out, p.M):
                taken.append(((p.rowsum_out - g0) // 4, p.M))
            if not p.adam and inside(p.out_f32, 1):
                return None                         # a weight gradient this very launch STORES (no epilogue): not complete when the front tiles run
        for o, r, c in A["fusable"]:
            if o in A["covered"]:
                taken.append((o, r * c))
        taken.sort()
        if any(taken[i][0] + taken[i][1] > taken[i + 1][0] for i in range(len(taken) - 1)):
            return None                             # a gradient with two producers (shared module): keep the separate passes
        key = tuple(taken)
        hit = A["aux_cache"].get(key)
        if hit is None:
            offs, lens, cur = [], [], 0
            for o, n in taken + [(n_flat, 0)]:
                lo, hi = (cur + 3) // 4 * 4, o // 4 * 4            # (every parameter starts on a multiple of 8 elements; paddings are inert)
                while lo < hi:
                    k = min(4096, hi - lo)
                    offs.append(lo); lens.append(k); lo += k
                cur = o + n
            hit = ((C.c_long * max(1, len(offs)))(*offs), (C.c_int * max(1, len(lens)))(*lens), len(offs))
            A["aux_cache"][key] = hit
        ln_arr = (L.TtLnUnit * max(1, len(ln_units)))()
        for i, (partial, nparts, d, a_off, b_off) in enumerate(ln_units):
            ln_arr[i].partial, ln_arr[i].nparts, ln_arr[i].d, ln_arr[i].a_off, ln_arr[i].b_off = partial, nparts, d, a_off, b_off
        aux = L.TtAux()
        aux.p, aux.g, aux.m, aux.v, aux.lp, aux.n_flat = A["p"], g0, A["m"], A["v"], A["lp"], n_flat
        aux.n_ln, aux.ln = len(ln_units), ln_arr
        aux.n_chunks, aux.chunk_off, aux.chunk_len = hit[2], hit[0], hit[1]
        aux.bias_adam = 1
        aux.state, aux.grad_scale = A["state"], A["grad_scale"]
        aux.beta1, aux.beta2, aux.eps = A["betas"][0], A["betas"][1], A["eps"]
        return aux, (ln_arr, hit)

    def add(self, dtype, problems, ln_desc, keep):
        assert self.dtype in (None, dtype)
        self.dtype = dtype
        self.gemm.extend(problems)
        if ln_desc is not None:
            self.ln.append(ln_desc)
        self.keep.extend(keep)
        if not self._armed:
            self._armed = True
            torch.autograd.Variable._execution_engine.queue_callback(self.flush)

    def add_embed(self, descs, keep):
        """Defer embedding-table gradient scatters (mtn_embed_bwd_group) to the flush: the text streams' table and the target
        table are separate autograd nodes, but one grouped launch serves both (one workgroup grid per table)."""
        self.embed.extend(descs)
        self.keep.extend(keep)
        if not self._armed:
            self._armed = True
            torch.autograd.Variable._execution_engine.queue_callback(self.flush)

    def reset(self):
        """Drop everything queued and disarm.  A backward pass that raises never reaches the engine's final callbacks, so the
        queue would stay armed with stale problems and no later backward would register a flush: the step's error path and
        the start of every step call this."""
        self.gemm, self.ln, self.keep, self.embed = [], [], [], []
        self._armed = False
        self.adam = None

    def flush(self):
        self._armed = False
        if not self.gemm and not self.ln and not self.embed:
            return
        lib = L.load()
        cur = torch.cuda.current_stream()
        for i in range(0, len(self.embed), 8):            # (MTN_LN_MAX_GROUP descriptors per launch)
            chunk = self.embed[i:i + 8]
            arr = (L.EmbedBwdDesc * len(chunk))(*chunk)
            L.check(lib.mtn_embed_bwd_group(len(chunk), arr, cur.cuda_stream))
        self.embed = []
        if not self.gemm and not self.ln:
            self.keep = []
            return
        for t in self.keep:
            t.record_stream(cur)
        adam_keep = self._attach_adam() if self.adam is not None else None      # noqa: F841 (descriptors live until the launches)
        # a grouped launch lasts as long as its longest contraction: keep the long ones (memories: K = B*m rows) together
        self.gemm.sort(key=lambda p: -p.K)
        if self.dtype == L.MTN_BF16:
            # ALL parameter-gradient problems in one launch of 128x128 tiles (csrc/gemm.hip, table form), long and short
            # contractions side by side: no launch boundaries or partial rounds (296 vs 430 us at cfg2), and with the optimiser
            # epilogue the tiles' streaming phases overlap other tiles' contractions.  Without the epilogue only when the
            # problems fill 128-wide tiles (tiny test models keep the 64-wide kernels).
            tt = [p for p in self.gemm if p.a_trans and p.b_trans and p.M % 8 == 0 and p.N % 8 == 0 and not p.residual]
            big = all(p.M >= 128 and p.N >= 128 for p in tt) and sum(((p.M + 127) // 128) * ((p.N + 127) // 128) for p in tt) >= 192
            if tt and len(tt) <= 1024 and (self.adam is not None or big):
                order, lo, hi = [], 0, len(tt) - 1
                while lo <= hi:
                    order.append(tt[lo]); lo += 1
                    if lo <= hi:
                        order.append(tt[hi]); hi -= 1
                arr = (L.GemmProblem * len(order))(*order)
                rest = [p for p in self.gemm if id(p) not in set(id(q) for q in tt)]
                aux = self._table_aux(tt) if (self.adam is not None and not rest) else None
                if aux is not None:
                    L.check(lib.mtn_gemm_tt_table_aux(self.dtype, len(order), arr, C.byref(aux[0]), cur.cuda_stream))
                    self.adam["rest_done"] = True          # LayerNorm finalize + every remaining Adam update ran as front tiles
                    self.ln = []
                else:
                    L.check(lib.mtn_gemm_tt_table(self.dtype, len(order), arr, cur.cuda_stream))
                self.gemm = rest
        # ... and at most 512 of the 128x128 tiles (two resident workgroups per CU x 256 CUs) per launch: a launch that
        # spills into a second round pays for a whole extra round
        chunk, tiles = [], 0
        for p in self.gemm + [None]:
            t = 0 if p is None else ((p.M + 127) // 128) * ((p.N + 127) // 128)
            if chunk and (p is None or len(chunk) == L.GEMM_MAX_GROUP or tiles + t > 512):
                arr = (L.GemmProblem * len(chunk))(*chunk)
                L.check(lib.mtn_gemm(self.dtype, len(chunk), arr, cur.cuda_stream))
                chunk, tiles = [], 0
            if p is not None:
                chunk.append(p); tiles += t
        if self.ln:
            arr = (L.LnFinalizeDesc * len(self.ln))(*self.ln)
            L.check(lib.mtn_layernorm_bwd_finalize(len(self.ln), arr, cur.cuda_stream))
        self.gemm, self.ln, self.keep = [], [], []


# ------------------------------------------------------------------------------------------ gradient protocols
class GradMeet:
    """Where the gradients of a tensor with several consumers meet: one fp32 buffer instead of autograd adds.  It rides on the
    tensor as `_mtn_gacc`.  Every consumer joins in forward; in backward each settles once, in autograd's order: as an INPUT
    (`settle`: its dx becomes the buffer, or is added to it after the launch) or as an attention MEMORY (`buffer`: the dmem GEMM
    writes or accumulates in place).  The last to settle returns the sum to autograd; everyone before returns nothing."""
    __slots__ = ("buf", "remaining")

    def __init__(self):
        self.buf, self.remaining = None, 0

    @staticmethod
    def join(t, create=False):
        """forward: one more consumer of `t` -> its meeting point (None when nobody opened one and `create` is off)."""
        g = getattr(t, "_mtn_gacc", None)
        if g is None and create:
            g = t._mtn_gacc = GradMeet()
        if g is not None:
            g.remaining += 1
        return g

    def settle(self, dx, later):
        """backward, input role.  -> what this consumer returns to autograd.  An addition into the buffer has to wait until dx is
        written: it is appended to `later` as (buffer, dx), for the caller to run after its launch, in order."""
        self.remaining -= 1
        if self.buf is None:
            if self.remaining > 0:
                self.buf = dx                  # first writer: the others accumulate into our dx
                return None
            return dx                          # nobody else came
        buf = self.buf
        later.append((buf, dx))
        if self.remaining > 0:
            return None
        self.buf = None
        return buf

    def buffer(self, shape, device):
        """backward, memory role.  -> (buffer, accumulate, last): write the gradient to `buffer` (accumulate = 0) or add it there
        (1); `last`: the sum is complete with this write, return it to autograd."""
        accumulate = int(self.buf is not None)
        if self.buf is None:
            self.buf = torch.empty(shape, device=device, dtype=torch.float32)
        buf = self.buf
        self.remaining -= 1
        if self.remaining == 0:
            self.buf = None
        return buf, accumulate, self.remaining == 0

    def seed(self, grad, shape):
        """A gradient that arrives from outside the graph (a leaf's .grad across a layer cut) takes the first writer's place.
        -> whether it was taken (then it must not go to autograd as well)."""
        if self.remaining > 0 and self.buf is None and grad.is_contiguous() and grad.dtype == torch.float32 and grad.shape == shape:
            self.buf = grad
            return True
        return False


def _out_site(cfg):
    """(p, salt, seed) of the dropout on a sublayer's output (mtn.py:127): the site of its own kernels and of its HandOff."""
    return cfg.p_out, cfg.salt * 4 + 1, cfg.seed


class HandOff:
    """A sublayer's dy, delivered by whoever computes it: the consumer of the sublayer's output writes its dx once more, through
    the PRODUCER's output dropout (p, salt, seed) and in the producer's compute dtype (lp), so the producer's backward starts
    without a cast launch (include/mtn_hip.h: dyl_ready / next_dyl).  It rides on the output tensor as `_mtn_next`."""
    __slots__ = ("p", "salt", "seed", "lp", "dyl", "dx_ptr", "ver", "shape")

    def __init__(self, p, salt, seed, lp):
        self.p, self.salt, self.seed, self.lp = p, salt, seed, lp
        self.dyl = self.dx_ptr = self.ver = self.shape = None

    @classmethod
    def of(cls, cfg):
        return cls(*_out_site(cfg), cfg.lp_dtype)

    def drop(self) -> L.Dropout:
        return _drop(self.p, self.salt, self.seed)

    def offer(self, dx, dtype):
        """consumer: -> the tensor its kernels fill with dropout-masked dx in `dtype`; remembers which dx that copy stands for."""
        self.dyl = torch.empty(dx.shape, device=dx.device, dtype=dtype)
        self.dx_ptr, self.ver, self.shape = dx.data_ptr(), dx._version, dx.shape
        return self.dyl

    def claim(self, dy):
        """producer: -> the offered copy if `dy` IS the dx it was made from, untouched, else None; the offer ends either way.
        Valid only with the same storage address, the same shape and the version counter dx had: autograd sums gradients in
        place with add_, which bumps it; any tensor derived from dx — a sum, a clone — is allocated while dx is still alive, so
        it cannot sit at dx's address.  The dx tensor itself is not held: a leaf's .grad may then take it over without a copy
        (layer-segmented backward)."""
        ok = self.dyl is not None and self.dx_ptr == dy.data_ptr() and self.ver == dy._version and tuple(self.shape) == tuple(dy.shape)
        ready, self.dyl, self.dx_ptr = (self.dyl if ok else None), None, None
        return ready

    def withdraw(self, ptr):
        """The tensor at `ptr` is about to be accumulated into outside autograd's sight: an offer made for it ends."""
        if self.dx_ptr == ptr:
            self.dyl = self.dx_ptr = None


# ------------------------------------------------------------------------------------------ LayerNorm
class LayerNormFn(torch.autograd.Function):
    """mtn.py:111-114.  Returns (y_f32, y_lp); y_lp (compute dtype copy for GEMM operands) is non-differentiable."""

    @staticmethod
    def forward(ctx, x, a2, b2, eps, lp_dtype, grad_a, grad_b, queue=None):
        _require_cuda(x, a2, b2)
        x = x.contiguous()
        d = x.size(-1)
        rows = x.numel() // d
        y = torch.empty_like(x)
        want_lp = lp_dtype is not None and lp_dtype != torch.float32
        y_lp = torch.empty_like(x, dtype=lp_dtype) if want_lp else None
        mean = torch.empty(rows, device=x.device, dtype=torch.float32)
        rstd = torch.empty_like(mean)
        code = L.dtype_code(lp_dtype) if want_lp else L.MTN_F32
        L.check(L.load().mtn_layernorm_fwd(code, rows, d, eps, x.data_ptr(), a2.data_ptr(), b2.data_ptr(), y.data_ptr(),
                                           L.ptr(y_lp), mean.data_ptr(), rstd.data_ptr(), L.stream_ptr()))
        ctx.save_for_backward(x, a2, mean, rstd)
        ctx.eps, ctx.grad_a, ctx.grad_b, ctx.queue = eps, grad_a, grad_b, queue
        if y_lp is None:
            y_lp = torch.empty(0, device=x.device, dtype=torch.float32)   # placeholder second output
        ctx.mark_non_differentiable(y_lp)
        return y, y_lp

    @staticmethod
    def backward(ctx, g, _g_lp):
        x, a2, mean, rstd = ctx.saved_tensors
        d = x.size(-1)
        rows = x.numel() // d
        g = g.contiguous()
        lib = L.load()
        dx = torch.empty_like(x)
        da = ctx.grad_a if ctx.grad_a is not None else torch.empty_like(a2)
        db = ctx.grad_b if ctx.grad_b is not None else torch.empty_like(a2)
        partial = torch.empty(lib.mtn_layernorm_bwd_partial_floats(rows, d), device=x.device, dtype=torch.float32)
        defer = ctx.queue is not None and ctx.grad_a is not None
        L.check(lib.mtn_layernorm_bwd(rows, d, ctx.eps, x.data_ptr(), a2.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                      g.data_ptr(), None, dx.data_ptr(), None if defer else da.data_ptr(),
                                      None if defer else db.data_ptr(), partial.data_ptr(), L.stream_ptr()))
        if defer:
            desc = L.LnFinalizeDesc(partial.data_ptr(), lib.mtn_layernorm_bwd_nparts(rows), d, da.data_ptr(), db.data_ptr())
            ctx.queue.add(None if ctx.queue.dtype is None else ctx.queue.dtype, [], desc, [partial])
        ret_a = None if ctx.grad_a is not None else da
        ret_b = None if ctx.grad_b is not None else db
        return dx, ret_a, ret_b, None, None, None, None, None


class LayerNormGroupFn(torch.autograd.Function):
    """Several independent LayerNorms (mtn.py:111-114; the decoder's final norms, mtn.py:164) in ONE launch each way.
    spec: norms = [(a2, b2, eps, grad_a, grad_b)] (grad_* = fp32 destinations or None), lp_dtype, queue.  With a compute dtype the
    outputs also go, in order, to consecutive row ranges of one buffer (spec['_lp_rows'], [sum rows, d]) — the operand of the
    loss head's GEMM, which then needs no cast launch.  Parameter gradients are written to grad_* (deferred through the queue)
    or, without destinations, returned through autograd as usual."""

    @staticmethod
    def forward(ctx, spec, *tensors):
        lib = L.load()
        n = len(spec["norms"])
        xs = [t.contiguous() for t in tensors[:n]]
        _require_cuda(*xs)
        dev = xs[0].device
        lp = spec["lp_dtype"]
        want_lp = lp is not None and lp != torch.float32
        code = L.dtype_code(lp) if want_lp else L.MTN_F32
        d = xs[0].size(-1)
        rows = [x.numel() // d for x in xs]
        y_lp = torch.empty(sum(rows), d, device=dev, dtype=lp) if want_lp else None
        descs = (L.LnFwdDesc * n)()
        ys, saved, off = [], [], 0
        for i, (x, (a2, b2, eps, _ga, _gb)) in enumerate(zip(xs, spec["norms"])):
            y = torch.empty_like(x)
            mean = torch.empty(rows[i], device=dev, dtype=torch.float32)
            rstd = torch.empty_like(mean)
            D = descs[i]
            D.rows, D.d, D.eps, D.x, D.a2, D.b2 = rows[i], d, eps, x.data_ptr(), a2.data_ptr(), b2.data_ptr()
            D.y_f32, D.y_lp, D.mean, D.rstd = y.data_ptr(), (y_lp[off:].data_ptr() if want_lp else None), mean.data_ptr(), rstd.data_ptr()
            ys.append(y)
            saved.append((x, mean, rstd))
            off += rows[i]
        L.check(lib.mtn_layernorm_fwd_group(code, n, descs, L.stream_ptr()))
        spec["_lp_rows"] = y_lp
        ctx.spec, ctx.saved, ctx.rows, ctx.d = spec, saved, rows, d
        # gradient hand-off (HandOff): the sublayer that produced an input wants dx once more, through ITS output dropout, in the
        # compute dtype
        ctx.feeds = [getattr(t, "_mtn_next", None) for t in tensors[:n]]
        # an input that a sublayer attends as memory too (the last layer's auto-encoder outputs): the two gradients meet in one
        # buffer (GradMeet) instead of an autograd add
        ctx.xaccs = [GradMeet.join(t) if (_XACC and t.requires_grad) else None for t in tensors[:n]]
        return tuple(ys)

    @staticmethod
    def backward(ctx, *gs):
        lib = L.load()
        spec, saved, rows, d = ctx.spec, ctx.saved, ctx.rows, ctx.d
        n = len(saved)
        queue = spec.get("queue")
        descs = (L.LnBwdDesc * n)()
        dxs, finals, keep, rets = [], [], [], []
        for i, ((x, mean, rstd), (a2, _b2, eps, ga, gb)) in enumerate(zip(saved, spec["norms"])):
            g = gs[i].contiguous() if gs[i] is not None else torch.zeros_like(x)
            dx = torch.empty_like(x)
            partial = torch.empty(lib.mtn_layernorm_bwd_partial_floats(rows[i], d), device=x.device, dtype=torch.float32)
            B_ = descs[i]
            B_.rows, B_.d, B_.eps, B_.x, B_.a2, B_.mean, B_.rstd = rows[i], d, eps, x.data_ptr(), a2.data_ptr(), mean.data_ptr(), rstd.data_ptr()
            B_.g, B_.dx, B_.partial = g.data_ptr(), dx.data_ptr(), partial.data_ptr()
            f = ctx.feeds[i]
            if f is not None and f.lp is not None and f.lp != torch.float32 and ctx.xaccs[i] is None:   # (a shared gradient buffer is not final here)
                nxt = f.offer(dx, f.lp)
                B_.dx_lp, B_.dx_lp_dtype, B_.dx_lp_drop = nxt.data_ptr(), L.dtype_code(f.lp), f.drop()
                keep.append(nxt)
            da = ga if ga is not None else torch.empty_like(a2)
            db = gb if gb is not None else torch.empty_like(a2)
            finals.append((L.LnFinalizeDesc(partial.data_ptr(), lib.mtn_layernorm_bwd_nparts(rows[i]), d, da.data_ptr(), db.data_ptr()), partial, ga is not None))
            rets.append((None if ga is not None else da, None if gb is not None else db))
            dxs.append(dx)
            keep += [g, partial]
        L.check(lib.mtn_layernorm_bwd_group(n, descs, L.stream_ptr()))
        post = []
        for i, xg in enumerate(ctx.xaccs):
            if xg is not None:
                dxs[i] = xg.settle(dxs[i], post)
        for buf, dxp in post:
            buf.add_(dxp)
        now = []
        for desc, partial, has_dest in finals:
            if queue is not None and has_dest:
                queue.add(queue.dtype, [], desc, [partial])
            else:
                now.append(desc)
        if now:
            L.check(lib.mtn_layernorm_bwd_finalize(len(now), (L.LnFinalizeDesc * len(now))(*now), L.stream_ptr()))
        ctx.keep = keep
        return (None,) + tuple(dxs) + tuple(r[0] for r in rets) + tuple(r[1] for r in rets)


def layer_norm_group(xs, modules):
    """-> [y_i fp32] for independent LayerNorm modules (mtn_amd.mtn.LayerNorm) in one launch; each output carries
    `_mtn_lp_rows = (buffer, first row, rows)`: its compute-dtype copy inside one [sum rows, d] buffer (None in fp32 mode)."""
    spec = dict(norms=[(m.a_2, m.b_2, m.eps) + (tuple(m._grads) if m._grads is not None else (None, None)) for m in modules],
                lp_dtype=modules[0]._lp_dtype, queue=modules[0]._queue)
    params = [m.a_2 for m in modules] + [m.b_2 for m in modules]        # autograd inputs (gradients returned when no destination is set)
    ys = LayerNormGroupFn.apply(spec, *xs, *params)
    buf, off = spec.get("_lp_rows"), 0
    for y in ys:
        r = y.numel() // y.size(-1)
        if buf is not None:
            y._mtn_lp_rows = (buf, off, r)
        off += r
    return list(ys)


def layer_norm(x, a2, b2, eps=1e-6, lp_dtype=None, grad_a=None, grad_b=None, queue=None):
    """-> (y fp32, y in the compute dtype).  grad_a/grad_b: optional fp32 destinations for da2/db2."""
    y, y_lp = LayerNormFn.apply(x, a2, b2, eps, lp_dtype, grad_a, grad_b, queue)
    if y_lp.numel() == 0 and y.numel() != 0:
        y_lp = y.detach()
    return y, y_lp


# ------------------------------------------------------------------------------------------ sublayers
@dataclass
class MhaConfig:
    heads: int
    eps: float = 1e-6
    p_attn: float = 0.0           # dropout on softmax probabilities (mtn.py:230)
    p_out: float = 0.0            # dropout on the sublayer output (mtn.py:127)
    salt: int = 0                 # unique per sublayer: sites salt*4+{0,1}
    seed: Optional[torch.Tensor] = None          # device int64[1], advanced once per step
    lp_dtype: torch.dtype = torch.bfloat16
    w_qkv_lp: Optional[torch.Tensor] = None      # compute-dtype copies of the weights ([3d,d], [d,d])
    w_o_lp: Optional[torch.Tensor] = None
    w_qkv_lpT: Optional[torch.Tensor] = None     # transposed compute-dtype copies (backward dX on the LDS-DMA GEMM path)
    w_o_lpT: Optional[torch.Tensor] = None
    grads: Optional[dict] = None                 # fp32 destinations: ln_a ln_b w_qkv b_qkv w_o b_o (flat-grad views)
    queue: Optional[ParamGradQueue] = None       # defer dW/db/LN-parameter work to the end of backward
    ln_fold: Optional[torch.Tensor] = None       # fold vectors of w_qkv behind the sublayer's LayerNorm (mtn_ln_fold), float [2K]


@dataclass
class FfnConfig:
    eps: float = 1e-6
    p_hidden: float = 0.0         # mtn.py:280
    p_out: float = 0.0            # mtn.py:127
    salt: int = 0
    seed: Optional[torch.Tensor] = None
    lp_dtype: torch.dtype = torch.bfloat16
    w1_lp: Optional[torch.Tensor] = None
    w2_lp: Optional[torch.Tensor] = None
    w1_lpT: Optional[torch.Tensor] = None
    w2_lpT: Optional[torch.Tensor] = None
    grads: Optional[dict] = None  # ln_a ln_b w1 b1 w2 b2
    queue: Optional[ParamGradQueue] = None
    ln_fold: Optional[torch.Tensor] = None        # fold vectors of w1 (mtn_ln_fold), float [2 d_ff]


# The argument structs (L.MhaArgs / L.FfnArgs) are filled HERE and nowhere else: the fields both kinds share by `_pack_fwd` /
# `_pack_bwd`, the rest by one packer per struct and direction.  A forward packer allocates what the sublayer saves and returns
# (y, sv): the output and everything backward needs, kept alive beside the struct; a backward packer completes the SAME struct.
# The single-sublayer Functions and SublayerGroupFn are both callers (one member / several), so a new field is threaded once.
def _pack_fwd(A, cfg, x, ln_a, ln_b):
    d = x.size(-1)
    rows = x.numel() // d
    y = torch.empty_like(x)
    xn = torch.empty(rows, d, device=x.device, dtype=cfg.lp_dtype)
    mean = torch.empty(rows, device=x.device, dtype=torch.float32)
    rstd = torch.empty_like(mean)
    A.ln_eps, A.drop_out = cfg.eps, _drop(*_out_site(cfg))
    A.x, A.ln_a, A.ln_b = x.data_ptr(), ln_a.data_ptr(), ln_b.data_ptr()
    A.y, A.xn, A.mean, A.rstd = y.data_ptr(), xn.data_ptr(), mean.data_ptr(), rstd.data_ptr()
    A.ln_fold = L.ptr(cfg.ln_fold)              # (read by backward only, like the transposed weights: csrc/sublayer.hip)
    return y, dict(x=x, xn=xn, mean=mean, rstd=rstd)


def _pack_mha_fwd(A, cfg: MhaConfig, x, mem, mem_lp, mask, params, w_qkv=None, w_o=None, kv_ready=None):
    """params = (ln_a, ln_b, b_qkv, b_o); w_qkv / w_o (fp32) are cast where cfg carries no compute-dtype copies; kv_ready: K|V of
    the memory, projected ahead (project_memories)."""
    ln_a, ln_b, b_qkv, b_o = params
    B, a, d = x.shape
    self_attn = mem is None
    m = a if self_attn else mem.size(1)
    lp, dev = cfg.lp_dtype, x.device
    if not self_attn and mem_lp is None:
        mem_lp = cast_to_lp(mem, lp)
    w_qkv_lp = cfg.w_qkv_lp if cfg.w_qkv_lp is not None else cast_to_lp(w_qkv, lp)
    w_o_lp = cfg.w_o_lp if cfg.w_o_lp is not None else cast_to_lp(w_o, lp)
    mask_u8, sb, sq = _mask_u8(mask, B, a, m)
    y, sv = _pack_fwd(A, cfg, x, ln_a, ln_b)
    qkv = torch.empty(B * a, 3 * d if self_attn else d, device=dev, dtype=lp)
    kv = None if self_attn else (kv_ready if kv_ready is not None else torch.empty(B * m, 2 * d, device=dev, dtype=lp))
    o = torch.empty(B * a, d, device=dev, dtype=lp)
    lse = torch.empty(2 * B * cfg.heads * a, device=dev, dtype=torch.float32)
    A.B, A.a, A.m, A.d, A.h, A.self_attn = B, a, m, d, cfg.heads, int(self_attn)
    A.drop_attn = _drop(cfg.p_attn, cfg.salt * 4 + 0, cfg.seed)
    A.mem, A.mask, A.mask_sb, A.mask_sq = L.ptr(mem_lp), L.ptr(mask_u8), sb, sq
    A.w_qkv, A.b_qkv, A.w_o, A.b_o = w_qkv_lp.data_ptr(), b_qkv.data_ptr(), w_o_lp.data_ptr(), b_o.data_ptr()
    A.w_qkv_t, A.w_o_t = L.ptr(cfg.w_qkv_lpT), L.ptr(cfg.w_o_lpT)
    A.qkv, A.kv, A.o, A.lse = qkv.data_ptr(), L.ptr(kv), o.data_ptr(), lse.data_ptr()
    A.kv_ready = int((not self_attn) and kv_ready is not None)
    sv.update(mem_lp=mem_lp, mask=mask_u8, qkv=qkv, kv=kv, o=o, lse=lse, need_dmem=(not self_attn) and mem.requires_grad,
              like=dict(ln_a=ln_a, ln_b=ln_b, w_qkv=w_qkv_lp, b_qkv=b_qkv, w_o=w_o_lp, b_o=b_o))
    return y, sv


def _pack_ffn_fwd(A, cfg: FfnConfig, x, params, w1=None, w2=None, want_lp=False):
    """params = (ln_a, ln_b, b1, b2); want_lp: the output also leaves in the compute dtype (sv['y_lp'])."""
    ln_a, ln_b, b1, b2 = params
    lp = cfg.lp_dtype
    w1_lp = cfg.w1_lp if cfg.w1_lp is not None else cast_to_lp(w1, lp)
    w2_lp = cfg.w2_lp if cfg.w2_lp is not None else cast_to_lp(w2, lp)
    y, sv = _pack_fwd(A, cfg, x, ln_a, ln_b)
    A.rows, A.d, A.d_ff = sv["xn"].size(0), x.size(-1), w1_lp.size(0)
    hid = torch.empty(A.rows, A.d_ff, device=x.device, dtype=lp)
    y_lp = torch.empty(y.shape, device=x.device, dtype=lp) if want_lp and lp != torch.float32 else None
    A.drop_hidden = _drop(cfg.p_hidden, cfg.salt * 4 + 2, cfg.seed)
    A.w1, A.b1, A.w2, A.b2 = w1_lp.data_ptr(), b1.data_ptr(), w2_lp.data_ptr(), b2.data_ptr()
    A.w1_t, A.w2_t = L.ptr(cfg.w1_lpT), L.ptr(cfg.w2_lpT)
    A.hid, A.y_lp = hid.data_ptr(), L.ptr(y_lp)
    sv.update(hid=hid, y_lp=y_lp, like=dict(ln_a=ln_a, ln_b=ln_b, w1=w1_lp, b1=b1, w2=w2_lp, b2=b2))
    return y, sv


def _dests(cfg, sv):
    """fp32 destinations of the parameter gradients: the caller's (cfg.grads), else fresh ones to return through autograd."""
    if cfg.grads is not None:
        return cfg.grads
    return {k: torch.empty(t.shape, device=t.device, dtype=torch.float32) for k, t in sv["like"].items()}


def _ffn_bwd_ws_lp_elems(rows, d, ff):
    return rows * d + rows * ff               # dyl [rows,d] | dh [rows,d_ff] (csrc/sublayer.hip ffn_ws)


def _pack_bwd(A, cfg, dy, dx, g, ws_lp_elems, ws_f32_floats, defer, ready, nxt):
    """ready: this sublayer's dy, already through its output dropout in the compute dtype (HandOff.claim); nxt: the HandOff of the
    sublayer that produced our input, on which our dx has just been offered.  -> tensors the deferred work reads."""
    ws_lp = torch.empty(ws_lp_elems, device=dx.device, dtype=cfg.lp_dtype)
    ws_f32 = torch.empty(ws_f32_floats, device=dx.device, dtype=torch.float32)
    A.dy, A.dx, A.d_ln_a, A.d_ln_b = dy.data_ptr(), dx.data_ptr(), g["ln_a"].data_ptr(), g["ln_b"].data_ptr()
    A.ws_lp, A.ws_f32, A.defer_param_grads = ws_lp.data_ptr(), ws_f32.data_ptr(), int(defer)
    A.dyl_ready, A.next_dyl = L.ptr(ready), L.ptr(nxt.dyl if nxt is not None else None)
    if nxt is not None:
        A.next_drop = nxt.drop()
    return [dy, ws_lp, ws_f32] + ([ready] if ready is not None else [])


def _pack_mha_bwd(A, cfg, sv, dy, dx, g, defer, dmem=None, accumulate=0, mem_nxt=None, ready=None, nxt=None):
    """dmem: fp32 destination of the memory's gradient (added to when `accumulate`); mem_nxt: the HandOff of the memory's producer,
    on which dmem has just been offered."""
    lib = L.load()
    B, a, m, d = A.B, A.a, A.m, A.d
    keep = _pack_bwd(A, cfg, dy, dx, g, lib.mtn_mha_bwd_ws_lp_elems(B, a, m, d, A.self_attn), lib.mtn_mha_bwd_ws_f32_floats(B, a, m, d),
                     defer, ready, nxt)
    A.dmem, A.dmem_accumulate = L.ptr(dmem), accumulate
    A.dmem_lp = L.ptr(mem_nxt.dyl if mem_nxt is not None else None)
    if mem_nxt is not None:
        A.dmem_lp_drop = mem_nxt.drop()
    A.d_w_qkv, A.d_b_qkv, A.d_w_o, A.d_b_o = g["w_qkv"].data_ptr(), g["b_qkv"].data_ptr(), g["w_o"].data_ptr(), g["b_o"].data_ptr()
    return keep + [sv["o"], sv["xn"]] + ([sv["mem_lp"]] if sv["mem_lp"] is not None else [])


def _pack_ffn_bwd(A, cfg, sv, dy, dx, g, defer, ready=None, nxt=None):
    rows, d, ff = A.rows, A.d, A.d_ff
    keep = _pack_bwd(A, cfg, dy, dx, g, _ffn_bwd_ws_lp_elems(rows, d, ff), L.load().mtn_ffn_bwd_ws_f32_floats(rows, d, ff), defer, ready, nxt)
    A.d_w1, A.d_b1, A.d_w2, A.d_b2 = g["w1"].data_ptr(), g["b1"].data_ptr(), g["w2"].data_ptr(), g["b2"].data_ptr()
    return keep + [sv["hid"], sv["xn"]]


def _queue_param_grads(queue, code, A, keep):
    """The dW/db GEMM problems and the LayerNorm finalize of one backward-packed struct -> the queue (nothing launched)."""
    lib = L.load()
    work = lib.mtn_mha_param_grad_work if isinstance(A, L.MhaArgs) else lib.mtn_ffn_param_grad_work
    probs = (L.GemmProblem * 3)()
    ln = L.LnFinalizeDesc()
    n = work(code, C.byref(A), probs, C.byref(ln))
    queue.add(code, [probs[i] for i in range(n)], ln, keep)


class MHASublayerFn(torch.autograd.Function):
    """y = x + dropout(MHA(LN(x), mem, mem, mask)).  mem=None -> self-attention (key=value=LN(x), mtn.py:183,209).
    Parameter gradients: returned through autograd (cfg.grads None), written at once to cfg.grads, or, with cfg.queue, deferred."""

    @staticmethod
    def forward(ctx, x, mem, mem_lp, mask, ln_a, ln_b, w_qkv, b_qkv, w_o, b_o, cfg: MhaConfig):
        _require_cuda(x, mem, ln_a, w_qkv)
        ctx.cfg, ctx.args = cfg, L.MhaArgs()
        y, ctx.sv = _pack_mha_fwd(ctx.args, cfg, x.contiguous(), mem, mem_lp, mask, (ln_a, ln_b, b_qkv, b_o), w_qkv, w_o)
        L.check(L.load().mtn_mha_sublayer_fwd(L.dtype_code(cfg.lp_dtype), C.byref(ctx.args), L.stream_ptr()))
        return y

    @staticmethod
    def backward(ctx, dy):
        cfg, A, sv = ctx.cfg, ctx.args, ctx.sv
        code = L.dtype_code(cfg.lp_dtype)
        dx = torch.empty_like(sv["x"])
        dmem = torch.empty(A.B, A.m, A.d, device=dx.device, dtype=torch.float32) if sv["need_dmem"] else None
        g = _dests(cfg, sv)
        defer = cfg.grads is not None and cfg.queue is not None
        keep = _pack_mha_bwd(A, cfg, sv, dy.contiguous(), dx, g, defer, dmem)
        L.check(L.load().mtn_mha_sublayer_bwd(code, C.byref(A), L.stream_ptr()))
        if defer:
            _queue_param_grads(cfg.queue, code, A, keep)
        if cfg.grads is not None:
            return dx, dmem, None, None, None, None, None, None, None, None, None
        return dx, dmem, None, None, g["ln_a"], g["ln_b"], g["w_qkv"], g["b_qkv"], g["w_o"], g["b_o"], None


class FFNSublayerFn(torch.autograd.Function):
    """y = x + dropout(w_2(dropout(relu(w_1 LN(x))))).  Parameter gradients as for MHASublayerFn."""

    @staticmethod
    def forward(ctx, x, ln_a, ln_b, w1, b1, w2, b2, cfg: FfnConfig):
        _require_cuda(x, ln_a, w1)
        ctx.cfg, ctx.args = cfg, L.FfnArgs()
        y, ctx.sv = _pack_ffn_fwd(ctx.args, cfg, x.contiguous(), (ln_a, ln_b, b1, b2), w1, w2)
        L.check(L.load().mtn_ffn_sublayer_fwd(L.dtype_code(cfg.lp_dtype), C.byref(ctx.args), L.stream_ptr()))
        return y

    @staticmethod
    def backward(ctx, dy):
        cfg, A, sv = ctx.cfg, ctx.args, ctx.sv
        code = L.dtype_code(cfg.lp_dtype)
        dx = torch.empty_like(sv["x"])
        g = _dests(cfg, sv)
        defer = cfg.grads is not None and cfg.queue is not None
        keep = _pack_ffn_bwd(A, cfg, sv, dy.contiguous(), dx, g, defer)
        L.check(L.load().mtn_ffn_sublayer_bwd(code, C.byref(A), L.stream_ptr()))
        if defer:
            _queue_param_grads(cfg.queue, code, A, keep)
        if cfg.grads is not None:
            return dx, None, None, None, None, None, None, None
        return dx, g["ln_a"], g["ln_b"], g["w1"], g["b1"], g["w2"], g["b2"], None


# ------------------------------------------------------------------------------------------ lockstep sublayer groups
@dataclass
class GroupMember:
    """One sublayer of a lockstep group.  kind 'mha': params = (ln_a, ln_b, b_qkv, b_o), cfg = MhaConfig with the compute-dtype
    weights and `grads` destinations set; kind 'ffn': params = (ln_a, ln_b, b1, b2), cfg = FfnConfig likewise."""
    kind: str
    cfg: object
    params: tuple
    mask: Optional[torch.Tensor] = None
    mem_lp: Optional[torch.Tensor] = None
    # gradient hand-off along a chain of sublayers (HandOff; include/mtn_hip.h, dyl_ready / next_dyl): `holder` travels with this
    # member's OUTPUT tensor to the sublayer that consumes it; `feeds` is the holder found on this member's INPUT tensor.
    holder: Optional[HandOff] = None
    feeds: Optional[HandOff] = None
    kv_ready: Optional[torch.Tensor] = None     # K|V of a constant memory, projected ahead of the layer loop (project_memories)
    want_lp: bool = False                       # 'ffn': also write the output in the compute dtype (-> out_lp): it is attended as raw memory
    out_lp: Optional[torch.Tensor] = None


class SublayerGroupFn(torch.autograd.Function):
    """Independent sublayers of one DecoderLayer executed in lockstep (one grouped launch per stage, see csrc/sublayer.hip).
    apply(members, x_0, mem_0, x_1, mem_1, ...) -> (y_0, y_1, ...); mem_i is None for self-attention / FFN members.
    Parameter gradients go straight to cfg.grads (flat gradient buffer) through cfg.queue (always deferred)."""

    @staticmethod
    def forward(ctx, members, *tensors):
        xs = [t.contiguous() for t in tensors[0::2]]
        _require_cuda(*xs)
        code = L.dtype_code(members[0].cfg.lp_dtype)
        n_mha = sum(1 for m in members if m.kind == "mha")
        n_ffn = len(members) - n_mha
        mha_args = (L.MhaArgs * max(1, n_mha))()
        ffn_args = (L.FfnArgs * max(1, n_ffn))()
        # an input that an EARLIER sublayer already attends as memory (an auto-encoder output feeds the next layer's chain
        # and is the memory of x's attention): both gradients meet in one buffer instead of an autograd add
        xaccs = [GradMeet.join(t) if (_XACC and t.requires_grad) else None for t in tensors[0::2]]     # (grad mode is off inside forward)
        slots = {"mha": iter(mha_args), "ffn": iter(ffn_args)}
        args, saved, ys = [], [], []
        for mem_t, x, mb in zip(tensors[1::2], xs, members):
            A = next(slots[mb.kind])
            if mb.kind == "mha":
                y, sv = _pack_mha_fwd(A, mb.cfg, x, mem_t, mb.mem_lp, mb.mask, mb.params, kv_ready=mb.kv_ready)
                if sv["need_dmem"]:          # a memory serves every layer: its gradient is accumulated in place by the dmem GEMMs
                    sv["gacc"] = GradMeet.join(mem_t, create=True)
                    sv["mem_next"] = getattr(mem_t, "_mtn_next", None)     # the memory's producer (hand-off holder)
            else:
                y, sv = _pack_ffn_fwd(A, mb.cfg, x, mb.params, want_lp=mb.want_lp)
                mb.out_lp = sv["y_lp"]
            args.append(A); saved.append(sv); ys.append(y)
        L.check(L.load().mtn_sublayer_group_fwd(code, n_mha, mha_args, n_ffn, ffn_args, L.stream_ptr()))
        ctx.members, ctx.saved_bufs, ctx.code, ctx.xaccs = members, saved, code, xaccs
        ctx.args, ctx.mha_args, ctx.ffn_args, ctx.n_mha, ctx.n_ffn = args, mha_args, ffn_args, n_mha, n_ffn
        return tuple(ys)

    @staticmethod
    def backward(ctx, *dys):
        code = ctx.code
        queue = ctx.members[0].cfg.queue
        grads_out, work = [], []
        post = []                    # (buffer, dx) pairs to sum after the launch: input-role accumulators that were not first
        for dy, mb, A, sv, xg in zip(dys, ctx.members, ctx.args, ctx.saved_bufs, ctx.xaccs):      # (forward pointers are still valid: `sv`)
            cfg = mb.cfg
            x = sv["x"]
            dy = dy.contiguous() if dy is not None else torch.zeros_like(x)
            dx = torch.empty_like(x)
            dx_ret = dx if xg is None else xg.settle(dx, post)       # see forward: the gradient of this input is collected in a shared buffer
            # hand-off, consumer side: the sublayer that ran before us in backward already wrote dy through OUR output dropout
            ready = mb.holder.claim(dy) if mb.holder is not None else None
            # producer side: write our dx also as the next sublayer's masked compute-dtype dy
            nxt = mb.feeds if (mb.feeds is not None and mb.feeds.lp == cfg.lp_dtype and xg is None) else None
            if nxt is not None:
                nxt.offer(dx, cfg.lp_dtype)
            if mb.kind == "mha":
                dmem = dmem_ret = mem_nxt = None
                accumulate = 0
                if sv["need_dmem"]:
                    dmem, accumulate, last = sv["gacc"].buffer((A.B, A.m, A.d), x.device)
                    if last:                         # last user (first in forward order): hand the sum to autograd once
                        dmem_ret = dmem
                        # ... and, through the dmem GEMM's epilogue, to the sublayer that produced the memory: the sum once
                        # more, through that sublayer's output dropout, in the compute dtype (its backward then needs no cast)
                        fm = sv["mem_next"]
                        if fm is not None and fm.lp == cfg.lp_dtype and cfg.lp_dtype != torch.float32 and _HANDOFF_MEM:
                            mem_nxt = fm
                            fm.offer(dmem, cfg.lp_dtype)
                keep = _pack_mha_bwd(A, cfg, sv, dy, dx, cfg.grads, 1, dmem, accumulate, mem_nxt, ready, nxt)
                grads_out += [dx_ret, dmem_ret]
            else:
                keep = _pack_ffn_bwd(A, cfg, sv, dy, dx, cfg.grads, 1, ready, nxt)
                grads_out += [dx_ret, None]
            work.append((A, keep))
        L.check(L.load().mtn_sublayer_group_bwd(code, ctx.n_mha, ctx.mha_args, ctx.n_ffn, ctx.ffn_args, L.stream_ptr()))
        for buf, dxp in post:
            buf.add_(dxp)
        for A, keep in work:
            _queue_param_grads(queue, code, A, keep)
        return (None, *grads_out)


def generator_logits(x, w_lp, bias):
    """The projection of Generator.forward alone (mtn.py:68: proj(x)): x (..., d) fp32 or compute dtype -> (..., V) fp32 logits, one
    grouped-GEMM launch (x W^T + b).  What score_rows reads: log-probabilities of chosen columns need no (rows, V) log-softmax."""
    _require_cuda(x, w_lp)
    lp = w_lp.dtype
    V, d = w_lp.shape
    a = x.reshape(-1, d)
    a = a.contiguous() if a.dtype == lp else cast_to_lp(a.contiguous(), lp)
    rows = a.size(0)
    out = torch.empty(rows, V, device=x.device, dtype=torch.float32)
    pr = L.GemmProblem()
    pr.A, pr.B, pr.lda, pr.ldb, pr.M, pr.N, pr.K = a.data_ptr(), w_lp.data_ptr(), d, d, rows, V, d
    pr.bias, pr.gate_scale, pr.out_f32, pr.ldc = bias.data_ptr(), 1.0, out.data_ptr(), V
    gemm(L.dtype_code(lp), [pr])
    return out.view(*x.shape[:-1], V)


def score_rows(logits, target, pad, out=None):
    """Per-token log-probability and rank of ``target`` (n_seq, L) int64 under ``logits`` (n_seq * L, V) or (n_seq, L, V) fp32 (unit
    column stride; a row stride >= V), and their per-sequence sums (csrc/score.hip; include/mtn_hip.h mtn_score_rows gives the
    definitions) -> (tok_logp (n_seq, L) fp32, tok_rank (n_seq, L) int32, seq_logp (n_seq,) float64, seq_len (n_seq,) int32).
    ``pad`` positions (and ids outside the vocabulary) give 0 / -1 and are not counted.  ``out``: the four tensors to write into."""
    _require_cuda(logits, target)
    if target.dim() != 2 or target.dtype != torch.int64 or not target.is_contiguous():
        raise ValueError("score_rows: target is a contiguous (n_seq, L) int64 tensor")
    n_seq, Ls = target.shape
    if logits.dim() == 3 and logits.is_contiguous():
        logits = logits.view(-1, logits.size(-1))
    if (logits.dim() != 2 or logits.dtype != torch.float32 or logits.size(0) != n_seq * Ls or (logits.size(1) > 1 and logits.stride(1) != 1)
            or logits.stride(0) < logits.size(1)):
        raise ValueError("score_rows: logits fp32 (n_seq * L, V) with unit column stride, one row per target position")
    dev = logits.device
    if out is None:
        out = (torch.empty(n_seq, Ls, device=dev, dtype=torch.float32), torch.empty(n_seq, Ls, device=dev, dtype=torch.int32),
               torch.empty(n_seq, device=dev, dtype=torch.float64), torch.empty(n_seq, device=dev, dtype=torch.int32))
    tl, tr, sl, sn = out
    _require_cuda(*out)
    if not (tl.dtype == torch.float32 and tr.dtype == torch.int32 and sl.dtype == torch.float64 and sn.dtype == torch.int32
            and tl.shape == tr.shape == target.shape and sl.numel() == sn.numel() == n_seq and all(t.is_contiguous() for t in out)):
        raise ValueError("score_rows: out = (fp32 (n_seq, L), int32 (n_seq, L), float64 (n_seq,), int32 (n_seq,)), each contiguous")
    a = L.ScoreArgs()
    a.n_seq, a.L, a.V, a.pad, a.ldz = n_seq, Ls, logits.size(1), int(pad), logits.stride(0)
    a.logits, a.target = logits.data_ptr(), target.data_ptr()
    a.tok_logp, a.tok_rank, a.seq_logp, a.seq_len = tl.data_ptr(), tr.data_ptr(), sl.data_ptr(), sn.data_ptr()
    L.check(L.load().mtn_score_rows(C.byref(a), L.stream_ptr()))
    return out


def generator_log_probs(x, w_lp, bias):
    """Generator.forward at inference (mtn.py:68-69: log_softmax(proj(x))) on the HIP path: x (..., d) fp32 or compute dtype ->
    (..., V) fp32 log-probabilities.  One grouped-GEMM launch (x W^T + b, fp32 logits) and one row kernel (csrc/select.hip) —
    no vendor BLAS / softmax kernels in a decode step.  No autograd: training goes through GeneratorLossFn (fused loss head)."""
    V = w_lp.size(0)
    out = generator_logits(x, w_lp, bias).view(-1, V)
    L.check(L.load().mtn_log_softmax_rows(out.data_ptr(), out.size(0), V, V, out.data_ptr(), V, L.stream_ptr()))
    return out.view(*x.shape[:-1], V)


def topk_rows(x, k, extra_col=-1):
    """x (rows, V) fp32 -> (rows, 2k+1) fp32: per row its k largest entries in descending order, their column indices (as floats)
    and x[row, extra_col] — the part of a log-probability row the beam search looks at (data_utils.py:219), csrc/select.hip."""
    _require_cuda(x)
    x = x.contiguous()
    out = torch.empty(x.size(0), 2 * k + 1, device=x.device, dtype=torch.float32)
    L.check(L.load().mtn_topk_rows(x.data_ptr(), x.size(0), x.size(1), x.stride(0), k, extra_col, out.data_ptr(), L.stream_ptr()))
    return out


def sample_args(logp, seed, keys, step, log, *, temperature=1.0, top_k=0, top_p=1.0, banned=(), eos=-1, min_len=0, rows=None,
                tokens=None, pos=None, anc=None):
    """The argument block of mtn_sample_rows (include/mtn_hip.h) for logp (n, V) fp32: seed (1,) / keys (rows,) int64 and step (rows,)
    int32 on the device, log = (tokens int32, log-probabilities fp32, u fp32), each (L, rows).  ``rows`` > n with n = 1 makes every
    row read the one distribution (ldx = 0).  tokens / pos / anc: what the next persistent decode step reads, as pointers or tensors."""
    _require_cuda(logp, seed, keys, step, *log)
    if logp.dtype != torch.float32 or logp.stride(-1) != 1 or seed.dtype != torch.int64 or keys.dtype != torch.int64 or step.dtype != torch.int32:
        raise ValueError("sample_rows: logp fp32 with unit column stride, seed / keys int64, step int32")
    n, V = logp.shape
    rows = n if rows is None else int(rows)
    if rows != n and n != 1:
        raise ValueError("sample_rows: rows differs from logp's only when one distribution serves every row")
    banned = [int(b) for b in banned]
    lt, ll, lu = log
    if len(banned) > 4 or keys.numel() != rows or step.numel() != rows or seed.numel() != 1:
        raise ValueError("sample_rows: at most 4 banned tokens; one key and one step per row, one seed")
    if not (lt.dtype == torch.int32 and ll.dtype == lu.dtype == torch.float32 and lt.shape == ll.shape == lu.shape and lt.dim() == 2
            and lt.size(1) == rows and all(t.is_contiguous() for t in (lt, ll, lu, keys, step))):
        raise ValueError("sample_rows: the log is (int32, fp32, fp32), each contiguous (L, rows)")
    a = L.SampleArgs()
    a.rows, a.V, a.ldx, a.logp = rows, V, (0 if rows != n else (V if n == 1 else logp.stride(0))), logp.data_ptr()
    a.temperature, a.top_k, a.top_p = float(temperature), int(top_k), float(top_p)
    a.n_banned, a.eos, a.min_len = len(banned), int(eos), int(min_len)
    for i, b in enumerate(banned):
        a.banned[i] = b
    a.seed, a.key, a.step, a.L = seed.data_ptr(), keys.data_ptr(), step.data_ptr(), lt.size(0)
    a.log_tok, a.log_logp, a.log_u = lt.data_ptr(), ll.data_ptr(), lu.data_ptr()
    as_ptr = lambda t: None if t is None else (t if isinstance(t, int) else t.data_ptr())
    a.tokens, a.pos, a.anc = as_ptr(tokens), as_ptr(pos), as_ptr(anc)
    return a


def sample_rows(logp, seed, keys, step, log=None, max_len=1, **kw):
    """One drawn token per row of logp (n, V) fp32 log-probabilities (csrc/sample.hip; include/mtn_hip.h mtn_sample_rows gives the
    definitions of ban / temperature / top-k / top-p / draw): row r draws with u = hash(seed, keys[r], step[r]), logs (token,
    logp[token], u) at [step[r], r] of ``log`` (created as (max_len, rows) when None) and advances step[r].  Returns the log."""
    rows = kw.get("rows") or logp.size(0)
    if log is None:
        log = (torch.zeros(max_len, rows, device=logp.device, dtype=torch.int32), torch.zeros(max_len, rows, device=logp.device),
               torch.zeros(max_len, rows, device=logp.device))
    a = sample_args(logp, seed, keys, step, log, **kw)
    L.check(L.load().mtn_sample_rows(C.byref(a), L.stream_ptr()))
    return log


CONTRASTIVE_MAX_K = 16        # csrc/contrastive.hip CS_MAX_K: rows of a dialogue, and entries of a row's head
CONTRASTIVE_MAX_D = 1024      # csrc/contrastive.hip CS_MAX_D


def contrastive_args(hidden, top, tokens, pos, cand_logp, step, done, log, *, k, alpha, eos=-1, min_len=0, banned=()):
    """The argument block of mtn_contrastive_advance (include/mtn_hip.h) for hidden (rows, L, d) fp32 — the decoder's final-norm states,
    unit element stride, any row / position strides at least the dense ones —, top (rows, 2 * k_top + 1) fp32 as topk_rows leaves it,
    tokens (rows, L) int64, pos (1,) int64, cand_logp (rows,) fp32, step / done (rows / k,) int32 and log = (tokens int32,
    log-probabilities fp32, penalties fp32, ranks int32), each (L, rows / k); all but hidden contiguous."""
    lt, ll, lpn, lr = log
    _require_cuda(hidden, top, tokens, pos, cand_logp, step, done, *log)
    k, banned = int(k), [int(b) for b in banned]
    if hidden.dtype != torch.float32 or hidden.dim() != 3 or (hidden.size(2) > 1 and hidden.stride(2) != 1):
        raise ValueError("contrastive_advance: hidden is (rows, L, d) fp32 with unit element stride")
    rows, Lm, d = hidden.shape
    if not 1 <= k <= CONTRASTIVE_MAX_K or rows % k:
        raise ValueError("contrastive_advance: 1 <= k <= 16 rows per dialogue, and rows is a multiple of k")
    D = rows // k
    if not 1 <= d <= CONTRASTIVE_MAX_D or Lm < 1:
        raise ValueError("contrastive_advance: 1 <= d <= %d, L >= 1" % CONTRASTIVE_MAX_D)
    alpha = float(alpha)
    if not 0.0 <= alpha <= 1.0:                       # (a NaN fails both comparisons)
        raise ValueError("contrastive_advance: alpha is in [0, 1]")
    if len(banned) > 4:
        raise ValueError("contrastive_advance: at most 4 banned tokens")
    if top.dtype != torch.float32 or top.dim() != 2 or top.size(0) != rows or not top.is_contiguous() or top.size(1) % 2 != 1:
        raise ValueError("contrastive_advance: top is a contiguous (rows, 2 * k_top + 1) fp32 tensor")
    k_top = (top.size(1) - 1) // 2
    if not min(CONTRASTIVE_MAX_K, k + len(banned) + 1) <= k_top <= CONTRASTIVE_MAX_K:
        raise ValueError("contrastive_advance: min(16, k + banned + 1) <= k_top <= 16")
    if tokens.dtype != torch.int64 or tuple(tokens.shape) != (rows, Lm) or not tokens.is_contiguous() or pos.dtype != torch.int64 or pos.numel() != 1:
        raise ValueError("contrastive_advance: tokens is a contiguous (rows, L) int64 tensor, pos one int64")
    if cand_logp.dtype != torch.float32 or cand_logp.numel() != rows or not cand_logp.is_contiguous():
        raise ValueError("contrastive_advance: cand_logp is a contiguous (rows,) fp32 tensor")
    if any(t.dtype != torch.int32 or t.numel() != D or not t.is_contiguous() for t in (step, done)):
        raise ValueError("contrastive_advance: step and done are contiguous (dialogues,) int32 tensors")
    if not (lt.dtype == lr.dtype == torch.int32 and ll.dtype == lpn.dtype == torch.float32 and all(tuple(t.shape) == (Lm, D) and t.is_contiguous() for t in log)):
        raise ValueError("contrastive_advance: the log is (int32, fp32, fp32, int32), each contiguous (L, dialogues)")
    a = L.ContrastiveArgs()
    a.dialogues, a.k, a.L, a.d, a.k_top, a.alpha = D, k, Lm, d, k_top, alpha
    a.eos, a.min_len, a.n_banned = int(eos), int(min_len), len(banned)
    for i, b in enumerate(banned):
        a.banned[i] = b
    a.hidden = hidden.data_ptr()
    a.row_stride = hidden.stride(0) if rows > 1 else max(hidden.stride(0), (Lm - 1) * max(hidden.stride(1), d) + d)
    a.pos_stride = hidden.stride(1) if Lm > 1 else max(hidden.stride(1), d)
    a.top, a.tokens, a.pos, a.cand_logp, a.step, a.done = (t.data_ptr() for t in (top, tokens, pos, cand_logp, step, done))
    a.log_tok, a.log_logp, a.log_pen, a.log_rank = lt.data_ptr(), ll.data_ptr(), lpn.data_ptr(), lr.data_ptr()
    return a


def contrastive_advance(hidden, top, tokens, pos, cand_logp, step, done, log, **kw):
    """One token of a contrastive search for every dialogue of k rows (csrc/contrastive.hip; include/mtn_hip.h mtn_contrastive_advance
    gives the definition): scores the rows' candidates by probability and degeneration penalty, logs the choice at [step, dialogue] of
    ``log``, stores it into ``tokens`` and deals the winner's head to the rows as the next candidates — all in place, one launch.
    Keywords: k, alpha, eos, min_len, banned.  Returns the log."""
    a = contrastive_args(hidden, top, tokens, pos, cand_logp, step, done, log, **kw)
    if a.dialogues:
        L.check(L.load().mtn_contrastive_advance(C.byref(a), L.stream_ptr()))
    return log


SCHED_PICKS = {"argmax": L.MTN_SCHED_ARGMAX, "sample": L.MTN_SCHED_SAMPLE}


def sched_mix(logits, trg, keys, state, *, pad, prob, start=0, ramp=0, pick="argmax", temperature=1.0, seed=0, banned=(), out=None,
              stats=None, pick_score=None):
    """Scheduled sampling's token mix (csrc/sched.hip; include/mtn_hip.h mtn_sched_mix gives every formula): logits (B * T, V) fp32
    (unit column stride, any row stride >= V) are the generator's rows of a teacher-forced pass over the gold decoder inputs ``trg``
    (B, T) int64; row (b, t - 1) predicts trg[b, t].  Returns ``out`` (B, T) int64 (created when None; never ``trg`` itself): trg with a
    fraction p = prob * min(1, max(0, step - start) / ramp) of its eligible positions (t >= 1, not <pad>) replaced by the row's arg-max
    ("argmax") or a Gumbel-max draw at ``temperature`` ("sample") over the columns that are neither ``pad`` nor ``banned``.  ``keys``
    (B,) int64 name the rows to the counter hash; ``state`` is the optimiser's device state (FusedAdam.state): state[0], the step
    number, is read on the device, so a captured launch draws anew on every replay.  ``stats`` (3,) int64 accumulates [eligible,
    replaced, replaced with a token other than gold]; ``pick_score`` (B, T) fp32 receives the winning score (NaN where gold stays)."""
    _require_cuda(logits, trg, keys, state)
    if pick not in SCHED_PICKS:
        raise ValueError("sched_mix: pick is 'argmax' or 'sample'")
    if logits.dtype != torch.float32 or logits.dim() != 2 or (logits.size(1) > 1 and logits.stride(1) != 1):
        raise ValueError("sched_mix: logits is (B * T, V) fp32 with unit column stride")
    if trg.dtype != torch.int64 or trg.dim() != 2 or not trg.is_contiguous() or keys.dtype != torch.int64 or not keys.is_contiguous():
        raise ValueError("sched_mix: trg is a contiguous (B, T) int64 tensor, keys a contiguous (B,) int64 tensor")
    B, T = trg.shape
    if logits.size(0) != B * T or keys.numel() != B or state.dtype != torch.float32 or state.numel() < 1:
        raise ValueError("sched_mix: one logits row per target position, one key per sequence, an fp32 optimiser state")
    banned = [int(b) for b in banned]
    if len(banned) > 4:
        raise ValueError("sched_mix: at most 4 banned tokens")
    if not float(temperature) > 0.0:
        raise ValueError("sched_mix: temperature > 0")
    dev = trg.device
    if out is None:
        out = torch.empty_like(trg)
    if stats is None:
        stats = torch.zeros(3, dtype=torch.int64, device=dev)
    for name, t, dt, n in (("out", out, torch.int64, B * T), ("stats", stats, torch.int64, 3)) + \
            ((("pick_score", pick_score, torch.float32, B * T),) if pick_score is not None else ()):
        if t.dtype != dt or t.numel() != n or not t.is_contiguous() or t.device != dev:
            raise ValueError("sched_mix: %s is a contiguous %s tensor of %d elements on trg's device" % (name, dt, n))
    if B * T == 0:                    # (an empty tensor has no address to hand over)
        return out
    a = L.SchedArgs()
    a.B, a.T, a.V, a.ldx = B, T, logits.size(1), (logits.stride(0) if logits.size(0) > 1 else logits.size(1))
    a.logits, a.trg, a.key, a.state = logits.data_ptr(), trg.data_ptr(), keys.data_ptr(), state.data_ptr()
    a.pad, a.n_banned = int(pad), len(banned)
    for i, b in enumerate(banned):
        a.banned[i] = b
    a.p_max, a.start, a.ramp, a.pick = float(prob), int(start), int(ramp), SCHED_PICKS[pick]
    a.inv_temperature, a.seed = 1.0 / float(temperature), int(seed)
    a.mixed, a.stats, a.pick_score = out.data_ptr(), stats.data_ptr(), L.ptr(pick_score)
    L.check(L.load().mtn_sched_mix(C.byref(a), L.stream_ptr()))
    return out


def constrain_rows(logp, ngram=0, theta=1.0, *, hist=None, hist_len=None, log_tok=None, log_parent=None, step=None, width=1,
                   rows_per_step=1, log_len=None, out=None):
    """N-gram blocking and repetition penalty on the rows of logp (rows, V) fp32 from each row's history (csrc/constrain.hip;
    include/mtn_hip.h mtn_constrain_rows gives the definitions).  In place unless ``out`` (same shape, no overlap) is given.
    History, explicit: ``hist`` (rows, >= L) int32 and ``hist_len`` (rows,) int32 on the device.  Or from a search's step log:
    ``log_tok`` / ``log_parent`` (L, rows) int32 (log_parent None: every row is its own parent) and ``step`` int32 with one counter per
    ``rows_per_step`` rows; ``width`` = rows per dialogue.  The log and step may be tensors or raw device pointers (then ``log_len``, the
    log's L, is required: a captured search passes pointers into its state blocks).  Returns the rows written."""
    _require_cuda(logp)
    if logp.dim() != 2 or logp.dtype != torch.float32 or (logp.size(1) > 1 and logp.stride(1) != 1) or logp.stride(0) < logp.size(1):
        raise ValueError("constrain_rows: logp fp32 (rows, V) with unit column stride")
    rows, V = logp.shape
    ngram, theta = int(ngram), float(theta)
    if not 0 <= ngram <= 8 or not theta >= 1.0:
        raise ValueError("constrain_rows: 0 <= ngram <= 8, theta >= 1")
    if out is None:
        out = logp
    else:
        _require_cuda(out)
        if out.shape != logp.shape or out.dtype != torch.float32 or (V > 1 and out.stride(1) != 1) or out.stride(0) < V:
            raise ValueError("constrain_rows: out is fp32 of logp's shape with unit column stride")
        span = lambda t: (t.data_ptr(), t.data_ptr() + ((rows - 1) * t.stride(0) + V) * 4)
        (lo, hi), (olo, ohi) = span(logp), span(out)
        ld, off = logp.stride(0), abs(olo - lo) // 4
        # (equal row strides: rows meet only if the offset, modulo the stride, is less than V either way — two column blocks of one
        # buffer do not overlap; offset 0 is logp itself)
        apart = out.stride(0) == ld and (off == 0 or (off % ld >= V and ld - off % ld >= V))
        if lo < ohi and olo < hi and not apart:
            raise ValueError("constrain_rows: out overlaps logp without being logp (in place: leave out None or pass logp itself)")
    a = L.ConstrainArgs()
    a.rows, a.V, a.ldx, a.ldo, a.logp, a.out = rows, V, logp.stride(0), out.stride(0), logp.data_ptr(), out.data_ptr()
    a.ngram, a.theta = ngram, theta
    if hist is not None:
        if hist_len is None:
            raise ValueError("constrain_rows: hist needs hist_len, int32 (rows,)")
        _require_cuda(hist, hist_len)
        if (hist.dim() != 2 or hist.dtype != torch.int32 or hist.size(0) != rows or hist.size(1) < 1 or hist.stride(1) != 1 or hist_len.dtype != torch.int32
                or hist_len.numel() != rows or not hist_len.is_contiguous() or log_tok is not None):
            raise ValueError("constrain_rows: hist int32 (rows, L) with unit column stride and hist_len int32 (rows,); one history source")
        a.L = hist.size(1) if log_len is None else int(log_len)
        if a.L > hist.size(1):
            raise ValueError("constrain_rows: log_len exceeds the history table's width")
        a.hist, a.ldh, a.hist_len = hist.data_ptr(), max(hist.stride(0), hist.size(1)), hist_len.data_ptr()
    else:
        if log_tok is None or step is None:
            raise ValueError("constrain_rows: a history source is required (hist + hist_len, or log_tok + step)")
        width, rows_per_step = int(width), int(rows_per_step)
        if not 1 <= width <= 16 or rows % width or rows_per_step < 1:
            raise ValueError("constrain_rows: 1 <= width <= 16, rows a multiple of width, rows_per_step >= 1")
        for t in (log_tok, log_parent):
            if t is not None and not isinstance(t, int):
                _require_cuda(t)
                if t.dtype != torch.int32 or t.dim() != 2 or t.size(1) != rows or not t.is_contiguous() or (log_len is not None and t.size(0) < int(log_len)):
                    raise ValueError("constrain_rows: the step log is int32, contiguous (L, rows)")
        if not isinstance(step, int):
            _require_cuda(step)
            if step.dtype != torch.int32 or not step.is_contiguous() or step.numel() * rows_per_step < rows:
                raise ValueError("constrain_rows: step int32, one counter per rows_per_step rows")
        if log_len is None:
            if isinstance(log_tok, int):
                raise ValueError("constrain_rows: log_len is required with a raw log pointer")
            log_len = log_tok.size(0)
        as_ptr = lambda t: None if t is None else (t if isinstance(t, int) else t.data_ptr())
        a.L, a.log_tok, a.log_parent, a.step, a.width, a.rows_per_step = int(log_len), as_ptr(log_tok), as_ptr(log_parent), as_ptr(step), width, rows_per_step
    L.check(L.load().mtn_constrain_rows(C.byref(a), L.stream_ptr()))
    return out


ENSEMBLE_MODES = {"prob": 0, "logprob": 1}
ENSEMBLE_MAX = 8         # csrc/ensemble.hip ENS_MAX_M


def ensemble_weights(n, weights=None):
    """The weights of an n-member ensemble as float64, normalised to sum 1 (None: uniform).  ValueError for a wrong count, a negative or
    non-finite weight, or all weights 0."""
    import numpy as np
    w = np.full(n, 1.0, dtype=np.float64) if weights is None else np.asarray([float(v) for v in weights], dtype=np.float64)
    if w.shape != (n,) or not np.isfinite(w).all() or (w < 0).any() or not w.sum() > 0:
        raise ValueError("ensemble: one finite weight >= 0 per member, not all of them 0")
    return w / w.sum()


def ensemble_rows(xs, weights=None, mode="prob", out=None):
    """The rows of M <= 8 models combined into one row matrix of log-probabilities (csrc/ensemble.hip; include/mtn_hip.h mtn_ensemble_rows
    gives the definitions): xs = M tensors (rows, V) fp32 with unit column stride and a row stride >= V, logits or log-probabilities (every
    member row is normalised by the kernel); ``weights`` >= 0, normalised here to sum 1 in float64 (None: uniform); ``mode`` "prob" (log of the
    weighted mean probability) or "logprob" (weighted mean log-probability, renormalised).  ``out``: fp32 (rows, V) overlapping no input.
    Misuse raises ValueError; tensors that are not on the GPU raise MtnHipError, as in every operator of this module.  A single row's
    stride is not looked at."""
    xs = list(xs)
    if not 1 <= len(xs) <= ENSEMBLE_MAX:
        raise ValueError("ensemble_rows: 1 to 8 members")
    if mode not in ENSEMBLE_MODES:
        raise ValueError("ensemble_rows: mode is 'prob' or 'logprob'")
    w = ensemble_weights(len(xs), weights)
    _require_cuda(*xs)
    x0 = xs[0]
    for x in xs:
        if (x.dim() != 2 or x.dtype != torch.float32 or x.shape != x0.shape or x.device != x0.device or x.numel() == 0
                or (x.size(1) > 1 and x.stride(1) != 1) or (x.size(0) > 1 and x.stride(0) < x.size(1))):
            raise ValueError("ensemble_rows: every member is fp32 (rows, V), non-empty, of one shape and device, with unit column stride")
    rows, V = x0.shape
    if V >= 1 << 24:
        raise ValueError("ensemble_rows: V < 2^24")
    if out is None:
        out = torch.empty(rows, V, device=x0.device, dtype=torch.float32)
    else:
        _require_cuda(out)
        if out.shape != x0.shape or out.dtype != torch.float32 or out.device != x0.device or (V > 1 and out.stride(1) != 1) or (rows > 1 and out.stride(0) < V):
            raise ValueError("ensemble_rows: out is fp32 of the members' shape with unit column stride")
        span = lambda t: (t.data_ptr(), t.data_ptr() + ((rows - 1) * t.stride(0) + V) * 4)
        olo, ohi = span(out)
        for x in xs:
            lo, hi = span(x)
            if lo < ohi and olo < hi:
                raise ValueError("ensemble_rows: out overlaps a member")
    a = L.EnsembleArgs()
    a.rows, a.V, a.M, a.mode, a.out, a.ldo = rows, V, len(xs), ENSEMBLE_MODES[mode], out.data_ptr(), max(out.stride(0), V)
    for m, x in enumerate(xs):
        a.x[m], a.ld[m], a.w[m] = x.data_ptr(), max(x.stride(0), V), float(w[m])
    L.check(L.load().mtn_ensemble_rows(C.byref(a), L.stream_ptr()))
    return out


MBR_MAX_HYP, MBR_MAX_LEN, MBR_MAX_ORDER = 16, 128, 4        # include/mtn_hip.h MTN_MBR_MAX_HYP; csrc/mbr.hip MBR_MAX_L


def mbr_select(ngram, *, tok=None, length=None, n_hyp=None, w=None, log_tok=None, sets=None, eos=None, out=None, util=False):
    """Minimum-Bayes-risk selection over sets of at most 16 hypotheses (csrc/mbr.hip; include/mtn_hip.h mtn_mbr_select gives the
    definition), ``ngram`` = the maximum n-gram order N in 1..4.  Hypotheses, explicit: ``tok`` (sets, K, >= L) int32 with unit token
    stride, ``length`` (sets, K) and ``n_hyp`` (sets,) int32, ``w`` (sets, K) float64 or None for uniform weights.  Or the token log of a
    sampling search: ``log_tok`` (L, sets * K) int32 with ``sets`` and ``eos`` — set s is columns s * K .. s * K + K - 1, cut at the first
    <eos>.  Everything lives on the device.  ``out`` = (expected (sets, K) float64, best (sets,) int32, order (sets, K) int32), allocated
    when None; ``util``: True allocates, or a (sets, K, K) float64 tensor receives, the utility of every pair.
    Returns (expected, best, order, util or None)."""
    ngram = int(ngram)
    if not 1 <= ngram <= MBR_MAX_ORDER:
        raise ValueError("mbr_select: the n-gram order is in 1..4")
    a = L.MbrArgs()
    if tok is not None:
        if length is None or n_hyp is None or log_tok is not None:
            raise ValueError("mbr_select: explicit hypotheses need length and n_hyp; one source of hypotheses")
        _require_cuda(tok, length, n_hyp)
        if (tok.dim() != 3 or tok.dtype != torch.int32 or tok.numel() == 0 or (tok.size(2) > 1 and tok.stride(2) != 1)
                or tok.stride(1) < tok.size(2) or tok.stride(0) != tok.size(1) * tok.stride(1)):
            raise ValueError("mbr_select: tok int32 (sets, K, L), non-empty, with unit token stride and rows of one stride")
        S, K, Lh = tok.shape
        if length.dtype != torch.int32 or tuple(length.shape) != (S, K) or not length.is_contiguous() or n_hyp.dtype != torch.int32 \
                or n_hyp.numel() != S or not n_hyp.is_contiguous():
            raise ValueError("mbr_select: length int32 (sets, K) and n_hyp int32 (sets,), contiguous")
        a.tok, a.len, a.n_hyp, a.ldl = tok.data_ptr(), length.data_ptr(), n_hyp.data_ptr(), tok.stride(1)
        dev = tok.device
    else:
        if log_tok is None or sets is None or eos is None:
            raise ValueError("mbr_select: a source of hypotheses is required (tok + length + n_hyp, or log_tok + sets + eos)")
        _require_cuda(log_tok)
        S = int(sets)
        if log_tok.dim() != 2 or log_tok.dtype != torch.int32 or not log_tok.is_contiguous() or S < 1 or log_tok.size(1) < S or log_tok.size(1) % S:
            raise ValueError("mbr_select: the token log is int32, contiguous (L, sets * K)")
        Lh, K = log_tok.size(0), log_tok.size(1) // S
        a.log_tok, a.eos = log_tok.data_ptr(), int(eos)
        dev = log_tok.device
    if not 1 <= K <= MBR_MAX_HYP or not 1 <= Lh <= MBR_MAX_LEN:
        raise ValueError("mbr_select: at most 16 hypotheses per set, of at most 128 tokens")
    if w is not None:
        _require_cuda(w)
        if w.dtype != torch.float64 or tuple(w.shape) != (S, K) or not w.is_contiguous():
            raise ValueError("mbr_select: w float64 (sets, K), contiguous")
        a.w = w.data_ptr()
    if out is None:
        out = (torch.empty(S, K, device=dev, dtype=torch.float64), torch.empty(S, dtype=torch.int32, device=dev),
               torch.empty(S, K, dtype=torch.int32, device=dev))
    expected, best, order = out
    _require_cuda(expected, best, order)
    if (expected.dtype != torch.float64 or best.dtype != torch.int32 or order.dtype != torch.int32 or expected.numel() != S * K or best.numel() != S
            or order.numel() != S * K or not all(t.is_contiguous() for t in out)):
        raise ValueError("mbr_select: out = (expected float64 (sets, K), best int32 (sets,), order int32 (sets, K)), contiguous")
    if util is True:
        util = torch.empty(S, K, K, device=dev, dtype=torch.float64)
    elif util is False:
        util = None
    if util is not None:
        _require_cuda(util)
        if util.dtype != torch.float64 or util.numel() != S * K * K or not util.is_contiguous():
            raise ValueError("mbr_select: util float64 (sets, K, K), contiguous")
        a.util = util.data_ptr()
    a.sets, a.K, a.L, a.N = S, K, Lh, ngram
    a.expected, a.best, a.order = expected.data_ptr(), best.data_ptr(), order.data_ptr()
    L.check(L.load().mtn_mbr_select(C.byref(a), L.stream_ptr()))
    return expected, best, order, util


EVAL_MAX_REF, EVAL_MAX_LEN = 8, 128                        # include/mtn_hip.h MTN_EVAL_MAX_REF; csrc/eval.hip EV_L


def eval_workspace_bytes(Q, R, Lh):
    """Bytes of the document-frequency table eval_metrics needs for Q items of R references of Lh tokens (0 for sizes it refuses)."""
    return int(L.load().mtn_eval_workspace_bytes(int(Q), int(R), int(Lh)))


def eval_metrics(hyp, hyp_len, ref, ref_len, n_ref, *, workspace=None, out=None, df_of_ref=False):
    """BLEU-1..4, ROUGE-L and CIDEr of Q items on the device (csrc/eval.hip; include/mtn_hip.h mtn_eval_metrics gives the definition).
    ``hyp`` (Q, >= Lh) and ``ref`` (Q, R, >= Lh) int32 with unit token stride and ONE row stride (ldl) between them, ``hyp_len`` (Q,),
    ``ref_len`` (Q, R) and ``n_ref`` (Q,) int32, contiguous; R <= 8, Lh <= 128.  Everything lives on the device.  ``workspace``: a uint8
    tensor of at least eval_workspace_bytes(Q, R, Lh) bytes, allocated when None.  ``out`` = (stats (Q, 10) int32, rouge (Q,) float64,
    cider (Q,) float64, corpus (8,) float64), allocated when None; ``df_of_ref``: True allocates, or a (Q, R, Lh, 4) int32 tensor
    receives, the document frequency of the n-gram at every reference position.
    Returns (stats, rouge, cider, corpus, df_of_ref or None); corpus = Bleu_1..4, ROUGE_L, CIDEr, sum len(h), sum closest."""
    _require_cuda(hyp, hyp_len, ref, ref_len, n_ref)
    if (ref.dim() != 3 or ref.dtype != torch.int32 or ref.numel() == 0 or (ref.size(2) > 1 and ref.stride(2) != 1)
            or ref.stride(1) < ref.size(2) or ref.stride(0) != ref.size(1) * ref.stride(1)):
        raise ValueError("eval_metrics: ref int32 (Q, R, L), non-empty, with unit token stride and rows of one stride")
    Q, R, Lh = ref.shape
    ldl = ref.stride(1)
    if (hyp.dim() != 2 or hyp.dtype != torch.int32 or tuple(hyp.shape) != (Q, Lh) or (Lh > 1 and hyp.stride(1) != 1)
            or (Q > 1 and hyp.stride(0) != ldl)):
        raise ValueError("eval_metrics: hyp int32 (Q, L) with unit token stride and the row stride of ref")
    if not 1 <= R <= EVAL_MAX_REF or not 1 <= Lh <= EVAL_MAX_LEN:
        raise ValueError("eval_metrics: at most 8 references per item, sentences of at most 128 tokens")
    for t, shape, name in ((hyp_len, (Q,), "hyp_len (Q,)"), (ref_len, (Q, R), "ref_len (Q, R)"), (n_ref, (Q,), "n_ref (Q,)")):
        if t.dtype != torch.int32 or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError("eval_metrics: %s int32, contiguous" % name)
    need = eval_workspace_bytes(Q, R, Lh)
    if need <= 0:
        raise ValueError("eval_metrics: Q * R * L is at most 2^28")
    dev = ref.device
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    _require_cuda(workspace)
    if workspace.dtype != torch.uint8 or not workspace.is_contiguous() or workspace.numel() < need or workspace.data_ptr() % 16:
        raise ValueError("eval_metrics: workspace uint8, contiguous, 16-byte aligned, at least eval_workspace_bytes(Q, R, L) = %d bytes" % need)
    if out is None:
        out = (torch.empty(Q, 10, dtype=torch.int32, device=dev), torch.empty(Q, dtype=torch.float64, device=dev),
               torch.empty(Q, dtype=torch.float64, device=dev), torch.empty(8, dtype=torch.float64, device=dev))
    stats, rouge, cider, corpus = out
    _require_cuda(stats, rouge, cider, corpus)
    if (stats.dtype != torch.int32 or tuple(stats.shape) != (Q, 10) or any(t.dtype != torch.float64 for t in (rouge, cider, corpus))
            or rouge.numel() != Q or cider.numel() != Q or corpus.numel() != 8 or not all(t.is_contiguous() for t in out)):
        raise ValueError("eval_metrics: out = (stats int32 (Q, 10), rouge float64 (Q,), cider float64 (Q,), corpus float64 (8,)), contiguous")
    if df_of_ref is True:
        df_of_ref = torch.empty(Q, R, Lh, 4, dtype=torch.int32, device=dev)
    elif df_of_ref is False:
        df_of_ref = None
    a = L.EvalArgs()
    if df_of_ref is not None:
        _require_cuda(df_of_ref)
        if df_of_ref.dtype != torch.int32 or tuple(df_of_ref.shape) != (Q, R, Lh, 4) or not df_of_ref.is_contiguous():
            raise ValueError("eval_metrics: df_of_ref int32 (Q, R, L, 4), contiguous")
        a.df_of_ref = df_of_ref.data_ptr()
    a.Q, a.R, a.L, a.ldl = Q, R, Lh, ldl
    a.hyp, a.hyp_len, a.ref, a.ref_len, a.n_ref = hyp.data_ptr(), hyp_len.data_ptr(), ref.data_ptr(), ref_len.data_ptr(), n_ref.data_ptr()
    a.workspace, a.workspace_bytes = workspace.data_ptr(), workspace.numel()
    a.stats, a.rouge, a.cider, a.corpus = stats.data_ptr(), rouge.data_ptr(), cider.data_ptr(), corpus.data_ptr()
    L.check(L.load().mtn_eval_metrics(C.byref(a), L.stream_ptr()))
    return stats, rouge, cider, corpus, df_of_ref


# ------------------------------------------------------------------------------------------ self-critical sequence training (csrc/scst.hip)
def _eval_corpus_args(fn, ref, ref_len, n_ref, workspace):
    """The corpus half of an EvalRowsArgs: ``ref`` (Qc, R, >= L) int32 as eval_metrics takes it, ``workspace`` a uint8 table or None."""
    _require_cuda(ref, ref_len, n_ref)
    if (ref.dim() != 3 or ref.dtype != torch.int32 or ref.numel() == 0 or (ref.size(2) > 1 and ref.stride(2) != 1)
            or ref.stride(1) < ref.size(2) or ref.stride(0) != ref.size(1) * ref.stride(1)):
        raise ValueError(fn + ": ref int32 (Qc, R, L), non-empty, with unit token stride and rows of one stride")
    Qc, R, Lh = ref.shape
    if not 1 <= R <= EVAL_MAX_REF or not 1 <= Lh <= EVAL_MAX_LEN:
        raise ValueError(fn + ": at most 8 references per item, sentences of at most 128 tokens")
    for t, shape, name in ((ref_len, (Qc, R), "ref_len (Qc, R)"), (n_ref, (Qc,), "n_ref (Qc,)")):
        if t.dtype != torch.int32 or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(fn + ": %s int32, contiguous" % name)
    need = eval_workspace_bytes(Qc, R, Lh)
    if need <= 0:
        raise ValueError(fn + ": Qc * R * L is at most 2^28")
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=ref.device)
    _require_cuda(workspace)
    if workspace.dtype != torch.uint8 or not workspace.is_contiguous() or workspace.numel() < need or workspace.data_ptr() % 16:
        raise ValueError(fn + ": workspace uint8, contiguous, 16-byte aligned, at least eval_workspace_bytes(Qc, R, L) = %d bytes" % need)
    a = L.EvalRowsArgs()
    a.Qc, a.R, a.L, a.ldl = Qc, R, Lh, ref.stride(1)
    a.ref, a.ref_len, a.n_ref = ref.data_ptr(), ref_len.data_ptr(), n_ref.data_ptr()
    a.workspace, a.workspace_bytes = workspace.data_ptr(), workspace.numel()
    return a, workspace


def eval_table_build(ref, ref_len, n_ref, workspace=None):
    """The document-frequency table of a FIXED reference corpus (include/mtn_hip.h mtn_eval_table_build), built once: ``ref`` (Qc, R, >= L)
    int32, ``ref_len`` (Qc, R), ``n_ref`` (Qc,) as eval_metrics takes them.  Returns the table (a uint8 tensor; ``workspace`` when given).
    The table points into ``ref``: keep ref, ref_len and n_ref alive and unchanged for as long as eval_score_rows reads the table."""
    a, workspace = _eval_corpus_args("eval_table_build", ref, ref_len, n_ref, workspace)
    L.check(L.load().mtn_eval_table_build(C.byref(a), L.stream_ptr()))
    return workspace


def eval_score_rows(hyp, hyp_len, item, ref, ref_len, n_ref, table, out=None):
    """CIDEr, ROUGE-L and the BLEU integers of N hypotheses, hypothesis n against corpus item ``item[n]`` with the corpus table's df and
    Q = Qc (mtn_eval_score_rows: one launch, no atomics, equal bytes from equal inputs).  ``hyp`` (N, L) int32 with the row stride of
    ``ref``, ``hyp_len`` and ``item`` (N,) int32, ``table`` = eval_table_build(ref, ref_len, n_ref).  ``out`` = (stats (N, 10) int32,
    rouge (N,) float64, cider (N,) float64), allocated when None.  Returns (stats, rouge, cider)."""
    a, _ = _eval_corpus_args("eval_score_rows", ref, ref_len, n_ref, table)
    _require_cuda(hyp, hyp_len, item)
    if hyp.dim() != 2 or hyp.dtype != torch.int32 or hyp.size(0) < 1 or hyp.size(1) != a.L or (a.L > 1 and hyp.stride(1) != 1) or (
            hyp.size(0) > 1 and hyp.stride(0) != a.ldl):
        raise ValueError("eval_score_rows: hyp int32 (N, L) with unit token stride and the row stride of ref")
    N = hyp.size(0)
    for t, name in ((hyp_len, "hyp_len"), (item, "item")):
        if t.dtype != torch.int32 or tuple(t.shape) != (N,) or not t.is_contiguous():
            raise ValueError("eval_score_rows: %s int32 (N,), contiguous" % name)
    dev = ref.device
    if out is None:
        out = (torch.empty(N, 10, dtype=torch.int32, device=dev), torch.empty(N, dtype=torch.float64, device=dev),
               torch.empty(N, dtype=torch.float64, device=dev))
    stats, rouge, cider = out
    _require_cuda(stats, rouge, cider)
    if (stats.dtype != torch.int32 or tuple(stats.shape) != (N, 10) or rouge.dtype != torch.float64 or cider.dtype != torch.float64
            or rouge.numel() != N or cider.numel() != N or not all(t.is_contiguous() for t in out)):
        raise ValueError("eval_score_rows: out = (stats int32 (N, 10), rouge float64 (N,), cider float64 (N,)), contiguous")
    a.N, a.hyp, a.hyp_len, a.item = N, hyp.data_ptr(), hyp_len.data_ptr(), item.data_ptr()
    a.stats, a.rouge, a.cider = stats.data_ptr(), rouge.data_ptr(), cider.data_ptr()
    L.check(L.load().mtn_eval_score_rows(C.byref(a), L.stream_ptr()))
    return stats, rouge, cider


def scst_assemble(log_tok, sos, eos, pad, T=None, out=None, hyp_stride=None):
    """The sample log ``log_tok`` (L, rows) int32 (as sample_rows writes it) cut at each row's first <eos> (L - 1 tokens without one) and
    written as teacher-forcing targets: (trg (rows, T) int64 = <sos>, y.., <pad>..; trg_y (rows, T) int64 = y.., <eos>, <pad>..;
    hyp (rows, L) int32 with row stride ``hyp_stride`` (default L) = y.., <pad>..; hyp_len (rows,) int32), T >= L (default L).
    ``out``: the four tensors, allocated when None.  One launch (mtn_scst_assemble), no host read."""
    _require_cuda(log_tok)
    if log_tok.dim() != 2 or log_tok.dtype != torch.int32 or not log_tok.is_contiguous() or log_tok.numel() == 0:
        raise ValueError("scst_assemble: log_tok int32 (L, rows), contiguous, non-empty")
    Lm, rows = log_tok.shape
    T = Lm if T is None else int(T)
    ldh = Lm if hyp_stride is None else int(hyp_stride)
    if T < Lm or ldh < Lm:
        raise ValueError("scst_assemble: T >= L and hyp_stride >= L")
    dev = log_tok.device
    if out is None:
        out = (torch.empty(rows, T, dtype=torch.long, device=dev), torch.empty(rows, T, dtype=torch.long, device=dev),
               torch.full((rows, ldh), int(pad), dtype=torch.int32, device=dev)[:, :Lm], torch.empty(rows, dtype=torch.int32, device=dev))
    trg, trg_y, hyp, hyp_len = out
    _require_cuda(trg, trg_y, hyp, hyp_len)
    if any(t.dtype != torch.long or tuple(t.shape) != (rows, T) or not t.is_contiguous() for t in (trg, trg_y)):
        raise ValueError("scst_assemble: trg, trg_y int64 (rows, T), contiguous")
    if (hyp.dtype != torch.int32 or tuple(hyp.shape) != (rows, Lm) or (Lm > 1 and hyp.stride(1) != 1) or (rows > 1 and hyp.stride(0) != ldh)
            or hyp_len.dtype != torch.int32 or tuple(hyp_len.shape) != (rows,) or not hyp_len.is_contiguous()):
        raise ValueError("scst_assemble: hyp int32 (rows, L) with row stride hyp_stride, hyp_len int32 (rows,)")
    a = L.ScstAssembleArgs()
    a.rows, a.L, a.T, a.log_tok, a.sos, a.eos, a.pad = rows, Lm, T, log_tok.data_ptr(), int(sos), int(eos), int(pad)
    a.trg, a.trg_y, a.hyp, a.ldh, a.hyp_len = trg.data_ptr(), trg_y.data_ptr(), hyp.data_ptr(), ldh, hyp_len.data_ptr()
    L.check(L.load().mtn_scst_assemble(C.byref(a), L.stream_ptr()))
    return trg, trg_y, hyp, hyp_len


def scst_advantage(reward, T, baseline=None, roww=None, means=None, adv=None):
    """Rewards -> signed row weights (mtn_scst_advantage): ``reward`` (D, S) float64; ``baseline`` (D,) float64 or None = the leave-one-out
    mean of the dialogue's other rewards (S >= 2).  Writes ``roww`` — the first D * S * T floats of a contiguous float32 tensor, (D * S, T)
    when allocated here — with -(r - b) on every target row of a sample, ``means`` (2,) float64 = mean reward, mean baseline, and ``adv``
    (D, S) float64 = r - b when given (True allocates).  Returns (roww, means, adv or None)."""
    _require_cuda(reward)
    if reward.dim() != 2 or reward.dtype != torch.float64 or not reward.is_contiguous() or reward.numel() == 0:
        raise ValueError("scst_advantage: reward float64 (D, S), contiguous, non-empty")
    D, S = reward.shape
    T = int(T)
    if not (1 <= D <= 1024 and 1 <= S <= 64 and T >= 1) or (baseline is None and S < 2):
        raise ValueError("scst_advantage: 1 <= D <= 1024, 1 <= S <= 64 (S >= 2 without a baseline), T >= 1")
    dev = reward.device
    a = L.ScstAdvantageArgs()
    if baseline is not None:
        _require_cuda(baseline)
        if baseline.dtype != torch.float64 or baseline.numel() != D or not baseline.is_contiguous():
            raise ValueError("scst_advantage: baseline float64 (D,), contiguous")
        a.baseline = baseline.data_ptr()
    if roww is None:
        roww = torch.empty(D * S, T, dtype=torch.float32, device=dev)
    if means is None:
        means = torch.empty(2, dtype=torch.float64, device=dev)
    if adv is True:
        adv = torch.empty(D, S, dtype=torch.float64, device=dev)
    _require_cuda(roww, means)
    if roww.dtype != torch.float32 or not roww.is_contiguous() or roww.numel() < D * S * T:
        raise ValueError("scst_advantage: roww float32, contiguous, at least D * S * T elements")
    if means.dtype != torch.float64 or means.numel() != 2 or not means.is_contiguous():
        raise ValueError("scst_advantage: means float64 (2,), contiguous")
    if adv is not None:
        _require_cuda(adv)
        if adv.dtype != torch.float64 or adv.numel() != D * S or not adv.is_contiguous():
            raise ValueError("scst_advantage: adv float64 (D, S), contiguous")
        a.adv = adv.data_ptr()
    a.D, a.S, a.T, a.reward, a.roww = D, S, T, reward.data_ptr(), roww.data_ptr()
    a.mean_reward, a.mean_baseline = means.data_ptr(), means.data_ptr() + 8
    L.check(L.load().mtn_scst_advantage(C.byref(a), L.stream_ptr()))
    return roww, means, adv


# ------------------------------------------------------------------------------------------ memory K/V, ahead of the layers
def project_memories(items, lp_dtype, outs=None, n_now=None, order=None):
    """K|V projections (mtn.py:257-258) of CONSTANT memories for many sublayers at once: items = [(mem_lp (B,m,d) compute dtype,
    w_qkv_lp (3d,d), b_qkv (3d,) fp32)] -> list of (B*m, 2d) compute-dtype tensors.  The encoder-side memories (history,
    caption, query, video) are the same tensors in every decoder layer, so their N x (3+F) projections do not depend on
    anything computed inside the layer loop: they run here as a few large grouped GEMMs instead of riding in N x (3+F)
    small per-sublayer launches (and, in the decode path, once per dialogue instead of once per token).
    ``n_now`` (whole-model training forward): only the first n_now items are needed at once; the library may keep the others, in
    the order of their first use (``order``: a permutation of the item indices that keeps the first n_now in front), for compute units that the fused forward launches of the layers leave empty (mtn_kv_project), and computes
    whatever a launch is about to read.  The caller ends the forward with flush_riders()."""
    if not items:
        return []
    code = L.dtype_code(lp_dtype)
    reuse, outs, probs = outs, [], []          # `outs`: write into these buffers (a captured graph keeps reading them)
    for k, (mem_lp, w, b) in enumerate(items):
        Bm = mem_lp.size(0) * mem_lp.size(1)
        d = mem_lp.size(-1)
        kv = reuse[k] if reuse is not None else torch.empty(Bm, 2 * d, device=mem_lp.device, dtype=lp_dtype)
        p = L.GemmProblem()
        p.A, p.B, p.lda, p.ldb, p.M, p.N, p.K = mem_lp.data_ptr(), w.data_ptr() + d * d * w.element_size(), d, d, Bm, 2 * d, d
        p.bias, p.gate_scale, p.out_lp, p.ldc = b.data_ptr() + d * b.element_size(), 1.0, kv.data_ptr(), 2 * d
        outs.append(kv)
        probs.append(p)
    if n_now is not None:
        arr = (L.GemmProblem * len(probs))(*(probs[k] for k in (order if order is not None else range(len(probs)))))
        L.check(L.load().mtn_kv_project(code, len(probs), arr, min(n_now, len(probs)), L.stream_ptr()))
        return outs
    for i in range(0, len(probs), L.GEMM_MAX_GROUP):
        gemm(code, probs[i:i + L.GEMM_MAX_GROUP])
    return outs


def flush_riders():
    """Compute whatever project_memories(..., n_now=...) left waiting (nothing, when every tile found a launch to ride in)."""
    L.check(L.load().mtn_riders_flush(L.stream_ptr()))


# ------------------------------------------------------------------------------------------ fused embeddings
class EmbedNormFn(torch.autograd.Function):
    """Embeddings (lut[tok] * sqrt(d), mtn.py:288-289) + PositionalEncoding (+pe, dropout, mtn.py:307-309) + the Encoder's
    LayerNorm for that stream (mtn.py:83-101), for several token streams in ONE grouped launch; backward = grouped LayerNorm
    backward + one grouped scatter-add into the embedding-table gradients.
    apply(spec, *luts) -> one fp32 tensor per stream.  spec["streams"]: dicts with tokens (B,L) int64, lut (index into luts),
    pe (max_len,d), scale, p (dropout), salt, ln = None | (a2, b2, eps, grad_a, grad_b).  Table gradients are accumulated into
    lut.grad when it exists (flat gradient buffer), else returned."""

    @staticmethod
    def forward(ctx, spec, *luts):
        lib = L.load()
        streams = spec["streams"]
        lp = spec["lp_dtype"]
        code = L.dtype_code(lp) if lp is not None else L.MTN_F32
        dev = luts[0].device
        descs = (L.LnFwdDesc * len(streams))()
        outs, saved = [], []
        for i, st in enumerate(streams):
            tok = st["tokens"].contiguous()
            B, Ls = tok.shape
            d = luts[st["lut"]].size(1)
            rows = B * Ls
            y = torch.empty(B, Ls, d, device=dev, dtype=torch.float32)
            D = descs[i]
            D.rows, D.d, D.tokens, D.lut, D.emb_scale = rows, d, tok.data_ptr(), luts[st["lut"]].data_ptr(), float(st["scale"])
            D.pe, D.seq_len = st["pe"].data_ptr(), Ls
            D.drop = _drop(st["p"], st["salt"], spec["seed"])
            sv = dict(tok=tok, rows=rows, d=d)
            if st["ln"] is not None:
                a2, b2, eps = st["ln"][0], st["ln"][1], st["ln"][2]
                x_save = torch.empty(rows, d, device=dev, dtype=torch.float32)
                mean = torch.empty(rows, device=dev, dtype=torch.float32)
                rstd = torch.empty_like(mean)
                y_lp = torch.empty(B, Ls, d, device=dev, dtype=lp) if (lp is not None and lp != torch.float32) else None
                D.eps, D.a2, D.b2, D.x_out, D.mean, D.rstd = eps, a2.data_ptr(), b2.data_ptr(), x_save.data_ptr(), mean.data_ptr(), rstd.data_ptr()
                D.y_f32, D.y_lp, D.no_ln = y.data_ptr(), L.ptr(y_lp), 0
                sv.update(x=x_save, mean=mean, rstd=rstd, a2=a2, y_lp=y_lp)
            else:
                D.y_f32, D.no_ln = y.data_ptr(), 1
            outs.append(y)
            saved.append(sv)
        L.check(lib.mtn_layernorm_fwd_group(code, len(streams), descs, L.stream_ptr()))
        ctx.spec, ctx.saved_streams, ctx.luts = spec, saved, luts
        ctx.lp_copies = [sv.get("y_lp") for sv in saved]
        spec["_lp_out"] = ctx.lp_copies
        return tuple(outs)

    @staticmethod
    def backward(ctx, *dys):
        lib = L.load()
        spec, saved, luts = ctx.spec, ctx.saved_streams, ctx.luts
        streams = spec["streams"]
        dev = luts[0].device
        queue = spec.get("queue")
        ln_descs, ln_final, emb = [], [], (L.EmbedBwdDesc * len(streams))()
        keep = []
        ret = [None] * len(luts)
        dluts = []
        for j, lut in enumerate(luts):
            if lut.grad is not None:
                dluts.append(lut.grad)
            else:
                g = torch.zeros_like(lut)
                dluts.append(g)
                ret[j] = g
        for i, (st, sv, dy) in enumerate(zip(streams, saved, dys)):
            dy = dy.contiguous() if dy is not None else torch.zeros(sv["rows"], sv["d"], device=dev)
            dx = dy
            if st["ln"] is not None:
                dx = torch.empty(sv["rows"], sv["d"], device=dev, dtype=torch.float32)
                partial = torch.empty(lib.mtn_layernorm_bwd_partial_floats(sv["rows"], sv["d"]), device=dev, dtype=torch.float32)
                ln_descs.append(L.LnBwdDesc(sv["rows"], sv["d"], st["ln"][2], sv["x"].data_ptr(), sv["a2"].data_ptr(), sv["mean"].data_ptr(),
                                            sv["rstd"].data_ptr(), dy.data_ptr(), None, dx.data_ptr(), partial.data_ptr()))
                ga, gb = st["ln"][3], st["ln"][4]
                ln_final.append((L.LnFinalizeDesc(partial.data_ptr(), lib.mtn_layernorm_bwd_nparts(sv["rows"]), sv["d"], ga.data_ptr(), gb.data_ptr()), partial))
            keep += [dy, dx]
            E = emb[i]
            E.rows, E.d, E.tokens, E.dx, E.emb_scale = sv["rows"], sv["d"], sv["tok"].data_ptr(), dx.data_ptr(), float(st["scale"])
            E.drop = _drop(st["p"], st["salt"], spec["seed"])
            E.dlut = dluts[st["lut"]].data_ptr()
            E.lut_rows = luts[st["lut"]].size(0)
        if ln_descs:
            arr = (L.LnBwdDesc * len(ln_descs))(*ln_descs)
            L.check(lib.mtn_layernorm_bwd_group(len(ln_descs), arr, L.stream_ptr()))
            if queue is not None:
                for desc, partial in ln_final:
                    queue.add(queue.dtype, [], desc, [partial])
            else:
                farr = (L.LnFinalizeDesc * len(ln_final))(*[f[0] for f in ln_final])
                L.check(lib.mtn_layernorm_bwd_finalize(len(ln_final), farr, L.stream_ptr()))
        if queue is not None and all(r is None for r in ret):
            # every table's gradient lives in the flat gradient buffer: the scatter can wait for the end of backward and share its
            # launch with the other tables' (the queue's flush); dx / dy stay alive in the queue until then
            queue.add_embed([emb[i] for i in range(len(streams))], keep)
        else:
            L.check(lib.mtn_embed_bwd_group(len(streams), emb, L.stream_ptr()))
        return (None, *ret)


# ------------------------------------------------------------------------------------------ feature streams
class FeatureEncodeFn(torch.autograd.Function):
    """vid_encoder of mtn.py:378 for ALL feature streams at once: Linear(ft_i, d) -> ReLU -> + positional encoding -> dropout,
    followed by that stream's Encoder LayerNorm (mtn.py:83-101).  Forward = one grouped cast of the features, one grouped
    MFMA GEMM (bias + ReLU in the epilogue), one grouped LayerNorm launch (PE, dropout, LN, compute-dtype copy); backward =
    grouped LayerNorm backward, one grouped mask+cast (dropout, ReLU), dW/db GEMMs on the deferred queue.
    apply(spec, *weights) -> one fp32 (B, V_i, d) tensor per stream.  spec["streams"]: dicts with x (B,V,ft) fp32, w (index),
    w_lp, bias, grad_w, grad_b, pe, p, salt, ln = (a2, b2, eps, grad_a, grad_b).  Features get no gradient (inputs)."""

    @staticmethod
    def forward(ctx, spec, *weights):
        lib = L.load()
        streams, lp = spec["streams"], spec["lp_dtype"]
        code = L.dtype_code(lp)
        dev = weights[0].device
        n = len(streams)
        casts = (L.CastDesc * n)()
        probs, lns, saved, outs = [], (L.LnFwdDesc * n)(), [], []
        for i, st in enumerate(streams):
            x = st["x"].contiguous()
            B, V, F = x.shape
            d = st["w_lp"].size(0)
            rows = B * V
            x_lp = torch.empty(rows, F, device=dev, dtype=lp)
            casts[i].n, casts[i].src, casts[i].dst = rows * F, x.data_ptr(), x_lp.data_ptr()
            h = torch.empty(rows, d, device=dev, dtype=torch.float32)
            p = L.GemmProblem()
            p.A, p.B, p.lda, p.ldb, p.M, p.N, p.K = x_lp.data_ptr(), st["w_lp"].data_ptr(), F, F, rows, d, F
            p.bias, p.relu, p.gate_scale, p.out_f32, p.ldc = st["bias"].data_ptr(), 1, 1.0, h.data_ptr(), d
            probs.append(p)
            a2, b2, eps = st["ln"][0], st["ln"][1], st["ln"][2]
            y = torch.empty(B, V, d, device=dev, dtype=torch.float32)
            y_lp = torch.empty(B, V, d, device=dev, dtype=lp) if lp != torch.float32 else None
            xs = torch.empty(rows, d, device=dev, dtype=torch.float32)
            mean = torch.empty(rows, device=dev, dtype=torch.float32)
            rstd = torch.empty_like(mean)
            D = lns[i]
            D.rows, D.d, D.eps, D.x, D.a2, D.b2 = rows, d, eps, h.data_ptr(), a2.data_ptr(), b2.data_ptr()
            D.pe, D.seq_len, D.drop = st["pe"].data_ptr(), V, _drop(st["p"], st["salt"], spec["seed"])
            D.x_out, D.mean, D.rstd, D.y_f32, D.y_lp = xs.data_ptr(), mean.data_ptr(), rstd.data_ptr(), y.data_ptr(), L.ptr(y_lp)
            outs.append(y)
            saved.append(dict(x_lp=x_lp, h=h, xs=xs, mean=mean, rstd=rstd, rows=rows, d=d, F=F, y_lp=y_lp, a2=a2))
        if lp != torch.float32:
            L.check(lib.mtn_cast_group(code, n, casts, L.stream_ptr()))
        else:
            for sv, st in zip(saved, streams):
                sv["x_lp"].copy_(st["x"].reshape(sv["rows"], sv["F"]))
        gemm(code, probs)
        L.check(lib.mtn_layernorm_fwd_group(code, n, lns, L.stream_ptr()))
        ctx.spec, ctx.saved_streams, ctx.n_w = spec, saved, len(weights)
        spec["_lp_out"] = [sv["y_lp"] for sv in saved]
        return tuple(outs)

    @staticmethod
    def backward(ctx, *dys):
        lib = L.load()
        spec, saved = ctx.spec, ctx.saved_streams
        streams, lp = spec["streams"], spec["lp_dtype"]
        code = L.dtype_code(lp)
        queue = spec.get("queue")
        n = len(streams)
        dev = saved[0]["h"].device
        lnb = (L.LnBwdDesc * n)()
        casts = (L.CastDesc * n)()
        probs, finals, keep = [], [], []
        for i, (st, sv, dy) in enumerate(zip(streams, saved, dys)):
            rows, d, F = sv["rows"], sv["d"], sv["F"]
            dy = dy.contiguous() if dy is not None else torch.zeros(rows, d, device=dev)
            dxs = torch.empty(rows, d, device=dev, dtype=torch.float32)
            partial = torch.empty(lib.mtn_layernorm_bwd_partial_floats(rows, d), device=dev, dtype=torch.float32)
            B_ = lnb[i]
            B_.rows, B_.d, B_.eps, B_.x, B_.a2, B_.mean, B_.rstd = rows, d, st["ln"][2], sv["xs"].data_ptr(), sv["a2"].data_ptr(), sv["mean"].data_ptr(), sv["rstd"].data_ptr()
            B_.g, B_.dx, B_.partial = dy.data_ptr(), dxs.data_ptr(), partial.data_ptr()
            finals.append((L.LnFinalizeDesc(partial.data_ptr(), lib.mtn_layernorm_bwd_nparts(rows), d, st["ln"][3].data_ptr(), st["ln"][4].data_ptr()), partial))
            dh = torch.empty(rows, d, device=dev, dtype=lp)
            casts[i].n, casts[i].src, casts[i].dst = rows * d, dxs.data_ptr(), dh.data_ptr()
            casts[i].drop, casts[i].gate = _drop(st["p"], st["salt"], spec["seed"]), sv["h"].data_ptr()
            p = L.GemmProblem()      # dW = dh^T x, db = column sums of dh
            p.A, p.B, p.lda, p.ldb, p.M, p.N, p.K, p.a_trans, p.b_trans = dh.data_ptr(), sv["x_lp"].data_ptr(), d, F, d, F, rows, 1, 1
            p.gate_scale, p.out_f32, p.ldc, p.rowsum_out = 1.0, st["grad_w"].data_ptr(), F, st["grad_b"].data_ptr()
            probs.append(p)
            keep += [dy, dxs, dh, sv["x_lp"], sv["h"]]
        L.check(lib.mtn_layernorm_bwd_group(n, lnb, L.stream_ptr()))
        L.check(lib.mtn_cast_group(code, n, casts, L.stream_ptr()))
        if queue is not None:
            for k, (desc, partial) in enumerate(finals):
                queue.add(code, [probs[k]], desc, [partial] + (keep if k == 0 else []))
        else:
            gemm(code, probs)
            farr = (L.LnFinalizeDesc * n)(*[f[0] for f in finals])
            L.check(lib.mtn_layernorm_bwd_finalize(n, farr, L.stream_ptr()))
        return (None,) + (None,) * ctx.n_w


# ------------------------------------------------------------------------------------------ loss head
def _per_stream(vals, rows, key, what):
    """``vals`` (of spec[key]) as a list of one entry per stream."""
    if len(vals) != len(rows):
        raise ValueError("GeneratorLossFn: spec['%s'] holds one %s per stream" % (key, what))
    return list(vals)


def _check_distill(spec, rows, V, dev):
    """The teachers per stream (a tensor or None), alpha and the temperature; None when no stream has a teacher."""
    if spec.get("teacher") is None or all(q is None for q in spec["teacher"]):
        return None
    teachers = _per_stream(spec["teacher"], rows, "teacher", "entry (a tensor or None)")
    alpha, T = float(spec.get("alpha", 0.5)), float(spec.get("temperature", 1.0))
    if not (0.0 <= alpha <= 1.0) or not (T > 0.0 and math.isfinite(T)):
        raise ValueError("GeneratorLossFn: alpha in [0, 1] and a finite temperature > 0")
    for q, r in zip(teachers, rows):
        if q is None:
            continue
        if not (torch.is_tensor(q) and q.device == dev and q.dtype == torch.float32 and q.dim() == 2 and tuple(q.shape) == (r, V)
                and q.stride(1) == 1 and q.stride(0) >= V and q.stride(0) % 4 == 0 and q.data_ptr() % 16 == 0):
            raise ValueError("GeneratorLossFn: a teacher is an fp32 (rows, V) tensor on the student's device, unit column stride, row stride a "
                             "multiple of 4, 16-byte aligned")
        if q.requires_grad:
            raise ValueError("GeneratorLossFn: teacher rows carry no gradient (detach them)")
    return teachers, alpha, T


def _check_weighted(spec, rows, V, dev):
    """(weights per stream: a tensor or None, smoothing per stream: a float, negative = the spec's); None when neither key is given."""
    weights, sms = spec.get("row_weights"), spec.get("smoothing_seg")
    if (weights is None or all(w is None for w in weights)) and sms is None:
        return None
    weights = [None] * len(rows) if weights is None else list(weights)
    sms = [-1.0] * len(rows) if sms is None else [-1.0 if s is None else float(s) for s in sms]
    if len(weights) != len(rows) or len(sms) != len(rows):
        raise ValueError("GeneratorLossFn: spec['row_weights'] and spec['smoothing_seg'] hold one entry per stream")
    if any(math.isnan(s) for s in sms):
        raise ValueError("GeneratorLossFn: a stream's smoothing is a number (negative: the spec's smoothing)")
    for w, r in zip(weights, rows):
        if w is None:
            continue
        if not (torch.is_tensor(w) and w.device == dev and w.dtype == torch.float32 and w.numel() == r and w.is_contiguous()):
            raise ValueError("GeneratorLossFn: row weights are a contiguous fp32 tensor of one value per row on the logits' device")
        if w.requires_grad:
            raise ValueError("GeneratorLossFn: row weights carry no gradient (detach them)")
    return weights, sms


def _check_alpha_ints(key, name, what, fits, misfit):
    """The validator of a head that is spec[key] = (alpha, per stream an int or None): (alpha, [int per stream, 0 = none]); None when the
    key is absent, alpha is 0 or no stream has an int (the plain head runs)."""
    def check(spec, rows, V, dev):
        if spec.get(key) is None:
            return None
        alpha = float(spec[key][0])
        if not (alpha >= 0.0 and math.isfinite(alpha)):
            raise ValueError("GeneratorLossFn: the %s alpha is finite and >= 0" % name)
        ints = [0 if n is None else int(n) for n in _per_stream(spec[key][1], rows, key, what + " (an int or None)")]
        if any(n < 0 or (n > 0 and not fits(r, n)) for n, r in zip(ints, rows)):
            raise ValueError("GeneratorLossFn: " + misfit)
        return (alpha, ints) if alpha != 0.0 and any(ints) else None
    return check


def _fill_distill(A, p, R, dev):
    teachers, A.alpha, A.temperature = p
    for i, q in enumerate(teachers):
        if q is not None:
            A.teacher[i], A.ldq[i] = q.data_ptr(), q.stride(0)
    rowkd = torch.empty(R, device=dev, dtype=torch.float32)
    A.rowkd = rowkd.data_ptr()
    return [rowkd]


def _fill_weighted(A, p, R, dev):
    for i, (w, sm) in enumerate(zip(*p)):
        A.roww[i], A.smoothing_seg[i] = L.ptr(w), sm
    return []


def _fill_alpha_ints(alpha, ints, *row_fields):
    """The fill of such a head: its alpha, its int per stream, and one fp32 row buffer per field of ``row_fields``."""
    def fill(A, p, R, dev):
        setattr(A, alpha, p[0])
        for i, n in enumerate(p[1]):
            getattr(A, ints)[i] = n
        made = [torch.empty(R, device=dev, dtype=torch.float32) for _ in row_fields]
        for f, t in zip(row_fields, made):
            setattr(A, f, t.data_ptr())
        return made
    return fill


@dataclass(frozen=True)
class LossHead:
    """One form of the loss head (csrc/losshead.hip).  ``keys``: the spec keys that switch it on; ``check(spec, rows, V, dev)``: its
    validator, None = the spec does not ask for it, else its parameters; ``args`` / ``entry``: the lib.py argument struct and the stem of
    the mtn_<entry>_fwd / _bwd entry points; ``fill(A, parameters, R, dev)`` writes the form's fields and returns the tensors it allocated,
    the form's extra row term first; ``sum_key``: the spec key that term's sum is left under; ``label``: how a conflict names the form."""
    keys: tuple
    check: Optional[Callable]
    args: str
    entry: str
    fill: Optional[Callable] = None
    sum_key: Optional[str] = None
    label: str = ""


# At most one form besides "plain" per call (each is the plain head with one extra term: include/mtn_hip.h).  The validators run in this
# order, and a conflict names the last form asked for, then the first.
LOSS_HEADS = {
    "distill": LossHead(("teacher", "alpha", "temperature"), _check_distill, "DistillHeadArgs", "distill", _fill_distill, "kd_sum",
                        "teacher soft targets"),
    "weighted": LossHead(("row_weights", "smoothing_seg"), _check_weighted, "WLossHeadArgs", "wlosshead", _fill_weighted, None, "row weights"),
    "unlikelihood": LossHead(("unlikelihood",), _check_alpha_ints("unlikelihood", "unlikelihood", "sequence length", lambda r, T: r % T == 0,
                                                                  "a stream's rows are a multiple of its sequence length"),
                             "ULossHeadArgs", "ulosshead", _fill_alpha_ints("ul_alpha", "seq_len", "rowul"), "ul_sum", "unlikelihood"),
    "rdrop": LossHead(("rdrop",), _check_alpha_ints("rdrop", "R-Drop", "pair distance", lambda r, N: r == 2 * N,
                                                    "a paired stream holds 2 N rows, N its pair distance"),
                      "RLossHeadArgs", "rlosshead", _fill_alpha_ints("rd_alpha", "pair", "rowrd", "rowkl"), "rd_sum", "R-Drop"),
    "plain": LossHead((), None, "LossHeadArgs", "losshead"),
}


def one_loss_head(asked, prefix=""):
    """The one form among ``asked`` (kinds, in LOSS_HEADS' order), "plain" for none; two do not combine."""
    if len(asked) > 1:
        a, b = LOSS_HEADS[asked[-1]].label, LOSS_HEADS[asked[0]].label
        raise ValueError("%s%s %s not combine with %s" % (prefix, a, "do" if a.endswith("s") else "does", b))
    return asked[0] if asked else "plain"


class GeneratorLossFn(torch.autograd.Function):
    """sum_i coef_i * KLDiv(log_softmax(x_i W_i^T + b_i), smooth(y_i)) / norm_i  — Generator (mtn.py:62-69) +
    LabelSmoothing (label_smoothing.py) + SimpleLossCompute's weighted sum (data_utils.py:133-144) as: one grouped cast,
    one grouped GEMM (logits), one row kernel (log-sum-exp + closed-form KL); backward: one row kernel (dlogits), two
    grouped GEMMs (dX, dW+db).  `spec`: targets, norms (device float scalars), coefs, gens [(w_lp, bias, grad_w, grad_b)],
    vocab, pad, smoothing, lp_dtype.  Generator gradients are written to the flat gradient buffer (not returned).
    One more term on any stream (LOSS_HEADS: at most one form per call) puts that form's row kernels, mtn_<entry>_fwd / _bwd of
    csrc/losshead.hip (include/mtn_hip.h gives the formulas), in the place of the two loss-head calls, casts and GEMMs unchanged:
    knowledge distillation: ``spec["teacher"]`` = per stream a (rows_i, V) fp32 device tensor of teacher logits / log-probabilities or
    None, with ``spec["alpha"]`` and ``spec["temperature"]``; ``spec["kd_sum"]`` is left holding the device scalar sum_rows kd;
    signed row weights (self-critical sequence training): ``spec["row_weights"]`` = per stream a contiguous fp32 device tensor of one weight
    per row or None (all ones), ``spec["smoothing_seg"]`` = per stream a smoothing or None (the spec's);
    unlikelihood training (Welleck et al. 2019): ``spec["unlikelihood"]`` = (alpha > 0, per stream the sequence length T of its (B, T)
    targets or None); ``spec["ul_sum"]`` is left holding the device scalar sum_rows ul;
    R-Drop (Liang et al. 2021): ``spec["rdrop"]`` = (alpha > 0, per stream the pair distance N of its 2 N rows — rows i and i + N are two
    passes of one position — or None); ``spec["rd_sum"]`` is left holding the device scalar sum_rows rd."""

    @staticmethod
    def forward(ctx, spec, *xs):
        lib = L.load()
        lp = spec["lp_dtype"]
        code = L.dtype_code(lp)
        dev = xs[0].device
        d, V = xs[0].size(-1), spec["vocab"]
        rows = [x.numel() // d for x in xs]
        R = sum(rows)
        # inputs that are consecutive row ranges of one compute-dtype buffer already (layer_norm_group): no cast
        ready, off = None, 0
        for i, x in enumerate(xs):
            tag = getattr(x, "_mtn_lp_rows", None)
            if tag is None or tag[1] != off or tag[2] != rows[i] or tag[0].dtype != lp or (ready is not None and tag[0] is not ready):
                ready = None
                break
            ready, off = tag[0], off + rows[i]
        if ready is not None and ready.size(0) != R:
            ready = None
        x_lp = ready if ready is not None else torch.empty(R, d, device=dev, dtype=lp)
        logits = torch.empty(R, V, device=dev, dtype=torch.float32)
        casts = (L.CastDesc * len(xs))()
        off = 0
        offs = []
        for i, x in enumerate(xs):
            xc = x.contiguous()
            casts[i].n, casts[i].src, casts[i].dst = xc.numel(), xc.data_ptr(), x_lp[off:off + rows[i]].data_ptr()
            casts[i].drop = L.Dropout(0.0, 0, None)
            offs.append(off)
            off += rows[i]
            ctx_keep = xc
        if ready is not None:
            pass
        elif lp == torch.float32:
            for i, x in enumerate(xs):
                x_lp[offs[i]:offs[i] + rows[i]].copy_(x.reshape(rows[i], d))
        else:
            L.check(lib.mtn_cast_group(code, len(xs), casts, L.stream_ptr()))
        gens = spec["gens"]
        shared = all(g[0].data_ptr() == gens[0][0].data_ptr() for g in gens)
        segs = [(0, R, gens[0])] if shared else [(offs[i], rows[i], gens[i]) for i in range(len(xs))]
        probs = []
        for o, r, (w_lp, bias, _gw, _gb, *_rest) in segs:
            p = L.GemmProblem()
            p.A, p.B, p.lda, p.ldb, p.M, p.N, p.K = x_lp[o:].data_ptr(), w_lp.data_ptr(), d, d, r, V, d
            p.bias, p.gate_scale, p.out_f32, p.ldc = bias.data_ptr(), 1.0, logits[o:].data_ptr(), V
            probs.append(p)
        gemm(code, probs)
        params = {kind: p for kind, h in LOSS_HEADS.items() if h.check is not None for p in [h.check(spec, rows, V, dev)] if p is not None}
        head = LOSS_HEADS[one_loss_head(list(params), "GeneratorLossFn: ")]
        params = next(iter(params.values()), None)
        A = getattr(L, head.args)()
        A.n_seg = len(xs)
        norms = [n.float().reshape(1) if n.dtype != torch.float32 or n.dim() == 0 else n for n in spec["norms"]]
        targets = [t.contiguous().view(-1) for t in spec["targets"]]
        for i in range(len(xs)):
            A.rows[i], A.target[i], A.norm[i], A.coef[i] = rows[i], targets[i].data_ptr(), norms[i].data_ptr(), float(spec["coefs"][i])
        A.V, A.ldz, A.pad, A.smoothing = V, V, spec["pad"], float(spec["smoothing"])
        lse = torch.empty(R, device=dev, dtype=torch.float32)
        rowloss = torch.empty(R, device=dev, dtype=torch.float32)
        A.logits, A.lse, A.rowloss = logits.data_ptr(), lse.data_ptr(), rowloss.data_ptr()
        made = head.fill(A, params, R, dev) if head.fill is not None else []
        L.check(getattr(lib, "mtn_%s_fwd" % head.entry)(C.byref(A), L.stream_ptr()))
        if head.sum_key is not None:
            spec[head.sum_key] = made[0].sum()
        ctx.args, ctx.bwd = A, getattr(lib, "mtn_%s_bwd" % head.entry)
        ctx.keep = (x_lp, logits, lse, norms, targets, params, made)      # (everything ctx.args points to: the form's inputs and its rows)
        ctx.meta = (spec, segs, rows, offs, d, V, R, code, [x.shape for x in xs])
        return rowloss.sum()

    @staticmethod
    def backward(ctx, g):
        spec, segs, rows, offs, d, V, R, code, shapes = ctx.meta
        x_lp, logits, lse = ctx.keep[:3]                      # (the rest is kept alive for the pointers in ctx.args)
        lp = spec["lp_dtype"]
        dev = x_lp.device
        A = ctx.args
        gl = g.contiguous().float().reshape(1)
        dlogits = torch.empty(R, V, device=dev, dtype=lp)
        A.gloss, A.dlogits, A.ldd = gl.data_ptr(), dlogits.data_ptr(), V
        L.check(ctx.bwd(code, C.byref(A), L.stream_ptr()))
        dx = torch.empty(R, d, device=dev, dtype=torch.float32)
        p_dx, p_dw = [], []
        for o, r, (w_lp, bias, gw, gb, *rest) in segs:
            p = L.GemmProblem()      # dX = dlogits W  (through the transposed weight copy when the model keeps one)
            w_lpT = rest[0] if rest else None
            if w_lpT is not None:
                p.A, p.B, p.lda, p.ldb, p.M, p.N, p.K, p.b_trans = dlogits[o:].data_ptr(), w_lpT.data_ptr(), V, V, r, d, V, 0
            else:
                p.A, p.B, p.lda, p.ldb, p.M, p.N, p.K, p.b_trans = dlogits[o:].data_ptr(), w_lp.data_ptr(), V, d, r, d, V, 1
            p.gate_scale, p.out_f32, p.ldc = 1.0, dx[o:].data_ptr(), d
            p_dx.append(p)
            q = L.GemmProblem()      # dW = dlogits^T x, db = column sums of dlogits
            q.A, q.B, q.lda, q.ldb, q.M, q.N, q.K, q.a_trans, q.b_trans = dlogits[o:].data_ptr(), x_lp[o:].data_ptr(), V, d, V, d, r, 1, 1
            q.gate_scale, q.out_f32, q.ldc, q.rowsum_out = 1.0, gw.data_ptr(), d, gb.data_ptr()
            p_dw.append(q)
        gemm(code, p_dx)
        queue = spec.get("queue")
        if queue is not None and queue.adam is not None:
            queue.add(code, p_dw, None, [dlogits, x_lp])      # with the optimiser epilogue: one of the problems of the table launch
        else:
            gemm(code, p_dw)
        return (None,) + tuple(dx[offs[i]:offs[i] + rows[i]].view(shapes[i]) for i in range(len(rows)))


# ------------------------------------------------------------------------------------------ attention core (tests / decode)
def attention(q, k, v, mask, heads: int, p_drop: float = 0.0, seed=None, salt: int = 0):
    """mtn.py:221-231 on packed-head layouts: q (B,a,d), k/v (B,m,d) of the compute dtype.  Returns (o, lse)."""
    _require_cuda(q, k, v)
    B, a, d = q.shape
    m = k.size(1)
    q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
    o = torch.empty_like(q)
    lse = torch.empty(2 * B * heads * a, device=q.device, dtype=torch.float32)
    mask_u8, sb, sq = _mask_u8(mask, B, a, m)
    args = L.AttnArgs()
    args.B, args.h, args.a, args.m, args.dk = B, heads, a, m, d // heads
    args.q, args.k, args.v, args.ldq, args.ldkv = q.data_ptr(), k.data_ptr(), v.data_ptr(), d, d
    args.mask, args.mask_sb, args.mask_sq = L.ptr(mask_u8), sb, sq
    args.drop = _drop(p_drop, salt, seed)
    args.o, args.ldo, args.lse = o.data_ptr(), d, lse.data_ptr()
    L.check(L.load().mtn_attention_fwd(L.dtype_code(q.dtype), C.byref(args), L.stream_ptr()))
    return o, lse


def attention_bwd(q, k, v, o, lse, d_o, mask, heads: int, p_drop: float = 0.0, seed=None, salt: int = 0):
    B, a, d = q.shape
    m = k.size(1)
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    mask_u8, sb, sq = _mask_u8(mask, B, a, m)
    args = L.AttnArgs()
    args.B, args.h, args.a, args.m, args.dk = B, heads, a, m, d // heads
    args.q, args.k, args.v, args.ldq, args.ldkv = q.data_ptr(), k.data_ptr(), v.data_ptr(), d, d
    args.mask, args.mask_sb, args.mask_sq = L.ptr(mask_u8), sb, sq
    args.drop = _drop(p_drop, salt, seed)
    args.o, args.ldo, args.lse = o.data_ptr(), d, lse.data_ptr()
    args.d_o, args.dq, args.dk_out, args.dv_out = d_o.contiguous().data_ptr(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr()
    kv_acc = None
    if a > 32 and q.dtype != torch.float32:      # several query-block passes: their dK / dV sums stay in fp32 until the last one
        kv_acc = torch.empty(2, B * m, d, device=q.device, dtype=torch.float32)
        args.kv_acc = kv_acc.data_ptr()
    L.check(L.load().mtn_attention_bwd(L.dtype_code(q.dtype), C.byref(args), L.stream_ptr()))
    return dq, dk, dv


# ------------------------------------------------------------------------------------------ un-fused operator forms
class AttentionCoreFn(torch.autograd.Function):
    """attention() of mtn.py:221-231 with autograd, on (B,L,d) packed-head tensors of the compute dtype."""

    @staticmethod
    def forward(ctx, q, k, v, mask, heads, p_drop, seed, salt):
        o, lse = attention(q, k, v, mask, heads, p_drop, seed, salt)
        ctx.save_for_backward(q.contiguous(), k.contiguous(), v.contiguous(), o, lse)
        ctx.meta = (mask, heads, p_drop, seed, salt)
        return o

    @staticmethod
    def backward(ctx, d_o):
        q, k, v, o, lse = ctx.saved_tensors
        mask, heads, p_drop, seed, salt = ctx.meta
        dq, dk, dv = attention_bwd(q, k, v, o, lse, d_o.to(q.dtype), mask, heads, p_drop, seed, salt)
        return dq, dk, dv, None, None, None, None, None


class LinearFn(torch.autograd.Function):
    """y = [relu](x W^T + b) on the MFMA GEMM (nn.Linear as used at mtn.py:243-244,273-276,378)."""

    @staticmethod
    def forward(ctx, x, w, b, lp_dtype, relu, out_f32):
        _require_cuda(x, w)
        code = L.dtype_code(lp_dtype)
        K, N = w.size(1), w.size(0)
        x2 = x.reshape(-1, K)
        x_lp = x2.contiguous() if x2.dtype == lp_dtype else cast_to_lp(x2.float(), lp_dtype)
        w_lp = w.contiguous() if w.dtype == lp_dtype else cast_to_lp(w.float(), lp_dtype)
        M = x_lp.size(0)
        out = torch.empty(M, N, device=x.device, dtype=torch.float32 if out_f32 else lp_dtype)
        p = L.GemmProblem()
        p.A, p.B, p.lda, p.ldb, p.M, p.N, p.K = x_lp.data_ptr(), w_lp.data_ptr(), K, K, M, N, K
        p.bias, p.relu, p.gate_scale, p.ldc = L.ptr(b), int(relu), 1.0, N
        if out.dtype == torch.float32:
            p.out_f32 = out.data_ptr()
        else:
            p.out_lp = out.data_ptr()
        gemm(code, [p])
        ctx.save_for_backward(x_lp, w_lp, out if relu else None)
        ctx.meta = (lp_dtype, relu, x.shape, x.dtype, b is not None)
        return out.view(*x.shape[:-1], N)

    @staticmethod
    def backward(ctx, dy):
        x_lp, w_lp, out = ctx.saved_tensors
        lp_dtype, relu, xshape, xdtype, has_b = ctx.meta
        code = L.dtype_code(lp_dtype)
        M, K = x_lp.shape
        N = w_lp.size(0)
        dy2 = dy.reshape(M, N)
        if relu:
            dy2 = dy2 * (out > 0).to(dy2.dtype)
        dy_lp = dy2.contiguous() if dy2.dtype == lp_dtype else cast_to_lp(dy2.float(), lp_dtype)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty(M, K, device=dy.device, dtype=torch.float32)
            p = L.GemmProblem()
            p.A, p.B, p.lda, p.ldb, p.M, p.N, p.K, p.b_trans = dy_lp.data_ptr(), w_lp.data_ptr(), N, K, M, K, N, 1
            p.gate_scale, p.out_f32, p.ldc = 1.0, dx.data_ptr(), K
            gemm(code, [p])
            dx = dx.view(xshape).to(xdtype)
        dw = torch.empty(N, K, device=dy.device, dtype=torch.float32)
        db = torch.empty(N, device=dy.device, dtype=torch.float32)
        p = L.GemmProblem()
        p.A, p.B, p.lda, p.ldb, p.M, p.N, p.K, p.a_trans, p.b_trans = dy_lp.data_ptr(), x_lp.data_ptr(), N, K, N, K, M, 1, 1
        p.gate_scale, p.out_f32, p.ldc, p.rowsum_out = 1.0, dw.data_ptr(), K, db.data_ptr()
        gemm(code, [p])
        return dx, dw, (db if has_b else None), None, None, None


def linear(x, w, b, lp_dtype=torch.bfloat16, relu=False, out_f32=False):
    return LinearFn.apply(x, w, b, lp_dtype, relu, out_f32)
