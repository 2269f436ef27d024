"""Decode path (BASELINE configs[4]): greedy / beam search over the MTN decoder for ONE dialogue, as generate.py drives it
through data_utils.py:159-242, on the HIP kernels.

What the reference does per generated token (data_utils.py:200-205): for EVERY live hypothesis, one full ``model.decode`` of
its prefix — which re-runs all N decoder layers *including the auto-encoder chains*, although those chains depend only on
the dialogue (query/caption, video), never on the target prefix.  Here:

* the encoder side and the N x F auto-encoder chains run ONCE per dialogue (``DecoderLayer.forward_ae_chains``);
* all live hypotheses are decoded together, as the batch dimension of one target-stream pass
  (``DecoderLayer.forward_target``: 4 text attentions + F attend-to-auto-encoder + FFN per layer);
* the pass has a FIXED shape — (width, max_len) tokens under the causal mask, log-probabilities read at position l — so the
  whole pass is ONE hipGraph replayed per token (launch-latency-bound at the reference's max_len = 20);
* for longer searches (``kv_cache``, default above KV_CACHE_FROM tokens) the pass covers only the NEWEST position: every layer
  keeps K|V of the target prefix per hypothesis, the new row's K|V are projected into it, and the self-attention of that row is
  a cross-attention over the cache (keys 0..l enabled); a beam step re-orders hypotheses, so the cache rows follow their
  parents by one gather per token.  Same n-best lists as the full-prefix pass (tested), O(l) instead of O(l^2) work per token;
* hypothesis bookkeeping stays on the host exactly as in the reference (same candidate order, same tie behaviour).

The opposite question — how likely does the model find a GIVEN response — is ``score_candidates``: the same loaded session, the
candidates as the rows of ONE teacher-forced pass (``DecodeSession._pass_score``: the generator's logits at every position, then
csrc/score.hip: per-token log-probability and rank, per-row float64 sum), scored as the beam search scores a finished hypothesis.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import copy
import ctypes as C
import logging
import math
import os

import numpy as np
import torch

from . import lib as L
from . import ops
from .data_utils import subsequent_mask


def _capture(body):
    """``body`` as a graph: one warm-up run on a side stream (lazy allocations and library set-up happen outside the capture), then the
    capture itself — the body runs exactly twice.  The caller replays the returned graph."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        body()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with L.capturing(g):
        body()
    return g


class DecodeSession:
    """Everything about one dialogue that does not depend on the target prefix, plus the replayable target-stream pass.
    A session is reusable for further dialogues of the same shapes (``load``): buffers and the captured graph persist."""

    def __init__(self, model, batch, max_len: int, width: int, pad: int = 1, use_graph: bool = True, kv_cache: bool = False,
                 select=None, share=None):
        # share: another session of the same shape whose per-step inputs (tokens, pos, the cache's parent row) this one reads instead of
        # allocating its own — the members of an Ensemble session all read ONE set
        self.model, self.width, self.max_len, self.pad = model, width, max_len, pad
        self.kv_cache = bool(kv_cache)
        # select = (k, column): the pass also leaves, per row, its k largest log-probabilities, their columns and that column's
        # value in self.top (ops.topk_rows, inside the captured graph): the beam search reads only that
        self.select = select if (select is not None and batch.query.is_cuda) else None
        self.top = None
        self.use_graph = use_graph and batch.query.is_cuda
        dev = batch.query.device
        self.q = self.cp = self.hs = self.aes = self.masks = None
        self._kvs, self._kv_pairs = None, []
        self.D = batch.query.size(0)
        self.tokens = share.tokens if share is not None else torch.full((self.D * width, max_len), pad, dtype=torch.long, device=dev)
        self.pos = share.pos if share is not None else torch.zeros(1, dtype=torch.long, device=dev)
        self.trg_mask = subsequent_mask(max_len, device=dev)       # (1, L, L): data_utils.py:204 uses the causal mask only
        ops.prepare_masks(self.trg_mask)
        self.logp = None
        self._graph = None
        self._static = None                   # load(): a private copy of the dialogue's inputs that a captured encoder-side pass reads
        self._load_graph = None
        self._loads = 0
        # contrastive_log: the search's settings (frozen into its captured body), its device state [cand_logp | step | done | logs], the
        # views of it and the captured body; a search with other settings replaces all four
        self._cs_key = self._cs_state = self._cs_views = self._cs_graph = None
        self.load(batch)
        if self.kv_cache:
            # Prefix K/V cache of the target self-attention (the reference recomputes the whole prefix for every hypothesis and
            # token, data_utils.py:197-205): per layer (W, L, 2d) in the compute dtype, TWO copies — a beam step re-orders the
            # hypotheses, so the rows of the cache follow their parents by one gather from the other copy per token.
            W, L, d = self.D * width, max_len, model.decoder.layers[0].size
            lp = model.compute_dtype
            nl = len(model.decoder.layers)
            self._cache = [torch.zeros(nl, W, L, 2 * d, device=dev, dtype=lp) for _ in range(2)]
            self._cur = 0
            self._parent = share._parent if share is not None else torch.arange(W, device=dev)
            self._self_mem = torch.zeros(W, L, d, device=dev, dtype=torch.float32)      # shape carrier (never read: K|V are ready)
            self._self_mem._mtn_lp = torch.zeros(W, L, d, device=dev, dtype=lp) if lp != torch.float32 else self._self_mem
            self._self_mask = torch.zeros(W, 1, L, dtype=torch.bool, device=dev)
            self._self_mask._mtn_u8 = torch.zeros(W, 1, L, dtype=torch.uint8, device=dev)
            self._prev = None                                                            # prefixes of the previous step, per dialogue
            self._graphs = {}

    @staticmethod
    def signature(model, batch, max_len, width):
        ident = model.signature() if isinstance(model, Ensemble) else (id(model), model._flat.data_ptr() if model._flat is not None else 0, model.compute_dtype)
        return ident + (width, max_len, tuple(batch.query.shape), tuple(batch.his.shape),
                tuple(batch.cap.shape), tuple(tuple(f.shape) for f in (batch.fts or [])), str(batch.query.device))

    def load(self, batch):
        """Encoder side + the N x F auto-encoder chains of a new dialogue (target-independent: once per dialogue).  A batch of
        D dialogues is decoded side by side: every per-dialogue tensor is repeated `width` times along the batch dimension
        (rows d*width .. d*width+width-1 belong to dialogue d).
        The pass is ~100 small launches, host-bound when issued one by one (2-3 ms per dialogue — a fifth of a 20-token beam search):
        from the third dialogue of a shape on, the inputs are copied into a private static Batch and the whole pass is ONE graph replay."""
        model = self.model
        if model.training:                       # (nn.Module.eval() walks every submodule: ~1 ms of Python per dialogue)
            model.eval()
        model.prepare()
        self._loads += 1
        # what a captured pass froze: the weights' flat buffers (prepare() re-creates them when parameters were replaced) and the set of
        # hoisted projections — if either changed since the capture, the graph is stale: capture again
        ver = (getattr(model, "_flat_version", None), len(getattr(model, "_kv_targets", None) or ()))
        if getattr(self, "_load_ver", ver) != ver:
            self._load_graph, self._loads = None, 2 if self._static is not None else 1
        self._load_ver = ver
        if not (self.use_graph and batch.query.is_cuda) or self._loads == 1:
            return self._load_body(batch)
        self._stage(batch)
        if self._load_graph is None:
            if self._loads == 2:
                return self._load_body(self._static)       # warm-up on the static inputs (and this dialogue's results)
            try:
                torch.cuda.synchronize()
                g = torch.cuda.CUDAGraph()
                with L.capturing(g):
                    self._load_body(self._static)
                self._load_graph = g
            except Exception as e:                          # never lose a decode to the faster path
                logging.getLogger("mtn_amd").warning("decode: capturing the encoder-side pass failed (%s); it stays eager", e)
                self._load_graph = False
                torch.cuda.synchronize()
                return self._load_body(self._static)
        if self._load_graph is False:
            return self._load_body(self._static)
        self._load_graph.replay()

    def _stage(self, b):
        """Copy a dialogue's inputs into the session's static Batch (created from the first one staged)."""
        tensors = lambda x: [x.query, x.query_mask, x.his, x.his_mask, x.cap, x.cap_mask] + list(x.fts or []) + list(x.fts_mask or [])
        if self._static is None:
            st = copy.copy(b)
            st.query, st.query_mask, st.his, st.his_mask, st.cap, st.cap_mask = (t.clone() for t in (b.query, b.query_mask, b.his, b.his_mask, b.cap, b.cap_mask))
            st.fts, st.fts_mask = [t.clone() for t in (b.fts or [])], [t.clone() for t in (b.fts_mask or [])]
            self._static = st
            return
        mine, theirs = tensors(self._static), tensors(b)
        # the captured pass is frozen to the first staged dialogue's shapes and dtypes: anything else must not be replayed into it
        if len(mine) != len(theirs) or any(d_.shape != s_.shape or d_.dtype != s_.dtype for d_, s_ in zip(mine, theirs)):
            raise ValueError("DecodeSession.load: this dialogue's tensors differ in shape / dtype from the session's (sessions are per shape: decode._session keys them)")
        for dst, src in zip(mine, theirs):
            dst.copy_(src)

    def _load_body(self, batch):
        model, width, b = self.model, self.width, batch
        self.D = D = b.query.size(0)
        lp = model.compute_dtype
        if b is self._static:                    # its masks' kernel images exist from the warm-up: refresh them (part of the captured pass)
            for mk in [b.query_mask, b.his_mask, b.cap_mask] + list(b.fts_mask):
                if getattr(mk, "_mtn_u8", None) is not None:
                    mk._mtn_u8.copy_(mk)
        with torch.no_grad():
            q, v, cp, hs, ae = model.encode(b.query, b.query_mask, b.his, b.his_mask, b.cap, b.cap_mask, b.fts, b.fts_mask)
            ops.prepare_masks(b.his_mask, b.cap_mask, b.query_mask, b.fts_mask)
            aes_per_layer = []
            for layer in model.decoder.layers:
                ae = layer.forward_ae_chains(cp, b.cap_mask, q, b.query_mask, v, b.fts_mask, ae, model.auto_encoder_ft)
                aes_per_layer.append(ae)

            def widen(t, into=None):                           # (D, m, d) -> (D*width, m, d), with its compute-dtype copy
                if into is None:
                    into = torch.empty(D * width, t.size(1), t.size(2), device=t.device, dtype=t.dtype)
                    into._mtn_lp = torch.empty_like(into, dtype=lp) if lp != torch.float32 else into
                into.view(D, width, t.size(1), t.size(2)).copy_(t.unsqueeze(1).expand(-1, width, -1, -1))
                if into._mtn_lp is not into:
                    into._mtn_lp.copy_(into)
                return into

            first = self.q is None
            self.q, self.cp, self.hs = widen(q, self.q), widen(cp, self.cp), widen(hs, self.hs)
            self.aes = [[widen(a, None if first else self.aes[k][i]) for i, a in enumerate(aes)] for k, aes in enumerate(aes_per_layer)]
            # K|V of the (widened) text memories for all layers: once per dialogue, not once per token; refreshed in place so
            # that a captured pass keeps reading the same buffers
            kvs = model.hoist_memory_kv(self.cp, self.hs, self.q, [], outs=None if first else self._kvs)
            if kvs is not None:
                self._kvs, self._kv_pairs = kvs, list(model._kv_targets)
                # ... and of the auto-encoder outputs the target stream attends un-projected (mtn.py:215): they do not change
                # with the prefix either, so their K|V leave the per-token pass as well (2 x N projections of Q rows per token)
                items, scs = [], []
                for k, layer in enumerate(model.decoder.layers):
                    for i, mem in enumerate(self.aes[k]):
                        f = layer.auto_encoder_attn[i].fused()
                        if f.get("w_qkv_lp") is None or mem._mtn_lp.dtype != lp:
                            continue
                        items.append((mem._mtn_lp, f["w_qkv_lp"], f["b_qkv"]))
                        scs.append(layer.sublayer[7 + 4 * i])
                if items:
                    self._ae_kvs = ops.project_memories(items, lp, None if first else getattr(self, "_ae_kvs", None))
                    self._kv_pairs += list(zip(scs, self._ae_kvs))
            model.clear_memory_kv()
            new_masks = (b.cap_mask, b.his_mask, b.query_mask)
            rep = lambda mk: mk.repeat_interleave(width, dim=0)
            if first:
                self.masks = tuple(rep(mk) for mk in new_masks)
                ops.prepare_masks(*self.masks)
            else:
                for mine, mk in zip(self.masks, new_masks):    # the captured pass reads the uint8 images
                    mine.copy_(rep(mk))
                    mine._mtn_u8.copy_(mine)

    def _head(self, rows):
        """What a pass leaves: its rows and, with in-pass selection, their heads."""
        self.logp = rows
        if self.select is not None:
            self.top = ops.topk_rows(self.logp, min(self.select[0], self.logp.size(1)), self.select[1])

    def _generate(self, x):
        """The generator on the rows of a pass: (rows, V) fp32 log-probabilities (mtn.py:68-69) — or, for a member of an Ensemble session,
        its logits: csrc/ensemble.hip normalises every member row itself."""
        return self.model.generator.logits(x) if getattr(self, "_logits", False) else self.model.generator(x).float()

    def _pass(self):
        self._head(self._target_rows())

    def _decoder_rows(self):
        """The full-prefix pass up to the decoder's final norm: (rows, max_len, d) activations of self.tokens under the causal mask."""
        m = self.model
        cap_mask, his_mask, q_mask = self.masks
        x = m.embed_target(self.tokens)
        m.attach_memory_kv(self._kv_pairs)
        try:
            for k, layer in enumerate(m.decoder.layers):
                x = layer.forward_target(x, self.cp, cap_mask, self.hs, his_mask, self.q, q_mask, self.trg_mask, self.aes[k],
                                         m.auto_encoder_ft)
        finally:
            m.clear_memory_kv()
        return m.decoder.norm(x)

    def _target_rows(self):
        last = self._decoder_rows().index_select(1, self.pos).squeeze(1)     # (width, d): the position being extended
        return self._generate(last)                                 # (width, V)

    def _pass_cached(self, cur: int):
        self._head(self._target_rows_cached(cur))

    def _target_rows_cached(self, cur: int):
        """One target position (self.pos) for every hypothesis, against the prefix cache: gather the cache rows of the parents
        (copy 1-cur -> cur), embed the newest token, per layer project its K|V into the cache and run the layer on that one row."""
        m = self.model
        cap_mask, his_mask, q_mask = self.masks
        src, dst = self._cache[1 - cur], self._cache[cur]
        torch.index_select(src, 1, self._parent, out=dst)
        tok = self.tokens.index_select(1, self.pos)                                  # (W, 1)
        emb, pos_enc = m.tgt_embed[0], m.tgt_embed[1]
        x = emb(tok) + pos_enc.pe[0].index_select(0, self.pos).unsqueeze(0)           # lut * sqrt(d) + PE[l]   (mtn.py:289, 308; eval: no dropout)
        ar = torch.arange(self.max_len, device=x.device)
        self._self_mask._mtn_u8.copy_((ar <= self.pos).view(1, 1, -1).expand_as(self._self_mask))
        m.attach_memory_kv(self._kv_pairs)
        try:
            for k, layer in enumerate(m.decoder.layers):
                kv_new = layer.self_kv_of_new_rows(x)                                # (W, 1, 2d)
                dst[k].index_copy_(1, self.pos, kv_new)
                x = layer.forward_target_cached(x, self.cp, cap_mask, self.hs, his_mask, self.q, q_mask, self.aes[k], m.auto_encoder_ft,
                                                dst[k].view(-1, dst.size(-1)), self._self_mem, self._self_mask)
        finally:
            m.clear_memory_kv()
        x = m.decoder.norm(x)
        return self._generate(x.squeeze(1))

    def _check_prefixes(self, prefix_lists):
        """The common length of a step's prefixes, checked against the session's shape."""
        if len(prefix_lists) != self.D:
            raise ValueError("one prefix list per dialogue of the session")
        l = len(prefix_lists[0][0])
        if max(len(p) for p in prefix_lists) > self.width or l > self.max_len:
            raise ValueError("more hypotheses / longer prefix than the session was built for")
        return l

    def _stage_prefixes(self, prefix_lists):
        """The checked prefixes of a step into self.tokens (dialogue d's from row d * width on, pad elsewhere) and their last position
        into self.pos; returns their length."""
        l = self._check_prefixes(prefix_lists)
        W = self.width
        host = torch.full((self.D * W, self.max_len), self.pad, dtype=torch.long)
        for d, prefixes in enumerate(prefix_lists):
            host[d * W:d * W + len(prefixes), :l] = torch.tensor(prefixes, dtype=torch.long)
        self.tokens.copy_(host, non_blocking=False)
        self.pos.fill_(l - 1)
        return l

    def _step_cached(self, prefix_lists):
        l = self._stage_prefixes(prefix_lists)
        W = self.width
        parent = torch.arange(self.D * W)
        if l > 1:
            for d, prefixes in enumerate(prefix_lists):
                prev = self._prev[d]
                # the hypothesis this one extends (same tokens but the last).  Two groups of a diverse search may hold the same prefix: the
                # lookup finds the first of them, whose cache rows hold the same values
                for i, p in enumerate(prefixes):
                    parent[d * W + i] = d * W + prev.index(list(p[:-1]))
        self._prev = [[list(p) for p in prefixes] for prefixes in prefix_lists]
        self._parent.copy_(parent)
        cur = self._cur
        with torch.no_grad():
            if not self.use_graph:
                self._pass_cached(cur)
            else:
                g = self._graphs.get(cur)
                if g is None:
                    g = _capture(lambda: self._pass_cached(cur))
                    g = self._graphs[cur] = (g, self.logp, self.top)          # each graph writes its own output buffers
                g[0].replay()
                self.logp, self.top = g[1], g[2]
        self._cur = 1 - cur
        return [self.logp[d * W:d * W + len(p)] for d, p in enumerate(prefix_lists)]

    def step(self, prefixes: Sequence[Sequence[int]]) -> torch.Tensor:
        """Log-probabilities (n, V) of the next token after each prefix of ONE dialogue (all prefixes have the same length)."""
        return self.step_many([prefixes])[0]

    def step_many(self, prefix_lists: Sequence[Sequence[Sequence[int]]]):
        """One decode step for all dialogues of the session: prefix_lists[d] = live prefixes of dialogue d (same length
        everywhere, at most `width` per dialogue) -> list of (n_d, V) log-probability tensors."""
        if self.kv_cache:
            return self._step_cached(prefix_lists)
        self._stage_prefixes(prefix_lists)
        with torch.no_grad():
            if not self.use_graph:
                self._pass()
            else:
                if self._graph is None:
                    self._graph = _capture(self._pass)
                self._graph.replay()
        return [self.logp[d * self.width:d * self.width + len(p)] for d, p in enumerate(prefix_lists)]

    def _pass_score(self):
        """_pass for scoring: the same target-stream pass, but the generator runs at EVERY position — logits only — and
        mtn_score_rows (csrc/score.hip) reads the targets' log-probabilities and ranks off them: no (rows, V) log-softmax."""
        ops.score_rows(self._score_logits(), self._score_target, self.pad, out=self._score_out)

    def _score_logits(self):
        z = self.model.generator.logits(self._decoder_rows())       # (D * width, max_len, V) fp32
        return z.view(-1, z.size(-1))

    def score(self, rows_tokens: Sequence[Sequence[int]], start: int, eos: int):
        """Teacher-forced scores of D * width token lists (row d * width + i belongs to dialogue d; no <sos> / <eos> in them, at most
        max_len - 1 tokens each): the pass reads [<sos>, c...] and is scored against [c..., <eos>], both padded to max_len.  One
        pass, captured as a graph of its own.  Returns (tok_logp (rows, max_len), tok_rank, seq_logp (rows,) float64, seq_len) as
        numpy arrays on the host (include/mtn_hip.h mtn_score_rows defines them)."""
        W, Lm = self.D * self.width, self.max_len
        if len(rows_tokens) != W or any(len(c) + 1 > Lm for c in rows_tokens):
            raise ValueError("one token list per row of the session, each at most max_len - 1 tokens")
        dev = self.tokens.device
        if getattr(self, "_score_out", None) is None:
            self._score_target = torch.full((W, Lm), self.pad, dtype=torch.long, device=dev)
            self._score_out = (torch.zeros(W, Lm, device=dev), torch.zeros(W, Lm, dtype=torch.int32, device=dev),
                               torch.zeros(W, dtype=torch.float64, device=dev), torch.zeros(W, dtype=torch.int32, device=dev))
            self._score_graph = None
        host = torch.full((2, W, Lm), self.pad, dtype=torch.long)
        for r, c in enumerate(rows_tokens):
            c = [int(t) for t in c]
            host[0, r, :len(c) + 1] = torch.tensor([start] + c, dtype=torch.long)
            host[1, r, :len(c) + 1] = torch.tensor(c + [eos], dtype=torch.long)
        self.tokens.copy_(host[0])
        self._score_target.copy_(host[1])
        with torch.no_grad():
            if not self.use_graph:
                self._pass_score()
            else:
                if self._score_graph is None:
                    self._score_graph = _capture(self._pass_score)
                self._score_graph.replay()
        return tuple(t.cpu().numpy() for t in self._score_out)

    def contrastive_log(self, start, k, alpha, eos, min_len, banned=(), trace=None):
        """A whole contrastive search (Su et al. 2022; include/mtn_hip.h mtn_contrastive_advance holds the definition) for every dialogue
        of the session, whose ``width`` = k rows are the dialogue's candidates.  The body of one token is the full-prefix pass up to the
        decoder's final norm — the (rows, max_len, d) states the degeneration penalty is taken from —, the generator on position ``pos``,
        the rows' heads (ops.topk_rows) and mtn_contrastive_advance (csrc/contrastive.hip), which scores the candidates, logs the choice
        and writes ``tokens`` / ``pos`` for the next pass in place.  The body is captured once per session and replayed max_len times
        (use_graph=False: run eagerly); no token is read on the host, the log is copied out once at the end.  The state is reset by device
        fills, so the session serves further searches after ``load``.
        Returns the numpy logs (tokens int32, log-probabilities fp32, penalties fp32, ranks int32), each (max_len, D); row 0 is the
        bootstrap and holds nothing.  ``trace`` (eager runs only): a list that receives, per step, a dict of host copies of what the kernel
        read — hidden, top, tokens, cand_logp, step, done."""
        k, banned = int(k), tuple(int(b) for b in banned)
        if self.kv_cache or isinstance(self.model, Ensemble) or isinstance(self, MegaDecodeSession):
            raise ValueError("contrastive_log: the search runs on the full-prefix launch-per-sublayer pass of one model")
        if k != self.width or not 1 <= k <= ops.CONTRASTIVE_MAX_K or len(banned) > 4:
            raise ValueError("contrastive_log: k is the session's width, 1..16; at most 4 banned tokens")
        if trace is not None and self.use_graph:
            raise ValueError("contrastive_log: the per-step trace needs an eager session (use_graph=False)")
        D, Lm, dev = self.D, self.max_len, self.tokens.device
        k_top = min(SELECT_MAX_K, k + len(banned) + 1)
        key = (k, float(alpha), int(eos), int(min_len), banned)
        if self._cs_key != key:               # (first search, or other settings: kernel arguments are frozen into the captured body)
            # [cand_logp (rows) | step (D) | done (D) | the four logs (4 x L x D)]: one block of 32-bit words, one fill per search
            W = D * k
            self._cs_state = torch.zeros(W + 2 * D + 4 * Lm * D, device=dev, dtype=torch.int32)
            o = W + 2 * D
            logs = self._cs_state[o:].view(4, Lm, D)
            self._cs_views = (self._cs_state[:W].view(torch.float32), self._cs_state[W:W + D], self._cs_state[W + D:o],
                              (logs[0], logs[1].view(torch.float32), logs[2].view(torch.float32), logs[3]))
            self._cs_graph, self._cs_key = None, key
        cand, step, done, log = self._cs_views
        kw = dict(k=k, alpha=float(alpha), eos=int(eos), min_len=int(min_len), banned=banned)

        def body():
            hidden = self._decoder_rows()
            if hidden.dtype != torch.float32:
                hidden = hidden.float()
            top = ops.topk_rows(self._generate(hidden.index_select(1, self.pos).squeeze(1)), k_top, -1)
            if trace is not None:
                snap = lambda t: t.detach().cpu().numpy().copy()
                trace.append(dict(hidden=snap(hidden), top=snap(top), tokens=snap(self.tokens), cand_logp=snap(cand), step=snap(step), done=snap(done)))
            ops.contrastive_advance(hidden, top, self.tokens, self.pos, cand, step, done, log, **kw)

        with torch.no_grad():
            if self.use_graph and self._cs_graph is None:
                self._cs_graph = _capture(body)          # (runs the body twice on whatever the state holds: the reset comes after it)
            self.tokens.fill_(self.pad)
            self.tokens[:, 0].fill_(int(start))
            self.pos.zero_()
            self._cs_state.zero_()
            for _ in range(Lm):
                if self.use_graph:
                    self._cs_graph.replay()
                else:
                    body()
        host = self._cs_state[D * k + 2 * D:].view(4, Lm, D).cpu().numpy()         # the one synchronisation of the search
        return host[0].copy(), host[1].view(np.float32).copy(), host[2].view(np.float32).copy(), host[3].copy()


class MegaDecodeSession(DecodeSession):
    """The per-token pass as ONE persistent launch (csrc/decode.hip, include/mtn_hip.h mtn_decode_step) + the generator's three small
    launches, for sessions of at most 16 live hypotheses on a bf16 model (8 at d_ff = 4096): the newest position of every hypothesis walks a
    device-resident stage list (per layer: self-attention over its prefix cache, the cross-attentions over the K|V hoisted by load(),
    the feed-forward) with grid barriers instead of ~90 dependent launches.  The prefix cache is never copied when a beam step
    re-orders hypotheses: position t of hypothesis j's prefix is read from cache slot anc[j][t], a (W, L) int table the host updates
    from the parents (the slot of row j at position l-1 is j itself).  Same search results as the launch-per-sublayer pass (tested).

    The launch needs ALL its workgroups resident at once (they poll each other).  `supported()` refuses devices with fewer compute units than
    the launch has workgroups; if a poll still times out (another kernel held compute units), `timed_out()` reports it, `recover()` makes the
    session's device state consistent again, and the callers below re-run the search on the launch-per-sublayer pass (FALLBACKS counts them)."""

    MAX_W = 16
    FALLBACKS = 0          # searches re-run on the launch-per-sublayer pass after a poll timeout of the persistent step

    @staticmethod
    def supported(model, batch, max_len, width) -> bool:
        if os.environ.get("MTN_DECODE_MEGA", "1") == "0" or not batch.query.is_cuda:
            return False
        if isinstance(model, Ensemble):                             # every member runs its own persistent step: all of them or none
            return all(MegaDecodeSession.supported(m, batch, max_len, width) for m in model.active)
        try:
            layer = model.decoder.layers[0]
            d, h = layer.size, layer.self_attn.h
            dff = layer.feed_forward.w_1.weight.size(0)
        except AttributeError:
            return False
        W = batch.query.size(0) * width
        if model.compute_dtype != torch.bfloat16 or W > MegaDecodeSession.MAX_W or W * d > 8192 or d not in (128, 256, 512, 1024) or d % h or d // h not in (32, 64):
            return False
        if dff > 4096 or dff < d or dff % 32 or max_len > 1024 or model.auto_encoder_ft not in ("query", "caption", "summary"):
            return False
        if W * (2 * max(d, dff) + 16) > 66048:                      # csrc/decode.hip DEC_ACT_BYTES: the activation image of the widest Linear
            return False
        if max([batch.his.size(1), batch.cap.size(1), batch.query.size(1)] + [f.size(1) for f in (batch.fts or [])]) > 1024:
            return False
        # every workgroup of the launch must be resident at once, one per compute unit: W x h attention units + d / 16 writers of the
        # residual stream + enough "wide" workgroups that a slice of the q|k|v / first FFN projection is at most 64 features
        grid = MegaDecodeSession.grid_for(batch.query.device)
        n_mid = min(128, grid - W * h - d // 16)
        if W * h > 128 or n_mid < 16 or (-(-max(3 * d, dff) // n_mid) + 3) // 4 * 4 > 64:
            return False
        n_stages = 2 + sum(3 + 2 * (3 + len(l.auto_encoder_attn)) + 2 for l in model.decoder.layers)       # csrc/decode.hip DEC_MAX_STAGES
        return n_stages <= 160 and all(len(l.sublayer) == 5 + 4 * len(l.auto_encoder_attn) for l in model.decoder.layers)

    @staticmethod
    def grid_for(device) -> int:
        """The most workgroups the persistent launch may use on this device: one per compute unit, at most 256."""
        return min(256, int(torch.cuda.get_device_properties(device).multi_processor_count))

    def __init__(self, model, batch, max_len, width, pad=1, use_graph=True, select=None, share=None):
        super().__init__(model, batch, max_len, width, pad=pad, use_graph=use_graph, kv_cache=False, select=select, share=share)
        dev = batch.query.device
        layers = model.decoder.layers
        d, h = layers[0].size, layers[0].self_attn.h
        dff = layers[0].feed_forward.w_1.weight.size(0)
        W, Lm, nl = self.D * width, max_len, len(layers)
        lp = torch.bfloat16
        self._W = W
        self._mcache = torch.zeros(nl, W, Lm, 2 * d, device=dev, dtype=lp)
        # granule buffers (8 bytes {data, tag}): residual stream, q|k|v of the newest row, attention output, FFN hidden — zeroed once
        self._x = torch.zeros(W, d, device=dev, dtype=torch.int64)
        self._q = torch.zeros(W, 3 * d // 2, device=dev, dtype=torch.int64)
        self._o = torch.zeros(W, d // 2, device=dev, dtype=torch.int64)
        self._hid = torch.zeros(W, dff // 2, device=dev, dtype=torch.int64)
        self._out_lp = torch.zeros(W, d, device=dev, dtype=lp)
        self._sync = torch.zeros(4, device=dev, dtype=torch.int32)
        # what the host changes every step, in ONE pinned block -> ONE copy: [W newest tokens (int64) | position (int32, padded) | anc (W x L int32)]
        self._off_pos, self._off_anc = 8 * W, 8 * W + 8
        nbytes = self._off_anc + 4 * W * Lm
        if share is None:
            self._host = torch.zeros(nbytes, dtype=torch.uint8).pin_memory()
            self._devblk = torch.zeros(nbytes, device=dev, dtype=torch.uint8)
        else:                               # (same W and max_len: the same layout) this launch reads the block the sharer's bookkeeping writes
            self._host, self._devblk = share._host, share._devblk
        hb = self._host.numpy()                       # numpy views of the pinned block: the per-step bookkeeping below is plain numpy slicing
        self._h_tok = hb[:8 * W].view(np.int64)
        self._h_pos = hb[self._off_pos:self._off_pos + 8].view(np.int32)
        self._h_anc = hb[self._off_anc:].view(np.int32).reshape(W, Lm)
        self._h_anc[:] = np.arange(W, dtype=np.int32)[:, None]
        self._prev = None
        self._top_host = None
        self._grid = self.grid_for(dev)     # the most the launch may use (one workgroup per CU); the library deals them to its three classes
        self._build_stages(L, d, h, dff)
        emb, pe = model.tgt_embed[0], model.tgt_embed[1]
        a = L.DecodeArgs()
        a.W, a.d, a.h, a.L, a.n_stages, a.d_ff, a.max_m = W, d, h, Lm, self._n_stages, dff, self._max_m
        self._dbg = torch.zeros(4 * self._n_stages, device=dev, dtype=torch.int64) if os.environ.get("MTN_DECODE_TIMELINE") == "1" else None
        a.dbg = self._dbg.data_ptr() if self._dbg is not None else None
        a.xg, a.qg, a.og, a.hg, a.out_lp = self._x.data_ptr(), self._q.data_ptr(), self._o.data_ptr(), self._hid.data_ptr(), self._out_lp.data_ptr()
        a.tokens = self._devblk.data_ptr()
        a.lut, a.emb_scale, a.pe = emb.lut.weight.data_ptr(), float(d) ** 0.5, pe.pe.data_ptr()
        a.pos, a.anc, a.sync = self._devblk.data_ptr() + self._off_pos, self._devblk.data_ptr() + self._off_anc, self._sync.data_ptr()
        self._args = a
        if pe.pe.size(1) < Lm or not emb.lut.weight.is_contiguous():
            raise ValueError("positional-encoding table shorter than max_len")

    def _build_stages(self, L, d, h, dff):
        """The stage list of one decode step (include/mtn_hip.h MTN_DEC_*): per decoder layer the schedule of mtn.py:183-218 for the
        target stream — self-attention, history, caption | query (order by auto_encoder_ft), one attention per auto-encoder stream,
        feed-forward — every attention followed by its output projection; pointers into the model's flat buffers and this session's
        hoisted K|V / masks (all refreshed IN PLACE by load(), so the table is built once)."""
        m = self.model
        cap_mask, his_mask, q_mask = self.masks
        kvmap = {id(sc): kv for sc, kv in self._kv_pairs}
        st = []
        self._max_m = 1

        def stage(kind, **kw):
            s_ = L.DecodeStage()
            s_.kind = kind
            for k, v in kw.items():
                setattr(s_, k, v)
            st.append(s_)

        def ln(sc):
            return dict(ln_a=sc.norm.a_2.data_ptr(), ln_b=sc.norm.b_2.data_ptr(), ln_eps=float(sc.norm.eps))

        stage(L.DEC_EMBED)
        for k, layer in enumerate(m.decoder.layers):
            sl, nF = layer.sublayer, len(layer.auto_encoder_attn)
            f = layer.self_attn.fused()
            cache = self._mcache[k].data_ptr()
            stage(L.DEC_SELF_QKV, N=3 * d, K=d, w=f["w_qkv_lp"].data_ptr(), bias=f["b_qkv"].data_ptr(), cache=cache, **ln(sl[0]))
            stage(L.DEC_SELF_ATT, cache=cache)
            stage(L.DEC_OUT, N=d, K=d, w=f["w_o_lp"].data_ptr(), bias=f["b_o"].data_ptr())
            text, _, _, ae_mask = layer._plan(self.cp, cap_mask, self.hs, his_mask, self.q, q_mask, None, [None] * nF, [None] * nF, m.auto_encoder_ft)
            cross = list(text[1:]) + [(sl[7 + 4 * i], layer.auto_encoder_attn[i], self.aes[k][i], ae_mask) for i in range(nF)]
            for sc, mod, mem, mask in cross:
                f = mod.fused()
                kv = kvmap.get(id(sc))
                if kv is None or kv.dtype != torch.bfloat16:
                    raise ValueError("a memory's K|V were not hoisted")
                mk = getattr(mask, "_mtn_u8", None)
                self._max_m = max(self._max_m, int(mem.size(1)))
                stage(L.DEC_CROSS, N=d, K=d, w=f["w_qkv_lp"].data_ptr(), bias=f["b_qkv"].data_ptr(), kv=kv.data_ptr(), m=mem.size(1),
                      mask=mk.data_ptr() if mk is not None else None, mask_stride=mem.size(1), **ln(sc))
                stage(L.DEC_OUT, N=d, K=d, w=f["w_o_lp"].data_ptr(), bias=f["b_o"].data_ptr())
            ff = layer.feed_forward.fused()
            stage(L.DEC_FFN1, N=dff, K=d, w=ff["w1_lp"].data_ptr(), bias=ff["b1"].data_ptr(), **ln(sl[4 + 4 * nF]))
            stage(L.DEC_FFN2, N=d, K=dff, w=ff["w2_lp"].data_ptr(), bias=ff["b2"].data_ptr())
        nrm = m.decoder.norm
        stage(L.DEC_FINAL, ln_a=nrm.a_2.data_ptr(), ln_b=nrm.b_2.data_ptr(), ln_eps=float(nrm.eps))
        arr = (L.DecodeStage * len(st))(*st)
        self._n_stages = len(st)
        self._stages_dev = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(self._x.device)

    def _pass_mega(self):
        # the step's host inputs and (with device-side selection) its host outputs travel INSIDE the pass — copy nodes of the captured graph —
        # so a generated token costs the host one replay and one stream synchronisation
        self._devblk.copy_(self._host, non_blocking=True)
        self._head(self._step_rows())                                                    # (W, V) fp32 log-probabilities (mtn.py:68-69)
        if self.select is not None:
            if self._top_host is None:
                self._top_host = torch.empty(self.top.shape, dtype=self.top.dtype).pin_memory()
            self._top_host.copy_(self.top, non_blocking=True)

    def _step_rows(self, logits=False):
        """One persistent decode step on the shared [tokens | pos | anc] block and the generator on its output rows: (W, V) fp32
        log-probabilities, or the logits (a member of an Ensemble session: csrc/ensemble.hip normalises them)."""
        L.check(L.load().mtn_decode_step(C.byref(self._args), self._stages_dev.data_ptr(), self._grid, L.stream_ptr()))
        g = self.model.generator._fused
        return (ops.generator_logits if logits else ops.generator_log_probs)(self._out_lp, g["w_lp"], g["bias"])

    def top_host(self):
        """The rows' heads of the last step on the host (a pinned block the pass itself filled)."""
        torch.cuda.current_stream().synchronize()
        return self._top_host.numpy()

    def search(self, beam, k, start, unk, eos, penalty, min_len, nbest, no_repeat_ngram=0, repetition_penalty=1.0, beam_groups=1,
               diversity_penalty=0.0):
        G = int(beam_groups)
        log = self._search_log(beam, k, start, unk, eos, penalty, min_len, eos, no_repeat_ngram, repetition_penalty, G, float(diversity_penalty))
        if log is None:
            return None
        par, tok, n_old, n_new, score, done_sc, flags = log

        def finished(base, p):
            """Per step, the hypotheses of the log's pseudo-dialogue p (its rows start at ``base``) that finished there, with their scores."""
            outs = [[]]
            for l in range(self.max_len):
                yield [(outs[h], float(done_sc[l, base + h])) for h in range(int(n_old[l, p]))] if l >= min_len else []
                outs = [outs[int(par[l, base + i])] + [int(tok[l, base + i])] for i in range(int(n_new[l, p]))]

        # diverse beam search: the log holds D x G pseudo-dialogues of width beam / G (group g of dialogue d owns rows d * width + g * Bp ..);
        # a dialogue's finished hypotheses are pooled in the order the stepped path appends them: step, group, hypothesis.  One group: the
        # dialogue itself, its finished hypotheses in step order, and the plain search's result (_Beam.result)
        Bp = self.width // G
        results = []
        for d_ in range(self.D):
            groups = [finished(d_ * self.width + g * Bp, d_ * G + g) for g in range(G)]
            done = [h for step in zip(*groups) for group in step for h in group]
            if G > 1:
                results.append(_pool_groups(done, nbest))
            elif done:
                results.append((sorted(done, key=lambda h: -h[1])[:nbest], max(h[1] for h in done)))
            else:
                results.append(([([], 0)], None))
        return results

    def greedy(self, start, no_repeat_ngram=0, repetition_penalty=1.0):
        """argmax decoding of every dialogue of the session as one graph replay: a beam of one per dialogue that skips nothing and
        finishes nothing (mtn_beam_advance with beam = k = 1, no <unk> / <eos>; dialogue d's tokens are column d * width of the step
        log).  Returns D lists of the max_len - 1 generated tokens, or None (tie / not applicable)."""
        log = self._search_log(1, 1, start, -1, -1, 0.0, self.max_len + 1, self.select[1] if self.select is not None else 0,
                               no_repeat_ngram, repetition_penalty)
        if log is None:
            return None
        return [[int(t) for t in log[1][:self.max_len - 1, d_ * self.width]] for d_ in range(self.D)]

    def _block_image(self, start, stride):
        """The pinned [tokens | pos | anc] block of a captured search before its first step: ``start`` in every ``stride``-th row and pad in
        the others, position 0, every row its own cache slots (identity ancestors)."""
        W = self._W
        blk = np.zeros(self._host.numel(), dtype=np.uint8)
        tok = blk[:8 * W].view(np.int64)
        tok[:] = self.pad
        tok[::stride] = start
        blk[self._off_anc:].view(np.int32).reshape(W, self.max_len)[:] = np.arange(W, dtype=np.int32)[:, None]
        return torch.from_numpy(blk).pin_memory()

    def _search_log(self, beam, k, start, unk, eos, penalty, min_len, extra_col, no_repeat_ngram=0, repetition_penalty=1.0, groups=1, diversity=0.0):
        """A whole beam search (data_utils.py:188-242) for every dialogue of the session as ONE graph replay: max_len x [persistent decode
        step, generator, row heads (csrc/select.hip topk_rows), hypothesis bookkeeping on the device (mtn_beam_advance)], the step log
        copied to a pinned block at the end.  The host synchronises once per search and rebuilds the n-best lists from the log.
        With a constraint on (no_repeat_ngram > 0 or repetition_penalty != 1; csrc/constrain.hip), one more launch per token sits between
        the generator and the row heads: it rewrites the rows in place from each hypothesis' history, which it walks out of this very step
        log (the parents and tokens of the steps before, the dialogue's step counter) — all device memory, so one graph serves every search.
        With ``groups`` = G > 1 (diverse beam search, csrc/diverse.hip) the bookkeeping launch is mtn_diverse_advance, one for one: the state
        and the log are those of D x G pseudo-dialogues of width beam / G — every group starts from <sos> in its own first row — and the row
        heads are the plain search's (beam + 2 entries and the tie sentinel: include/mtn_hip.h says why they suffice).  (G, lambda) are part
        of the search key; with one group nothing here differs from the plain search.
        Returns None when a row's head held an exact tie (the reference's visiting order then comes from the full row: the caller runs the
        search step by step) or when the device-side selection does not apply."""
        k_top = k + 1
        if self.select is None or self.select[0] != k_top or self.select[1] != extra_col or beam > self.width or k_top > SELECT_MAX_K or not self.use_graph:
            return None
        G = int(groups)
        if G > 1 and (beam != self.width or beam % G):
            return None
        # the bookkeeping's dialogues: D, or D x G groups of Wd = width / G rows each
        W, D, Lm, Wd = self._W, self.D * G, self.max_len, self.width // G
        ngram, theta = int(no_repeat_ngram), float(repetition_penalty)
        constrained = ngram > 0 or theta != 1.0
        key = (beam, k, start, unk, eos, float(penalty), min_len, ngram, theta)
        if G > 1:
            key += (G, float(diversity))
        if getattr(self, "_search_key", None) != key:
            dev = self._x.device
            # device state of the search [lp (W doubles) | n_live (D) | step (D) | flags (2)] and its initial image
            nst = 8 * W + 4 * (2 * D + 2)
            self._bstate = torch.zeros(nst, device=dev, dtype=torch.uint8)
            init = np.zeros(nst, dtype=np.uint8)
            init[8 * W:8 * W + 4 * D].view(np.int32)[:] = 1
            self._bstate_init = torch.from_numpy(init).pin_memory()
            self._blk_init = self._block_image(start, Wd)                    # <sos> in every dialogue's row 0
            # the step log: [parent | tok (int32 L x W each) | n_old | n_new (int32 L x D each) | score | done (double L x W each) | flags (2 x int32)]
            o_par, o_tok = 0, 4 * Lm * W
            o_nold, o_nnew = 8 * Lm * W, 8 * Lm * W + 4 * Lm * D
            o_sc = (8 * Lm * W + 8 * Lm * D + 7) // 8 * 8
            o_done = o_sc + 8 * Lm * W
            o_flags = o_done + 8 * Lm * W
            self._log = torch.zeros(o_flags + 8, device=dev, dtype=torch.uint8)
            self._log_host = torch.zeros(o_flags + 8, dtype=torch.uint8).pin_memory()
            hb = self._log_host.numpy()
            self._log_views = (hb[o_par:o_tok].view(np.int32).reshape(Lm, W), hb[o_tok:o_nold].view(np.int32).reshape(Lm, W),
                               hb[o_nold:o_nnew].view(np.int32).reshape(Lm, D), hb[o_nnew:o_nnew + 4 * Lm * D].view(np.int32).reshape(Lm, D),
                               hb[o_sc:o_done].view(np.float64).reshape(Lm, W), hb[o_done:o_flags].view(np.float64).reshape(Lm, W),
                               hb[o_flags:o_flags + 8].view(np.int32))
            da = L.DiverseArgs()                     # (one group: the plain arguments alone, and mtn_beam_advance)
            a = da.beam if G > 1 else L.BeamArgs()
            da.groups, da.diversity = G, float(diversity)
            a.dialogues, a.width, a.L, a.k_top, a.k, a.beam, a.unk, a.eos, a.pad, a.min_len = D, Wd, Lm, k_top, k, beam, unk, eos, self.pad, min_len
            if G > 1:
                a.beam, a.k = Wd, Wd + 2             # a group places at most Wd candidates per row and skips at most two
            a.penalty = float(penalty)
            p0, s0, l0 = self._devblk.data_ptr(), self._bstate.data_ptr(), self._log.data_ptr()
            a.tokens, a.pos, a.anc = p0, p0 + self._off_pos, p0 + self._off_anc
            a.lp, a.n_live, a.step, a.flags = s0, s0 + 8 * W, s0 + 8 * W + 4 * D, l0 + o_flags
            a.log_parent, a.log_tok, a.log_n_old, a.log_n_new, a.log_score, a.log_done = l0 + o_par, l0 + o_tok, l0 + o_nold, l0 + o_nnew, l0 + o_sc, l0 + o_done
            self._beam_args = a

            def body():
                self._devblk.copy_(self._blk_init, non_blocking=True)
                self._bstate.copy_(self._bstate_init, non_blocking=True)
                self._log[o_flags:].zero_()
                for _ in range(Lm):
                    logp = self._step_rows()
                    if constrained:
                        ops.constrain_rows(logp, ngram, theta, log_tok=a.log_tok, log_parent=a.log_parent, step=a.step, width=Wd,
                                           rows_per_step=Wd, log_len=Lm)
                    top = ops.topk_rows(logp, k_top, extra_col)
                    a.top = top.data_ptr()
                    if G > 1:
                        L.check(L.load().mtn_diverse_advance(C.byref(da), L.stream_ptr()))
                    else:
                        L.check(L.load().mtn_beam_advance(C.byref(a), L.stream_ptr()))
                self._log_host.copy_(self._log, non_blocking=True)

            with torch.no_grad():
                self._search_graph = _capture(body)
            self._search_key = key
        self._search_graph.replay()
        self._prev = None
        torch.cuda.current_stream().synchronize()
        if self.timed_out():                 # the log is garbage: the caller sees timed_out() and falls back
            return None
        return None if self._log_views[6][0] else self._log_views

    def sample_log(self, start, seed, keys, params, no_repeat_ngram=0, repetition_penalty=1.0, mbr=0):
        """A whole sampling search for every row of the session as ONE graph replay: max_len x [persistent decode step, generator,
        mtn_sample_rows (csrc/sample.hip)] — no row heads, no hypothesis bookkeeping: every row starts at <sos>, draws its next token on the
        device and keeps its own cache slots (identity ancestors).  seed and keys enter through one small pinned block (kernel arguments are
        frozen into the graph, and one graph serves every search of the session's shape); the step log [token | logp[token] | u], each
        (max_len, rows), is copied out at the end and the host synchronises once.  ``params``: the keyword arguments of ops.sample_args.
        With a constraint on, one csrc/constrain.hip launch per token rewrites the rows before the draw; a row's history is its own column of
        the token log (no parents).
        ``mbr`` = N > 0: minimum-Bayes-risk selection of order N (csrc/mbr.hip) is the LAST node of the graph — dialogue d's ``width`` rows
        are set d, read from the token log in device memory; its outputs are copied out next to the log, and the host still synchronises once.
        Returns the three host views (with mbr two more: expected utilities (D, width) and order (D, width)), or None after a poll timeout
        (timed_out() tells)."""
        if not self.use_graph:
            raise ValueError("the sampling search on the persistent step is a captured graph")
        W, Lm = self._W, self.max_len
        ngram, theta = int(no_repeat_ngram), float(repetition_penalty)
        constrained = ngram > 0 or theta != 1.0
        mbr = int(mbr)
        key = (start,) + tuple(sorted((k, tuple(v) if isinstance(v, (list, tuple)) else v) for k, v in params.items())) + (ngram, theta, mbr)
        if getattr(self, "_sample_key", None) != key:
            dev = self._x.device
            # [seed (int64) | keys (W int64) | step (W int32)]: the pinned image the host fills per search, and its device copy
            nst = 8 + 8 * W + 4 * W
            self._sstate = torch.zeros(nst, device=dev, dtype=torch.uint8)
            self._sstate_host = torch.zeros(nst, dtype=torch.uint8).pin_memory()
            hs = self._sstate_host.numpy()
            self._h_seed, self._h_keys = hs[:8].view(np.int64), hs[8:8 + 8 * W].view(np.int64)
            self._sblk_init = self._block_image(start, 1)                    # <sos> in every row
            self._slog = torch.zeros(3, Lm, W, device=dev, dtype=torch.int32)   # (the two float logs are viewed as such)
            self._slog_host = torch.zeros(3, Lm, W, dtype=torch.int32).pin_memory()
            hl = self._slog_host.numpy()
            self._slog_views = (hl[0], hl[1].view(np.float32), hl[2].view(np.float32))
            if mbr:
                # [expected (W float64) | order (W int32) | best (D int32)]: the selection's outputs in one block -> one copy
                D = self.D
                self._smbr = torch.zeros(12 * W + 4 * D, device=dev, dtype=torch.uint8)
                self._smbr_host = torch.zeros(12 * W + 4 * D, dtype=torch.uint8).pin_memory()
                hm = self._smbr_host.numpy()
                self._smbr_views = (hm[:8 * W].view(np.float64).reshape(D, W // D), hm[8 * W:12 * W].view(np.int32).reshape(D, W // D))
                mbr_out = (self._smbr[:8 * W].view(torch.float64), self._smbr[12 * W:].view(torch.int32), self._smbr[8 * W:12 * W].view(torch.int32))
            s0, p0 = self._sstate, self._devblk.data_ptr()
            log = (self._slog[0], self._slog[1].view(torch.float32), self._slog[2].view(torch.float32))

            def body():
                self._devblk.copy_(self._sblk_init, non_blocking=True)
                self._sstate.copy_(self._sstate_host, non_blocking=True)
                for _ in range(Lm):
                    logp = self._step_rows()
                    if constrained:
                        ops.constrain_rows(logp, ngram, theta, log_tok=self._slog[0], step=s0[8 + 8 * W:].view(torch.int32), width=1, rows_per_step=1)
                    ops.sample_rows(logp, s0[:8].view(torch.int64), s0[8:8 + 8 * W].view(torch.int64), s0[8 + 8 * W:].view(torch.int32), log,
                                    tokens=p0, pos=p0 + self._off_pos, anc=p0 + self._off_anc, **params)
                if mbr:
                    ops.mbr_select(mbr, log_tok=self._slog[0], sets=self.D, eos=params["eos"], out=mbr_out)
                    self._smbr_host.copy_(self._smbr, non_blocking=True)
                self._slog_host.copy_(self._slog, non_blocking=True)

            self._h_seed[0], self._h_keys[:] = 0, 0
            with torch.no_grad():
                self._sample_graph = _capture(body)
            self._sample_key = key
        self._h_seed[0] = seed
        self._h_keys[:] = keys
        self._sample_graph.replay()
        self._prev = None
        torch.cuda.current_stream().synchronize()
        if self.timed_out():                 # the log is garbage: the caller sees timed_out() and falls back
            return None
        return self._slog_views + self._smbr_views if mbr else self._slog_views

    def timed_out(self) -> bool:
        """True if a poll of any step since the session was built (or last recovered) timed out: the results since then are garbage."""
        return int(self._sync[1].item()) != 0

    def recover(self):
        """After a timeout: nothing advanced the launch generation and the granule buffers hold tags of the failed step.  Advance the
        generation past it, clear the timeout flag and the check-in counter — the next launch starts clean."""
        torch.cuda.synchronize()
        gen = int(self._sync[0].item())
        self._sync.copy_(torch.tensor([gen + 1, 0, 0, 0], dtype=torch.int32))
        self._prev = None
        torch.cuda.synchronize()

    def check(self):
        """Raises if a poll of any step since the session was built timed out (for callers that drive step() / step_extend() themselves;
        beam_search_decode / greedy_decode fall back to the launch-per-sublayer pass instead)."""
        if self.timed_out():
            raise RuntimeError("mtn_decode_step: a poll timed out (not every workgroup of the launch was resident?)")

    def step_extend(self, l: int, slots, tokens, parents):
        """One step given the live hypotheses directly: hypothesis in row ``slots[i]`` ends in ``tokens[i]`` (its l-th token) and extends
        the hypothesis that sat in row ``parents[i]`` at the previous step (ignored at l = 1).  What step_many() derives from prefix
        lists, without building or searching them: the beam search below knows every candidate's parent."""
        if l > 1:
            self._h_anc[slots, :l - 1] = self._h_anc[parents, :l - 1]          # (the right-hand side is gathered into a copy first)
        self._h_anc[slots, l - 1] = slots
        self._h_tok[:] = self.pad
        self._h_tok[slots] = tokens
        self._h_pos[0] = l - 1
        self._prev = None
        self._run()

    def _run(self):
        with torch.no_grad():
            if not self.use_graph:
                self._pass_mega()
            else:
                if self._graph is None:
                    self._graph = _capture(self._pass_mega)
                self._graph.replay()

    def step_many(self, prefix_lists):
        l = self._check_prefixes(prefix_lists)
        W = self.width
        anc_old = self._h_anc.copy() if l > 1 else None
        self._h_tok[:] = self.pad
        for d_, prefixes in enumerate(prefix_lists):
            for i, p in enumerate(prefixes):
                j = d_ * W + i
                self._h_tok[j] = int(p[-1])
                if l > 1:
                    parent = d_ * W + self._prev[d_].index(list(p[:-1]))          # the hypothesis this one extends
                    self._h_anc[j, :l - 1] = anc_old[parent, :l - 1]
                self._h_anc[j, l - 1] = j
        self._prev = [[list(p) for p in prefixes] for prefixes in prefix_lists]
        self._h_pos[0] = l - 1
        self._run()
        return [self.logp[d_ * W:d_ * W + len(p)] for d_, p in enumerate(prefix_lists)]


class Ensemble:
    """Several checkpoints decoded as one model: pass it wherever the functions below take a model.  Per generated token every member
    runs its own target-stream pass on its own session (own encoder side, hoisted K|V and prefix cache), and the members' generator
    logits become ONE row of log-probabilities per hypothesis in one launch (csrc/ensemble.hip; include/mtn_hip.h mtn_ensemble_rows):
    ``mode`` "prob", log sum_m w_m p_m, or "logprob", sum_m w_m log p_m renormalised.  Constraints, selection, sampling and scoring read
    those rows as they read a single model's.  Members may differ in depth, width, auto_encoder_ft and compute dtype; they share the
    vocabulary size and the batch.  ``weights``: one number >= 0 per member (normalised to sum 1; None: uniform) — a member at weight 0
    is not run at all.  ValueError: no member, more than 8, the same model object twice, different vocabulary sizes, bad weights / mode."""

    def __init__(self, models, weights=None, mode="prob"):
        self.models = list(models)
        if not 1 <= len(self.models) <= ops.ENSEMBLE_MAX:
            raise ValueError(f"Ensemble: 1 to {ops.ENSEMBLE_MAX} members")
        if len({id(m) for m in self.models}) != len(self.models):
            raise ValueError("Ensemble: the same model object twice (decode sessions are per model object: pass a copy)")
        if mode not in ops.ENSEMBLE_MODES:
            raise ValueError("Ensemble: mode is 'prob' or 'logprob'")
        self.mode = mode
        self.weights = tuple(float(w) for w in ops.ensemble_weights(len(self.models), weights))
        vocab = {int(m.generator.proj.weight.size(0)) for m in self.models}
        if len(vocab) != 1:
            raise ValueError(f"Ensemble: the members' vocabulary sizes differ ({sorted(vocab)})")
        self.vocab = vocab.pop()
        self.active = [m for m, w in zip(self.models, self.weights) if w > 0]               # the members that are run ...
        self.active_weights = [w for w in self.weights if w > 0]                            # ... and their weights (sum 1)

    def prepare(self):
        for m in self.active:
            m.prepare()

    @property
    def _flat_version(self):
        """Changes when any member's weights were replaced: a cached session of this ensemble is then stale."""
        return tuple(getattr(m, "_flat_version", None) for m in self.active)

    def signature(self):
        return (tuple((id(m), m._flat.data_ptr() if m._flat is not None else 0, m.compute_dtype) for m in self.models), self.weights, self.mode)

    def same_members(self, other) -> bool:
        return isinstance(other, Ensemble) and len(other.models) == len(self.models) and all(a is b for a, b in zip(self.models, other.models))

    def combine(self, rows):
        """The active members' (rows, V) logits -> (rows, V) log-probabilities of the ensemble, one launch."""
        return ops.ensemble_rows(rows, self.active_weights, self.mode)


class _OwnsMembers:
    """What the two Ensemble sessions share: they skip their base class' constructor (there is no single model to load) and own one session
    per active member instead.  Member 0 allocates the per-step inputs and every other member is built with ``share=`` member 0, so all of
    them read ONE set; the attributes of that shared state the base class' methods read (SHARED: the pinned block and its views, offsets, row
    count, grid, the cache's parent row) are looked up on member 0 — nothing is copied; every other missing attribute raises as usual.  What a
    session computes or captures (logp, top, graphs, search keys and logs) is set by those methods on this object itself."""

    def _own(self, cls, ens, batch, max_len, width, pad, use_graph, select, **kw):
        self.model, self.width, self.max_len, self.pad = ens, width, max_len, pad
        self.select = select if (select is not None and batch.query.is_cuda) else None
        self.use_graph = use_graph and batch.query.is_cuda
        self.top = self.logp = self._graph = self._prev = self._top_host = None
        self.members = []
        for m in ens.active:
            self.members.append(cls(m, batch, max_len, width, pad=pad, use_graph=use_graph, share=self.members[0] if self.members else None, **kw))
        self.D = self.members[0].D

    # the shared per-step state, by name: anything else a session lacks (a member's own outputs, arguments, flags; a typo) raises
    SHARED = frozenset(("tokens", "pos", "_parent", "_host", "_devblk", "_h_tok", "_h_pos", "_h_anc", "_off_pos", "_off_anc", "_W", "_x", "_grid"))

    def __getattr__(self, name):             # (only reached for what this object does not hold itself)
        if name in _OwnsMembers.SHARED and "members" in self.__dict__ and self.members:
            return getattr(self.members[0], name)
        raise AttributeError(f"{type(self).__name__} has no attribute {name!r}")

    def load(self, batch):
        for s in self.members:
            s.load(batch)
        self.D = self.members[0].D


class EnsembleSession(_OwnsMembers, DecodeSession):
    """DecodeSession of an Ensemble on the launch-per-sublayer pass (full prefix or prefix K/V cache): it owns one DecodeSession per active
    member, all reading ONE tokens / pos (/ parent) tensor, and its pass is the members' passes up to their logits + mtn_ensemble_rows + the
    row heads — captured as one graph per step, exactly as a single model's pass is.  Everything the searches below do with a session
    (step_many, score, logp, top) is DecodeSession's own code on the combined rows."""

    def __init__(self, ens, batch, max_len, width, pad=1, use_graph=True, kv_cache=False, select=None):
        self.kv_cache = bool(kv_cache)
        self._own(DecodeSession, ens, batch, max_len, width, pad, use_graph, select, kv_cache=self.kv_cache)
        for s in self.members:
            s._logits = True
        if self.kv_cache:
            self._cur, self._graphs = 0, {}

    def _target_rows(self):
        return self.model.combine([s._target_rows() for s in self.members])

    def _target_rows_cached(self, cur):
        return self.model.combine([s._target_rows_cached(cur) for s in self.members])

    def _score_logits(self):
        return self.model.combine([s._score_logits() for s in self.members])


class EnsembleMegaSession(_OwnsMembers, MegaDecodeSession):
    """MegaDecodeSession of an Ensemble whose active members are ALL eligible for the persistent step: one MegaDecodeSession per member, every
    one's launch reading the SAME [tokens | pos | anc] device block — the one the bookkeeping kernels write — so the prefix-cache slots are the
    same in all of them and nothing is kept in sync.  A step is M persistent launches, M generator GEMMs (logits) and one mtn_ensemble_rows;
    the captured searches (search / greedy / sample_log) and the stepped path are MegaDecodeSession's own code on the combined rows."""

    def __init__(self, ens, batch, max_len, width, pad=1, use_graph=True, kv_cache=False, select=None):
        self.kv_cache = False
        self._own(MegaDecodeSession, ens, batch, max_len, width, pad, use_graph, select)

    def _step_rows(self, logits=False):
        return self.model.combine([s._step_rows(logits=True) for s in self.members])

    def timed_out(self) -> bool:
        """True if a poll of ANY member timed out: the members' flags are gathered on the device and read in one copy."""
        return bool(torch.stack([s._sync[1] for s in self.members]).any().item())

    def recover(self):
        """A poll of ANY member timed out: every member's device state is made consistent again."""
        for s in self.members:
            s.recover()
        self._prev = None


_SESSIONS: dict = {}
SELECT_MAX_K = 16        # csrc/select.hip SEL_MAX_K
KV_CACHE_FROM = 32      # prefix K/V cache by default for searches longer than this (at the reference's max_len = 20 the full-prefix
                        # pass is launch-latency-bound and as fast; the cache makes a token cost O(l) instead of O(l^2) work beyond it)


def _session(model, batch, max_len, width, pad, use_graph, kv_cache=False, select=None, mega=False, mode=None) -> DecodeSession:
    """Sessions are kept per (model, shapes): a dialogue with the shapes of an earlier one reuses its buffers and graph.
    The cache is dropped when the model's weights change (prepare() version) or it grows past a few shapes."""
    model.prepare()
    mega = bool(mega) and MegaDecodeSession.supported(model, batch, max_len, width)
    key = DecodeSession.signature(model, batch, max_len, width) + (bool(use_graph), bool(kv_cache), select, mega)
    if mode is not None:             # (a sampling session is not a select session with select = None: its rows are samples, not hypotheses)
        key += (mode,)
    ver = getattr(model, "_flat_version", None)
    hit = _SESSIONS.get(key)
    if hit is not None and hit[1] == ver and (hit[0].model.same_members(model) if isinstance(model, Ensemble) else hit[0].model is model):
        hit[0].load(batch)
        return hit[0]
    if len(_SESSIONS) >= 8:
        _SESSIONS.clear()
    if isinstance(model, Ensemble):
        # ONE entry that owns its members' sessions: the eviction above drops an ensemble whole, never one member's half of it
        cls = EnsembleMegaSession if mega else EnsembleSession
        sess = cls(model, batch, max_len, width, pad=pad, use_graph=use_graph, kv_cache=bool(kv_cache), select=select)
    elif mega:
        sess = MegaDecodeSession(model, batch, max_len, width, pad=pad, use_graph=use_graph, select=select)
    else:
        sess = DecodeSession(model, batch, max_len, width, pad=pad, use_graph=use_graph, kv_cache=bool(kv_cache), select=select)
    _SESSIONS[key] = (sess, ver)
    return sess


def _constraints(no_repeat_ngram, repetition_penalty):
    """(N, theta, anything on?) of a decode call's constraint keywords, checked."""
    ngram, theta = int(no_repeat_ngram), float(repetition_penalty)
    if not 0 <= ngram <= 8 or not theta >= 1.0:
        raise ValueError("no_repeat_ngram in [0, 8] (0 = off), repetition_penalty >= 1 (1 = off)")
    return ngram, theta, ngram > 0 or theta != 1.0


def _pass_select(model, batch, max_len, width, mega, select, constrained):
    """The in-pass selection a search's session is built with.  A constrained search off the persistent step selects AFTER the
    constraint launch, so its pass selects nothing (heads of unconstrained rows would be computed and thrown away); the persistent-step
    session keeps its selection: the captured search needs it, and the tie fallback steps that same session."""
    if constrained and not (mega and MegaDecodeSession.supported(model, batch, max_len, width)):
        return None
    return select


def _constrain_step(sess, hists, ngram, theta):
    """The step-by-step paths' constraint: csrc/constrain.hip in explicit-history mode on ALL rows of the session's last log-probabilities,
    in place (the captured searches run the same kernel off their step log, so both give the same rows).  ``hists``: (row, generated tokens)
    of the live rows; every other row gets an empty history.  Table and lengths travel as one block, in one copy."""
    rows, Lm = sess.logp.size(0), sess.max_len
    blk = torch.zeros(rows * (Lm + 1), dtype=torch.int32)
    for r, toks in hists:
        blk[r * Lm:r * Lm + len(toks)] = torch.tensor(list(toks), dtype=torch.int32)
        blk[rows * Lm + r] = len(toks)
    blk = blk.to(sess.logp.device)
    ops.constrain_rows(sess.logp, ngram, theta, hist=blk[:rows * Lm].view(rows, Lm), hist_len=blk[rows * Lm:])


class _Beam:
    """Hypothesis bookkeeping of data_utils.py:196-240 for one dialogue (same candidate order and tie behaviour)."""

    def __init__(self, start_symbol, unk_symbol, end_symbol, beam, penalty, min_len):
        self.unk, self.eos, self.beam, self.penalty, self.min_len = unk_symbol, end_symbol, beam, penalty, min_len
        self.hyps = [([], 0.0, [start_symbol])]
        self.parents = [0]                        # per hypothesis: the index (in the previous step's list) of the one it extends
        self.best, self.done = None, []

    def prefixes(self):
        return [h[2] for h in self.hyps]

    def advance(self, logp, l, top=None):
        """logp: (n_hyp, V) log-probabilities on the host — or None when ``top`` = (values (n,k), indices (n,k), eos column (n,))
        carries each row's k = beam+2 best entries in descending order: at most `beam` candidates per hypothesis can enter the
        new beam and at most two (<unk>, <eos>) are skipped, so the rest of the vocabulary is never looked at."""
        new, par, argmin = [], [], 0
        for h, (out, lp, st) in enumerate(self.hyps):
            if top is None:
                lp_vec = (logp[h] + lp).astype("float32")
                eos_val = float(lp_vec[self.eos])
                order = ((int(o), float(lp_vec[o])) for o in np.argsort(lp_vec)[::-1])
            else:
                vals = (top[0][h] + lp).astype("float32")
                eos_val = float(np.float32(top[2][h] + lp))
                order = ((int(o), float(v)) for o, v in zip(top[1][h], vals))
            if l >= self.min_len:
                s = eos_val + self.penalty * (len(out) + 1)
                self.done.append((out, s))
                if self.best is None or self.best < s:
                    self.best = s
            for o, s in order:
                if o == self.unk or o == self.eos:
                    continue
                if len(new) == self.beam:
                    if new[argmin][1] < s:
                        new[argmin] = (out + [o], s, st + [o])
                        par[argmin] = h
                        argmin = min(range(len(new)), key=lambda i: new[i][1])
                    else:
                        break
                else:
                    new.append((out + [o], s, st + [o]))
                    par.append(h)
                    if len(new) == self.beam:
                        argmin = min(range(len(new)), key=lambda i: new[i][1])
        self.hyps, self.parents = new, par

    def result(self, nbest):
        if self.done:
            return sorted(self.done, key=lambda h: -h[1])[:nbest], self.best
        return [([], 0)], None


def beam_search_decode_many(model, batch, max_len, start_symbol, unk_symbol, end_symbol, pad_symbol, beam=5, penalty=1.0,
                            nbest=5, min_len=1, use_graph=True, kv_cache=None, no_repeat_ngram=0, repetition_penalty=1.0,
                            beam_groups=1, diversity_penalty=0.0):
    """beam_search_decode for a Batch of D dialogues at once: the D x beam live hypotheses are the batch dimension of ONE
    target-stream pass per generated token (the pass is launch-latency-bound, so D dialogues cost little more than one).
    Returns a list of D (n-best list, best score) pairs, each equal to what the single-dialogue search returns.
    ``no_repeat_ngram`` = N > 0: no hypothesis repeats an N-gram (the token that would complete one gets -inf); ``repetition_penalty`` =
    theta > 1: the log-probability of every token a hypothesis already holds is multiplied by theta (include/mtn_hip.h mtn_constrain_rows).
    Both act on the rows before candidates are selected, on every path; rows are not renormalised, so scores under a penalty are the
    penalised ones.  Off (0, 1.0), the search is exactly the unconstrained one.
    ``beam_groups`` = G > 1: diverse (group) beam search with Hamming diversity (Vijayakumar et al. 2016; include/mtn_hip.h
    mtn_diverse_advance holds the definition).  The beam is split into G groups of beam / G hypotheses, each a beam search of its own that
    starts from <sos>; at every step the groups go in order, and group g reads its rows lowered by ``diversity_penalty`` = lambda >= 0
    times the number of hypotheses the groups before it have just extended with that token.  Scores accumulate the penalised values and
    rows are not renormalised.  A dialogue's result pools the finished hypotheses of all groups: identical token lists once (the highest
    score), sorted by score, the first ``nbest``.  G must divide beam; lambda > 0 needs G > 1.  G = 1 is the plain search, launch for launch."""
    ngram, theta, _ = _constraints(no_repeat_ngram, repetition_penalty)
    G, lam = _diverse(beam, beam_groups, diversity_penalty)
    auto = kv_cache is None          # the caller leaves the pass to us: one persistent launch per token where it applies (<= 16 hypotheses, bf16)
    if kv_cache is None:
        kv_cache = max_len > KV_CACHE_FROM
    args = (model, batch, max_len, start_symbol, unk_symbol, end_symbol, pad_symbol, beam, penalty, nbest, min_len, use_graph, kv_cache)
    kw = dict(ngram=ngram, theta=theta, groups=G, lam=lam) if G > 1 else dict(ngram=ngram, theta=theta)
    return _with_fallback(lambda mega: _beam_search_many(*args, mega=mega, **kw), auto)


def _with_fallback(search, auto):
    """``search(mega)`` on the pass the caller left to us (``auto``: the persistent step where it applies).  None: a poll of the persistent
    step timed out (compute units held by another kernel) — the search runs again on the launch-per-sublayer pass."""
    res = search(auto)
    return search(False) if res is None else res


def _mega_failed(sess) -> bool:
    """After a search on a persistent-step session: True (and the session is made consistent again) if one of its polls timed out."""
    if not sess.timed_out():
        return False
    logging.getLogger("mtn_amd").warning("decode: the persistent step timed out (not every workgroup was resident); re-running on the launch-per-sublayer pass")
    sess.recover()
    MegaDecodeSession.FALLBACKS += 1
    return True


def _beam_search_many(model, batch, max_len, start_symbol, unk_symbol, end_symbol, pad_symbol, beam, penalty, nbest, min_len, use_graph, kv_cache, mega,
                      ngram=0, theta=1.0, groups=1, lam=0.0):
    auto = mega
    constrained = ngram > 0 or theta != 1.0
    k = beam + 2
    # device-side candidate selection (csrc/select.hip) holds at most SELECT_MAX_K entries per row: wider beams keep torch.topk
    sel = (k + 1, end_symbol) if k + 1 <= SELECT_MAX_K else None
    sess = _session(model, batch, max_len, beam, pad_symbol, use_graph, kv_cache,
                    select=_pass_select(model, batch, max_len, beam, auto, sel, constrained), mega=auto)
    mega = isinstance(sess, MegaDecodeSession)
    if mega and sel is not None:
        # the whole search as one graph replay, hypothesis bookkeeping on the device; None = a tie somewhere: step by step below
        res = sess.search(beam, k, start_symbol, unk_symbol, end_symbol, penalty, min_len, nbest, ngram, theta,
                          **(dict(beam_groups=groups, diversity_penalty=lam) if groups > 1 else {}))
        if _mega_failed(sess):
            return None
        if res is not None:
            return res
    # diverse beam search (groups > 1): `groups` beams of beam / groups per dialogue, advanced in group order; beams[] lists them dialogue
    # by dialogue, group by group — with one group it is the list of the dialogues' beams
    G, Bp = groups, beam // groups
    beams = [_Beam(start_symbol, unk_symbol, end_symbol, Bp, penalty, min_len) for _ in range(sess.D * G)]
    for l in range(max_len):
        if mega:
            # the persistent step takes (row, newest token, parent row) of every live hypothesis: no prefix lists are built or searched
            # (group g of dialogue d owns rows d * width + g * beam / groups ..: the beams' rows are Bp apart)
            live = [j * Bp + i for j, bm in enumerate(beams) for i in range(len(bm.hyps))]
            sess.step_extend(l + 1, live, [h[2][-1] for bm in beams for h in bm.hyps],
                             [j * Bp + p for j, bm in enumerate(beams) for p in bm.parents])
        else:
            # the launch passes take a dialogue's live prefixes packed, group after group (two groups may hold the same prefix: the prefix
            # cache's parent lookup then finds the first of them, whose cache rows hold the same values)
            packed_n = [lp.size(0) for lp in sess.step_many([[p for bm in beams[d * G:d * G + G] for p in bm.prefixes()] for d in range(sess.D)])]
            live = [r for d, n in enumerate(packed_n) for r in range(d * sess.width, d * sess.width + n)]
        counts = [len(bm.hyps) for bm in beams]
        top = sess.top
        if constrained:
            # the rows are rewritten in place before anything is selected from them: the pass selected nothing (_pass_select), except on
            # the persistent step, whose heads are of the unconstrained rows and are not read
            _constrain_step(sess, list(zip(live, [h[0] for bm in beams for h in bm.hyps])), ngram, theta)
            top = ops.topk_rows(sess.logp, min(k + 1, sess.logp.size(1)), end_symbol) if sel is not None else None
        if top is not None:
            # device-side selection inside the pass (csrc/select.hip): only the heads of the rows travel, in one copy
            full = (sess.top_host() if mega and not constrained else top.cpu().numpy()).astype("float64")
            packed = full[live]
            kk = (packed.shape[1] - 1) // 2
            allp = None
        else:
            allp = sess.logp[live]
            tv, ti = torch.topk(allp, min(k + 1, allp.size(1)), dim=-1)
            packed = torch.cat([tv.double(), ti.double(), allp[:, end_symbol:end_symbol + 1].double()], 1).cpu().numpy()
            kk = tv.size(1)
        vals, idx, eos = packed[:, :kk], packed[:, kk:2 * kk].astype("int64"), packed[:, 2 * kk]
        # exact ties inside a row's head would make the visiting order depend on the selection algorithm: the reference's
        # order (argsort, data_utils.py:219) is then taken from the full row
        tie = bool((vals[:, 1:] == vals[:, :-1]).any())
        if G > 1:
            rows = lambda: (allp if allp is not None else sess.logp[live]).float().cpu().numpy()
            _diverse_advance(beams, G, l, lam, vals, idx, eos, Bp + 2, rows, tie)
            continue
        host = (allp if allp is not None else sess.logp[live]).double().cpu().numpy() if tie else None
        o = 0
        for bm, n in zip(beams, counts):
            if tie:
                bm.advance(host[o:o + n], l)
            else:
                bm.advance(None, l, top=(vals[o:o + n, :k], idx[o:o + n, :k], eos[o:o + n]))
            o += n
    if mega and _mega_failed(sess):
        return None
    if G > 1:
        # a group's finished hypotheses carry their step (the length): pooled by step, then group, then hypothesis (sorted() is stable)
        return [_pool_groups(sorted((h for bm in beams[d * G:d * G + G] for h in bm.done), key=lambda h: len(h[0])), nbest) for d in range(sess.D)]
    return [bm.result(nbest) for bm in beams]


def _diverse(beam, beam_groups, diversity_penalty):
    """(G, lambda) of a beam search's diversity keywords, checked."""
    G, lam = int(beam_groups), float(diversity_penalty)
    if G != beam_groups or G < 1 or int(beam) % G:
        raise ValueError("beam_groups is an integer >= 1 that divides beam")
    if not (math.isfinite(lam) and lam >= 0.0):
        raise ValueError("diversity_penalty is finite and >= 0")
    if lam > 0.0 and G == 1:
        raise ValueError("diversity_penalty > 0 needs beam_groups > 1 (one group is the plain beam search)")
    return G, lam


def _pool_groups(done, nbest):
    """The result of a diverse search for one dialogue: ``done`` = the finished hypotheses of all its groups in the order step, group,
    hypothesis.  Identical token lists are kept once (the highest score; on equal scores the first), the pool is sorted by score (stable)."""
    at = {}
    for i, (toks, s) in enumerate(done):
        j = at.get(tuple(toks))
        if j is None or done[j][1] < s:
            at[tuple(toks)] = i
    kept = [done[i] for i in sorted(at.values())]
    if not kept:
        return [([], 0)], None
    return sorted(kept, key=lambda h: -h[1])[:nbest], max(h[1] for h in kept)


def _diverse_advance(beams, G, l, lam, vals, idx, eos, k, rows, tie):
    """One step of the G groups of every dialogue (include/mtn_hip.h mtn_diverse_advance), on the host: group g's rows are lowered by
    fl32(lambda * count) for the newest tokens of the final new beams of the groups before it, in float32 as the kernel does it.  vals / idx
    / eos: the live rows' heads in the beams' order; they are penalised, re-sorted (stable, descending) and their first k entries walked.
    A tie inside a head, before the penalty (``tie``) or after it, sends the WHOLE step down the full-row path (``rows()``: the live rows,
    fp32): the groups are put back as they were and advanced again on the penalised full rows, whose argsort is the reference's order."""
    f32 = np.float32

    def run(full):
        o = 0
        for j, bm in enumerate(beams):
            if j % G == 0:
                chosen = {}
            n = len(bm.hyps)
            if full is not None:
                r = full[o:o + n].copy()
                for t, c in chosen.items():
                    r[:, t] = r[:, t] - f32(lam) * f32(c)
                bm.advance(r.astype("float64"), l)
            else:
                v, ix = vals[o:o + n].astype(f32), idx[o:o + n]
                c = np.array([[chosen.get(int(t), 0) for t in row] for row in ix], dtype=f32).reshape(ix.shape)
                pv = (v - (f32(lam) * c).astype(f32)).astype(f32)
                order = np.argsort(-pv.astype("float64"), axis=1, kind="stable")
                pv, ix = np.take_along_axis(pv, order, 1), np.take_along_axis(ix, order, 1)
                if (pv[:, 1:] == pv[:, :-1]).any():
                    return False
                bm.advance(None, l, top=(pv[:, :k].astype("float64"), ix[:, :k], eos[o:o + n]))
            o += n
            for h in bm.hyps:
                chosen[h[2][-1]] = chosen.get(h[2][-1], 0) + 1
        return True

    if not tie:
        saved = [(bm.hyps, bm.parents, bm.best, len(bm.done)) for bm in beams]
        if run(None):
            return
        for bm, (hyps, parents, best, n_done) in zip(beams, saved):
            bm.hyps, bm.parents, bm.best = hyps, parents, best
            del bm.done[n_done:]
    run(rows())


def beam_search_decode(model, batch, max_len, start_symbol, unk_symbol, end_symbol, pad_symbol, beam=5, penalty=1.0,
                       nbest=5, min_len=1, use_graph=True, kv_cache=None, no_repeat_ngram=0, repetition_penalty=1.0,
                       beam_groups=1, diversity_penalty=0.0):
    """data_utils.py:188-242, same arguments and return value: (n-best list of (token list, score) sorted by score,
    best score).  A hypothesis ending with <eos> at length k scores logp + penalty * k; <unk> and <eos> never extend
    a hypothesis; candidates are visited in descending log-probability exactly as the reference does (data_utils.py:219).
    no_repeat_ngram / repetition_penalty / beam_groups / diversity_penalty: as beam_search_decode_many (off by default)."""
    if batch.query.size(0) != 1:
        raise ValueError("beam_search_decode works on one dialogue (data_utils.py:188); use beam_search_decode_many for a batch")
    return beam_search_decode_many(model, batch, max_len, start_symbol, unk_symbol, end_symbol, pad_symbol, beam, penalty, nbest,
                                   min_len, use_graph, kv_cache, no_repeat_ngram, repetition_penalty, beam_groups, diversity_penalty)[0]


def greedy_decode(model, batch, max_len, start_symbol, pad_symbol=1, use_graph=True, kv_cache=None, no_repeat_ngram=0, repetition_penalty=1.0):
    """data_utils.py:159-186 (the reference's own greedy_decode cannot run: it calls decode() with the wrong arity, SURVEY
    §8c) — pinned to: argmax of the generator's log-probabilities at every step, (1, max_len) tokens incl. <sos>.
    no_repeat_ngram / repetition_penalty (off by default): the argmax is taken over the constrained row, as in beam_search_decode_many."""
    if batch.query.size(0) != 1:
        raise ValueError("greedy_decode works on one dialogue (data_utils.py:159); use greedy_decode_many for a batch")
    return greedy_decode_many(model, batch, max_len, start_symbol, pad_symbol, use_graph, kv_cache, no_repeat_ngram, repetition_penalty)


def greedy_decode_many(model, batch, max_len, start_symbol, pad_symbol=1, use_graph=True, kv_cache=None, no_repeat_ngram=0,
                       repetition_penalty=1.0):
    """greedy_decode for a Batch of D dialogues at once: (D, max_len) tokens incl. <sos>, row d equal to greedy_decode on
    dialogue d alone.  On the persistent step the D argmax searches are ONE graph replay; otherwise the D rows are the batch
    dimension of one target-stream pass per token.  no_repeat_ngram / repetition_penalty: as greedy_decode."""
    ngram, theta, _ = _constraints(no_repeat_ngram, repetition_penalty)
    ys = _with_fallback(lambda mega: _greedy_many(model, batch, max_len, start_symbol, pad_symbol, use_graph, kv_cache, mega, ngram, theta),
                        kv_cache is None)
    return torch.tensor(ys, dtype=batch.query.dtype, device=batch.query.device)


def _greedy_many(model, batch, max_len, start_symbol, pad_symbol, use_graph, kv_cache, auto, ngram=0, theta=1.0):
    constrained = ngram > 0 or theta != 1.0
    sess = _session(model, batch, max_len, 1, pad_symbol, use_graph, max_len > KV_CACHE_FROM if kv_cache is None else kv_cache,
                    select=_pass_select(model, batch, max_len, 1, auto, (2, 0) if auto else None, constrained), mega=auto)
    D = sess.D
    ys = [[start_symbol] for _ in range(D)]
    if isinstance(sess, MegaDecodeSession) and sess.select is not None:
        # the whole decode as one graph replay (None: a tie in some row's head)
        toks = sess.greedy(start_symbol, ngram, theta)
        if toks is None:
            # step by step: every dialogue's row head (largest log-probability, its column; row d = dialogue d at width 1) arrives in a
            # pinned block — one replay and one stream synchronisation per token, no argmax launch, no .item()
            rows = list(range(D))
            for l in range(1, max_len):
                sess.step_extend(l, rows, [y[-1] for y in ys], rows)
                if constrained:          # (the head the pass took is of the unconstrained row)
                    _constrain_step(sess, [(d_, ys[d_][1:]) for d_ in rows], ngram, theta)
                    top = ops.topk_rows(sess.logp, 2, 0).cpu().numpy()
                else:
                    top = sess.top_host()
                for d_ in rows:
                    ys[d_].append(int(top[d_, 2]))
        else:
            ys = [[start_symbol] + t for t in toks]
        return None if _mega_failed(sess) else ys
    for _ in range(max_len - 1):
        logps = sess.step_many([[y] for y in ys])
        if constrained:
            _constrain_step(sess, [(d_ * sess.width, y[1:]) for d_, y in enumerate(ys)], ngram, theta)      # (in place: `logps` are views)
        logp = torch.cat(logps, 0)
        for y, nxt in zip(ys, logp.argmax(dim=-1).tolist()):
            y.append(int(nxt))
    return ys


def sample_decode_many(model, batch, max_len, start, eos, pad, *, samples=1, temperature=1.0, top_k=0, top_p=1.0, seed=0, keys=None,
                       banned=(), min_len=1, penalty=0.0, use_graph=True, kv_cache=None, trace=None, no_repeat_ngram=0, repetition_penalty=1.0,
                       mbr=0):
    """Stochastic decoding of a Batch of D dialogues x ``samples`` draws each (temperature / top-k / nucleus; include/mtn_hip.h
    mtn_sample_rows defines the filters).  Row d * samples + s draws with the random stream of key keys[d] * samples + s (keys: 0..D-1
    by default) under ``seed``: a pure function of (seed, key, position), so a dialogue's samples do not depend on what it is batched with.
    Every row starts at <sos> and is cut at its first <eos> (at max_len - 1 tokens without one); <eos> cannot be drawn before ``min_len``
    tokens, ``banned`` ids never.
    Returns per dialogue its (tokens up to <eos>, score) pairs, best first: score = sum of the drawn tokens' log-probabilities (the
    model's, <eos> included) + penalty * (len + 1) — a finished beam hypothesis' formula.  temperature = 0 means top_k = 1.
    On the persistent step (<= 16 rows, bf16) the whole search is one graph replay; elsewhere the launch-per-sublayer pass runs per token
    and the same kernel draws from its rows.  ``trace``: a list that receives (row keys, tokens, log-probabilities, u), each log
    (max_len, rows), of this search.
    no_repeat_ngram / repetition_penalty (off by default; include/mtn_hip.h mtn_constrain_rows): every row's log-probabilities are
    rewritten from that row's own draws before the filters see them, so no sample repeats an N-gram before its <eos>; the logged
    log-probabilities, and so the scores, are the penalised ones under a penalty.
    ``mbr`` = N in 1..4 (0: off): minimum-Bayes-risk selection of n-gram order N with uniform weights — the right ones for draws from the
    model — over each dialogue's samples (include/mtn_hip.h mtn_mbr_select; at most 16 samples, max_len <= 128): one more launch, the last
    node of the captured search on the persistent step, once after the token loop elsewhere; it changes no draw.  The result is then per
    dialogue its (tokens, score, expected utility) triples, largest expected utility first (equal ones in sample order)."""
    ngram, theta, _ = _constraints(no_repeat_ngram, repetition_penalty)
    D, S, mbr = batch.query.size(0), int(samples), int(mbr)
    if S < 1 or len(banned) > 4:
        raise ValueError("sample_decode_many: samples >= 1, at most 4 banned tokens")
    if not 0 <= mbr <= ops.MBR_MAX_ORDER or (mbr and (S > ops.MBR_MAX_HYP or max_len > ops.MBR_MAX_LEN)):
        raise ValueError("sample_decode_many: mbr in 0..4; with it at most 16 samples and max_len <= 128")
    if temperature == 0:
        temperature, top_k = 1.0, 1
    if not (temperature > 0 and top_k >= 0 and 0 < top_p <= 1):
        raise ValueError("sample_decode_many: temperature >= 0, top_k >= 0, 0 < top_p <= 1")
    keys = list(range(D)) if keys is None else [int(k) for k in keys]
    if len(keys) != D:
        raise ValueError("one key per dialogue")
    row_keys = [k * S + s for k in keys for s in range(S)]
    params = dict(temperature=float(temperature), top_k=int(top_k), top_p=float(top_p), banned=tuple(int(b) for b in banned), eos=int(eos),
                  min_len=int(min_len))
    log = _with_fallback(lambda mega: _sample_search(model, batch, max_len, start, pad, S, seed, row_keys, params, use_graph, kv_cache, mega,
                                                     ngram, theta, mbr), kv_cache is None)
    tok, lp, u = log[:3]
    if trace is not None:
        trace.append((list(row_keys), tok.copy(), lp.copy(), u.copy()))
    results = []
    for d in range(D):
        hyps = []
        for r in range(d * S, d * S + S):
            col = [int(t) for t in tok[:, r]]
            # tokens before <eos>; a row without one keeps max_len - 1 tokens, the longest a beam hypothesis (and the greedy output) gets
            n = col.index(eos) if eos in col else len(col) - 1
            used = n + 1 if eos in col else n
            hyps.append((col[:n], float(lp[:used, r].astype("float64").sum()) + penalty * (n + 1)))
        if mbr:                      # the kernel cut the same columns at the same places: its order and expected utilities, as they are
            expected, order = log[3], log[4]
            results.append([hyps[int(j)] + (float(expected[d, j]),) for j in order[d]])
        else:
            results.append(sorted(hyps, key=lambda h: -h[1]))
    return results


def _sample_search(model, batch, max_len, start, pad, S, seed, row_keys, params, use_graph, kv_cache, mega, ngram=0, theta=1.0, mbr=0,
                   on_device=False):
    """The step log (tokens, log-probabilities, u — numpy, (max_len, rows)) of one sampling search, or None after a persistent-step timeout.
    With ``mbr`` the selection's expected utilities and order, each (D, S), follow the log.  ``on_device`` (launch-per-sublayer pass, no
    mbr): the session's device log itself, valid until the session's next search — what the train step's reward launches read."""
    if on_device and (mega or mbr):
        raise ValueError("_sample_search: the device log is the launch-per-sublayer pass', without mbr")
    sess = _session(model, batch, max_len, S, pad, use_graph, max_len > KV_CACHE_FROM if kv_cache is None else kv_cache, select=None,
                    mega=mega and use_graph, mode="sample")
    if isinstance(sess, MegaDecodeSession):
        log = sess.sample_log(start, seed, row_keys, params, ngram, theta, mbr)
        if _mega_failed(sess):
            return None
        return log
    W, D = sess.D * S, sess.D
    dev = batch.query.device
    st = getattr(sess, "_sample_state", None)
    if st is None:                   # [seed | keys | step] and the log, per session
        st = sess._sample_state = (torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros(W, dtype=torch.int64, device=dev),
                                   torch.zeros(W, dtype=torch.int32, device=dev),
                                   (torch.zeros(max_len, W, dtype=torch.int32, device=dev), torch.zeros(max_len, W, device=dev),
                                    torch.zeros(max_len, W, device=dev)))
    seed_t, keys_t, step_t, log = st
    seed_t.fill_(int(seed))
    keys_t.copy_(torch.tensor(row_keys, dtype=torch.int64))
    step_t.zero_()
    prefixes = [[start] for _ in range(W)]
    for l in range(max_len):
        sess.step_many([prefixes[d * S:d * S + S] for d in range(D)])
        if ngram > 0 or theta != 1.0:        # a row's history is its own column of the token log, up to its step counter
            ops.constrain_rows(sess.logp, ngram, theta, log_tok=log[0], step=step_t, width=1, rows_per_step=1)
        ops.sample_rows(sess.logp, seed_t, keys_t, step_t, log, **params)      # the session's rows ARE d * S + s: all of them live
        for p, t in zip(prefixes, log[0][l].tolist()):
            p.append(int(t))
    if mbr:                          # once, after the token loop, on the device log
        expected, _, order, _ = ops.mbr_select(mbr, log_tok=log[0], sets=D, eos=params["eos"])
        return tuple(t.cpu().numpy() for t in log + (expected, order))
    if on_device:
        return log
    return tuple(t.cpu().numpy() for t in log)


def _contrastive(k, alpha, banned=()):
    """(k, alpha, banned ids) of a contrastive search's keywords, checked."""
    kk, a = int(k), float(alpha)
    if kk != k or not 1 <= kk <= ops.CONTRASTIVE_MAX_K:
        raise ValueError("contrastive search: k is an integer in 1..%d" % ops.CONTRASTIVE_MAX_K)
    if not 0.0 <= a <= 1.0:                      # (a NaN fails both comparisons)
        raise ValueError("contrastive search: alpha is in [0, 1]")
    banned = tuple(int(b) for b in banned)
    if len(banned) > 4:
        raise ValueError("contrastive search: at most 4 banned tokens")
    return kk, a, banned


def contrastive_decode_many(model, batch, max_len, start, eos, pad, *, k=5, alpha=0.6, banned=(), min_len=1, penalty=0.0, use_graph=True,
                            trace=None):
    """Contrastive search (Su et al. 2022) for a Batch of D dialogues: at every position the next token is, among the ``k`` most probable
    ones, the one that maximises (1 - alpha) * p(token) - alpha * max cosine between the decoder's final-norm state of that token and the
    states of the prefix (include/mtn_hip.h mtn_contrastive_advance holds the definition).  Deterministic; alpha = 0 or k = 1 is greedy.
    <eos> is no candidate before ``min_len`` tokens, ``banned`` ids never; a response ends at its <eos>, or at max_len - 1 tokens.
    Dialogue d's k candidates are rows d * k .. of ONE full-prefix launch-per-sublayer pass per token (the persistent step keeps no hidden
    rows, and the prefix-K/V pass would need a history of them), and the whole search is one captured body replayed max_len times with the
    selection on the device: the host synchronises once (DecodeSession.contrastive_log).  One model only: no Ensemble.
    Returns per dialogue (tokens up to <eos>, score, log-probabilities, penalties, ranks): score = sum of the chosen tokens'
    log-probabilities (the model's own, <eos> included) + penalty * (len + 1), a finished sample's formula; the three lists hold, per
    chosen token (<eos> included), its log-probability, its degeneration penalty and its rank among the k candidates (0: the most probable).
    ``trace``: a list that receives the numpy logs (tokens, log-probabilities, penalties, ranks), each (max_len, D), and — eager runs only
    (use_graph=False) — after them the per-step dicts of what the kernel read (hidden, top, tokens, cand_logp, step, done)."""
    k, alpha, banned = _contrastive(k, alpha, banned)
    if isinstance(model, Ensemble):
        raise ValueError("contrastive_decode_many: one model (the degeneration penalty reads ONE decoder's states), not an Ensemble")
    sess = _session(model, batch, max_len, k, pad, use_graph, False, select=None, mega=False, mode="contrastive")
    steps = [] if (trace is not None and not sess.use_graph) else None
    tok, lp, pen, rank = sess.contrastive_log(start, k, alpha, eos, min_len, banned, trace=steps)
    if trace is not None:
        trace.append((tok, lp, pen, rank) + ((steps,) if steps is not None else ()))
    results = []
    for d in range(sess.D):
        col = [int(t) for t in tok[1:, d]]
        n = col.index(eos) if eos in col else len(col)
        used = n + 1 if eos in col else n
        results.append((col[:n], float(lp[1:1 + used, d].astype("float64").sum()) + penalty * (n + 1), [float(v) for v in lp[1:1 + used, d]],
                        [float(v) for v in pen[1:1 + used, d]], [int(v) for v in rank[1:1 + used, d]]))
    return results


def mbr_weights(scores, temperature=1.0):
    """The ``score`` weights of mbr_rerank: w_j = exp((s_j - max s) / temperature) / sum, float64, the sum in ascending j."""
    top = max(scores)
    e = [math.exp((float(v) - float(top)) / float(temperature)) for v in scores]
    z = 0.0
    for v in e:
        z = z + v
    return [v / z for v in e]


def mbr_rerank(lists, ngram, weights="uniform", temperature=1.0, device=None):
    """Minimum-Bayes-risk re-ranking of hypothesis lists (include/mtn_hip.h mtn_mbr_select; csrc/mbr.hip): ``lists[d]`` is dialogue d's
    list of (tokens, score) pairs, as sample_decode_many and the beam search return them (at most 16 of at most 128 tokens; lists may
    differ in length or be empty).  One launch for all dialogues.  ``ngram``: the maximum n-gram order, 1..4.  ``weights``: "uniform", or
    "score" — w_j = exp((s_j - max s) / temperature) / sum over the list, computed here in float64.
    Returns per dialogue its (tokens, score, expected utility) triples, largest expected utility first, equal ones in input order."""
    lists = [list(l) for l in lists]
    if weights not in ("uniform", "score"):
        raise ValueError("mbr_rerank: weights is 'uniform' or 'score'")
    if not float(temperature) > 0:
        raise ValueError("mbr_rerank: temperature > 0")
    if not 1 <= int(ngram) <= ops.MBR_MAX_ORDER:
        raise ValueError("mbr_rerank: the n-gram order is in 1..4")
    if any(len(l) > ops.MBR_MAX_HYP for l in lists) or any(len(h[0]) > ops.MBR_MAX_LEN for l in lists for h in l):
        raise ValueError("mbr_rerank: at most 16 hypotheses per list, of at most 128 tokens")
    if not lists:
        return []
    S, K = len(lists), max(1, max(len(l) for l in lists))
    Lh = max([1] + [len(h[0]) for l in lists for h in l])
    tok, length = np.zeros((S, K, Lh), dtype=np.int32), np.zeros((S, K), dtype=np.int32)
    n_hyp = np.asarray([len(l) for l in lists], dtype=np.int32)
    w = np.zeros((S, K), dtype=np.float64) if weights == "score" else None
    for d, l in enumerate(lists):
        for k, h in enumerate(l):
            tok[d, k, :len(h[0])] = np.asarray(h[0], dtype=np.int64).astype(np.int32)
            length[d, k] = len(h[0])
        if w is not None and l:
            w[d, :len(l)] = mbr_weights([h[1] for h in l], temperature)
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    up = lambda a: None if a is None else torch.from_numpy(a).to(dev)
    expected, _, order, _ = ops.mbr_select(ngram, tok=up(tok), length=up(length), n_hyp=up(n_hyp), w=up(w))
    expected, order = expected.cpu().numpy(), order.cpu().numpy()
    return [[(l[j][0], l[j][1], float(expected[d, j])) for j in order[d, :len(l)].tolist()] for d, l in enumerate(lists)]


EVAL_NAMES = ("Bleu_1", "Bleu_2", "Bleu_3", "Bleu_4", "ROUGE_L", "CIDEr")


def evaluate_responses(hyps, refs, device=None):
    """BLEU-1..4, ROUGE-L and CIDEr of generated responses on the device (include/mtn_hip.h mtn_eval_metrics; csrc/eval.hip).  ``hyps[q]`` is
    item q's hypothesis as a list of token ids, ``refs[q]`` the list of its 1..8 references (token-id lists); any ids, sentences of at
    most 128 tokens (ValueError names the first item that breaks a bound).  The whole corpus is one call whatever its size: the document
    frequencies are the corpus'.  Returns dict(Bleu_1 .. Bleu_4, ROUGE_L, CIDEr: floats; hyp_len, ref_len: the corpus sums of hypothesis
    and closest reference lengths; stats (Q, 10) int32, rouge (Q,), cider (Q,) float64 numpy arrays, per item)."""
    hyps, refs = [list(h) for h in hyps], [[list(r) for r in rs] for rs in refs]
    if len(hyps) != len(refs):
        raise ValueError("evaluate_responses: one reference list per hypothesis (%d and %d)" % (len(hyps), len(refs)))
    if not hyps:
        raise ValueError("evaluate_responses: nothing to evaluate")
    for q, (h, rs) in enumerate(zip(hyps, refs)):
        if not 1 <= len(rs) <= ops.EVAL_MAX_REF:
            raise ValueError("evaluate_responses: item %d has %d references (1..%d)" % (q, len(rs), ops.EVAL_MAX_REF))
        if len(h) > ops.EVAL_MAX_LEN or any(len(r) > ops.EVAL_MAX_LEN for r in rs):
            raise ValueError("evaluate_responses: item %d holds a sentence of more than %d tokens" % (q, ops.EVAL_MAX_LEN))
    Q, R = len(hyps), max(len(rs) for rs in refs)
    Lh = max([1] + [len(h) for h in hyps] + [len(r) for rs in refs for r in rs])
    tok = np.zeros((Q, R + 1, Lh), dtype=np.int32)                # row R of an item: its hypothesis
    length = np.zeros((Q, R + 1), dtype=np.int32)
    for q, (h, rs) in enumerate(zip(hyps, refs)):
        for r, s in enumerate(rs + [None] * (R - len(rs)) + [h]):
            if s is not None:
                tok[q, r, :len(s)] = np.asarray(s, dtype=np.int64).astype(np.int32)
                length[q, r] = len(s)
    if device is None:                                           # (without a GPU the tensors stay on the host and ops.eval_metrics refuses them)
        device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else "cpu"
    dev = torch.device(device)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    ref_tok, hyp_tok = up(tok[:, :R]), up(tok[:, R])
    n_ref = up(np.asarray([len(rs) for rs in refs], dtype=np.int32))
    stats, rouge, cider, corpus, _ = ops.eval_metrics(hyp_tok, up(length[:, R]), ref_tok, up(length[:, :R]), n_ref)
    corpus = corpus.cpu().numpy()
    out = {k: float(v) for k, v in zip(EVAL_NAMES, corpus[:6])}
    out.update(hyp_len=int(corpus[6]), ref_len=int(corpus[7]), stats=stats.cpu().numpy(), rouge=rouge.cpu().numpy(), cider=cider.cpu().numpy())
    return out


def score_candidates(model, batch, candidates, start, eos, pad, *, penalty=0.0, max_len=None, width=None, use_graph=True):
    """Teacher-forced log-likelihood of GIVEN responses: candidates[d] is a list of token-id lists (no <sos> / <eos>; empty lists
    allowed; counts may differ) for dialogue d of ``batch``.  The encoder side and the auto-encoder chains run once per call
    (DecodeSession.load); the candidates are the rows of one teacher-forced pass per ``width`` of them — input [<sos>, c...], target
    [c..., <eos>] — whose logits mtn_score_rows (csrc/score.hip) turns into per-token log-probabilities and ranks.  ``max_len``: longest
    candidate + 1 rounded up to a multiple of 8 by default (a candidate that does not fit an explicit one raises ValueError);
    ``width``: min(most candidates of a dialogue, 32) by default; more candidates run as further passes of the same loaded session, and
    short rows are filled with copies of the dialogue's last candidate and dropped.
    Returns per dialogue, in input order, dict(logp, n_tokens, score, token_logp, token_rank): logp = sum of the tokens'
    log-probabilities, <eos> included (n_tokens counts it), score = logp + penalty * n_tokens — what the beam search assigns the same
    tokens as a finished hypothesis (data_utils.py:211-215).  token_rank: 0 where the token is the model's arg-max.
    Launch-per-sublayer pass for both compute dtypes; the persistent step is not involved."""
    D = batch.query.size(0)
    if len(candidates) != D:
        raise ValueError("score_candidates: one candidate list per dialogue of the batch")
    cands = [[[int(t) for t in c] for c in cs] for cs in candidates]
    longest = max((len(c) for cs in cands for c in cs), default=0)
    if max_len is None:
        max_len = -(-(longest + 1) // 8) * 8
    elif longest + 1 > max_len:
        raise ValueError(f"score_candidates: a candidate of {longest} tokens (+ <eos>) does not fit max_len = {max_len}")
    most = max(len(cs) for cs in cands)
    results = [[] for _ in range(D)]
    if most == 0:
        return results
    width = min(most, 32) if width is None else int(width)
    if width < 1:
        raise ValueError("score_candidates: width >= 1")
    sess = _session(model, batch, max_len, width, pad, use_graph, False, select=None, mega=False, mode="score")
    for c0 in range(0, most, width):
        rows = []
        for cs in cands:
            chunk = cs[c0:c0 + width]
            rows += chunk + [cs[-1] if cs else []] * (width - len(chunk))
        tok_logp, tok_rank, seq_logp, seq_len = sess.score(rows, start, eos)
        for d, cs in enumerate(cands):
            for i, c in enumerate(cs[c0:c0 + width]):
                r, n = d * width + i, len(c) + 1
                lp, counted = float(seq_logp[r]), int(seq_len[r])
                results[d].append(dict(logp=lp, n_tokens=counted, score=lp + penalty * counted,
                                       token_logp=[float(v) for v in tok_logp[r, :n]], token_rank=[int(v) for v in tok_rank[r, :n]]))
    return results
