"""Host references for the direct tests of the table launch's optimiser front tiles (tests/test_table_aux_gpu.py:
mtn_gemm_tt_table_aux, csrc/gemm.hip tt_front_tile); validated without a GPU by tests/test_table_refs.py.  Plain helpers, no
fixtures.

finalize_f32    the summation order of ln_bwd_finalize_kernel (csrc/layernorm.hip) restated with IEEE float32 additions on the
                host: the same bits as the kernel (the header's "same summation order, same bits" contract of the front tiles).
finalize_f64    the float64 column sum.
finalize_bound  a DERIVED bound on |float32 sum - exact sum| per column: every addend passes through at most
                ceil(nparts / 64) + 11 float32 additions, each of which costs at most 2^-24 relative to its own result, and no
                partial result exceeds sum |partial_i|.  The additions: chain s0 of a group of interleaved rows receives every
                fourth of the group's ceil(nparts / 16) rows from the two stride loops (at most ceil(nparts / 64)) and up to 3 tail
                rows; then 2 chain combines ((s0 + s1) + (s2 + s3)), 2 quad combines of the 16 group sums, 4 additions into t.
Layout          a seeded placement of LayerNorm gain / bias slots, Linear-bias slots and Adam chunks in one flat buffer, with holes.
Adam            row_refs.adam_inputs / adam_step64 / noam_state64 (nothing new here).
"""
from collections import namedtuple

import numpy as np
import torch

NPARTS = (1, 15, 16, 17, 48, 49, 64, 65, 112, 113, 128, 129, 241, 300, 513)       # around every loop bound of the kernel
REF_COLS = 272


def partials(nparts, cols, seed):
    """float32 [nparts, cols]: row i is N(0.2, sigma_i^2) with its own sigma_i in [0.05, 2.7] (the partial rows of a LayerNorm
    backward share a sign bias and differ in scale)."""
    gen = torch.Generator().manual_seed(seed)
    sigma = torch.exp(torch.rand(nparts, 1, generator=gen) * 4.0 - 3.0)
    return (torch.randn(nparts, cols, generator=gen) * sigma + 0.2).float()


def _np32(partial):
    x = partial.detach().cpu().numpy() if isinstance(partial, torch.Tensor) else np.asarray(partial)
    assert x.ndim == 2 and x.dtype == np.float32
    return x


def finalize_f32(partial):
    """[nparts, cols] float32 -> [cols] float32, in ln_bwd_finalize_kernel's order.  16 interleaved groups (rows q, q + 16, ...);
    each group dealt to four chains by the loops `i + 112 < n` (step 128: rows i, i+16, .., i+112 to chains 0 1 2 3 0 1 2 3),
    `i + 48 < n` (step 64: rows i, i+16, i+32, i+48 to chains 0 1 2 3) and a tail into chain 0; chains combined as
    (s0 + s1) + (s2 + s3); the 16 group sums as t += (r[k] + r[k+1]) + (r[k+2] + r[k+3]) for k = 0, 4, 8, 12."""
    x = _np32(partial)
    n, cols = x.shape
    red = []
    for q in range(16):
        s = [np.zeros(cols, np.float32) for _ in range(4)]
        i = q
        while i + 112 < n:
            for k in range(8):
                s[k & 3] = s[k & 3] + x[i + 16 * k]
            i += 128
        while i + 48 < n:
            for k in range(4):
                s[k] = s[k] + x[i + 16 * k]
            i += 64
        while i < n:
            s[0] = s[0] + x[i]
            i += 16
        red.append((s[0] + s[1]) + (s[2] + s[3]))
    t = np.zeros(cols, np.float32)
    for k in range(0, 16, 4):
        t = t + ((red[k] + red[k + 1]) + (red[k + 2] + red[k + 3]))
    assert t.dtype == np.float32
    return torch.from_numpy(t)


def index_order_f32(partial):
    """The same sum in plain row order (float32): NOT the kernel's order."""
    x = _np32(partial)
    t = np.zeros(x.shape[1], np.float32)
    for row in x:
        t = t + row
    return torch.from_numpy(t)


def finalize_f64(partial):
    return torch.from_numpy(_np32(partial).astype(np.float64).sum(0))


def finalize_depth(nparts):
    """The longest chain of float32 additions an addend of finalize_f32 passes through (see the module docstring)."""
    return (nparts + 63) // 64 + 11


def finalize_bound(partial):
    x = _np32(partial)
    return torch.from_numpy(finalize_depth(x.shape[0]) * 2.0 ** -24 * np.abs(x.astype(np.float64)).sum(0))


# ------------------------------------------------------------------------------------------ flat-buffer layout
LnSlot = namedtuple("LnSlot", "d a_off b_off")
BiasSlot = namedtuple("BiasSlot", "n off")
Chunk = namedtuple("Chunk", "off len")
GAPS = (4, 8, 64, 12, 132)          # holes between neighbours, in elements: multiples of 4, so every slot starts on a float4
SLACK = 64                          # behind the last slot: part of the allocation, never listed
MANY_CHUNKS = [4096] + [(4, 8, 12)[k % 3] for k in range(2039)]       # one long chunk, then short ones: 2040, with 5 LayerNorm units 2045 front tiles


class Layout:
    """n_flat, ln [LnSlot], bias [BiasSlot], chunks [Chunk] (ascending offsets) and one boolean mask [n_flat] per category
    ('ln', 'bias', 'chunk'; `untouched` = in none of them)."""

    def __init__(self, n_flat, ln, bias, chunks):
        self.n_flat, self.ln, self.bias, self.chunks = n_flat, ln, bias, chunks
        self.masks = {k: torch.zeros(n_flat, dtype=torch.bool) for k in ("ln", "bias", "chunk")}
        for s in ln:
            self.masks["ln"][s.a_off:s.a_off + s.d] = True
            self.masks["ln"][s.b_off:s.b_off + s.d] = True
        for s in bias:
            self.masks["bias"][s.off:s.off + s.n] = True
        for c in chunks:
            self.masks["chunk"][c.off:c.off + c.len] = True
        self.check()

    @property
    def untouched(self):
        return ~(self.masks["ln"] | self.masks["bias"] | self.masks["chunk"])

    def ranges(self, kind):
        """[(off, n)] of a category; a LayerNorm contributes its gain and its bias range"""
        if kind == "ln":
            return [r for s in self.ln for r in ((s.a_off, s.d), (s.b_off, s.d))]
        return [(s.off, s.n) for s in self.bias] if kind == "bias" else [(c.off, c.len) for c in self.chunks]

    def check(self):
        """The categories are pairwise disjoint, no two slots overlap, everything lies inside n_flat, and the offsets meet the
        rules of mtn_tt_aux (chunks: 0 < len <= 4096, offset and length multiples of 4) and of the separate passes the tests
        compare with (mtn_adam_step on a sub-range: offset and length multiples of 4; GEMM problems: M a multiple of 8)."""
        every = [(o, n) for k in ("ln", "bias", "chunk") for o, n in self.ranges(k)]
        assert all(o >= 0 and n > 0 and o + n <= self.n_flat for o, n in every)
        assert all(o % 4 == 0 and n % 4 == 0 for o, n in every)
        assert all(0 < c.len <= 4096 for c in self.chunks)
        assert all(s.n % 8 == 0 for s in self.bias)
        m = self.masks
        for a, b in (("ln", "bias"), ("ln", "chunk"), ("bias", "chunk")):
            assert not bool((m[a] & m[b]).any()), (a, b)
        assert sum(int(x.sum()) for x in m.values()) == sum(n for _, n in every)          # no two slots of one category overlap
        assert all(s.b_off != s.a_off + s.d and s.a_off != s.b_off + s.d for s in self.ln)      # gain | bias not adjacent
        assert not self.ln or any(s.b_off < s.a_off for s in self.ln)
        assert bool(self.untouched.any())
        offs = [c.off for c in self.chunks]
        assert offs == sorted(offs)


def build_layout(seed, ln_widths=(), bias_sizes=(), chunk_lens=()):
    """Deal the gain and the bias of every LayerNorm, every Linear bias and every chunk to one flat buffer in a seeded random
    order with holes between all neighbours (so gains and biases of one LayerNorm are never adjacent and the chunk list leaves
    holes); the first LayerNorm has its bias BEFORE its gain.  Chunks keep their list order."""
    rng = np.random.RandomState(seed)
    items = [("a", i, d) for i, d in enumerate(ln_widths)] + [("b", i, d) for i, d in enumerate(ln_widths)]
    items += [("bias", j, n) for j, n in enumerate(bias_sizes)] + [("chunk", k, n) for k, n in enumerate(chunk_lens)]
    order = [items[i] for i in rng.permutation(len(items))]
    # chunks in list order (mtn_adam_step_chunks's callers keep them sorted); LayerNorm 0: b before a
    chunk_pos = [i for i, it in enumerate(order) if it[0] == "chunk"]
    for pos, k in zip(chunk_pos, range(len(chunk_lens))):
        order[pos] = ("chunk", k, chunk_lens[k])
    if ln_widths:
        ia, ib = order.index(("a", 0, ln_widths[0])), order.index(("b", 0, ln_widths[0]))
        if ia < ib:
            order[ia], order[ib] = order[ib], order[ia]
    a_off, b_off, bias_off, chunk_off = {}, {}, {}, {}
    cur = int(rng.choice(GAPS))
    for kind, idx, n in order:
        {"a": a_off, "b": b_off, "bias": bias_off, "chunk": chunk_off}[kind][idx] = cur
        cur += n + int(rng.choice(GAPS))
    n_flat = cur + SLACK
    return Layout(n_flat,
                  [LnSlot(d, a_off[i], b_off[i]) for i, d in enumerate(ln_widths)],
                  [BiasSlot(n, bias_off[j]) for j, n in enumerate(bias_sizes)],
                  [Chunk(chunk_off[k], n) for k, n in enumerate(chunk_lens)])


def front_units(ln_widths, n_chunks):
    """(LayerNorm units of 256 columns of [da2 | db2], front tiles after padding to a multiple of 8)"""
    units = sum((2 * d + 255) // 256 for d in ln_widths)
    return units, (units + n_chunks + 7) // 8 * 8
