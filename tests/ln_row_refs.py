"""Host references for the direct tests of the LayerNorm row kernels and the embedding scatter (csrc/layernorm.hip: ln_fwd_small_kernel,
ln_fwd_kernel, ln_bwd_small_kernel, ln_bwd_kernel, ln_bwd_finalize_kernel, embed_bwd_kernel, embed_bwd_det_kernel;
tests/test_ln_row_kernels_gpu.py, tests/test_embed_scatter_kernel_gpu.py); validated without a GPU by tests/test_ln_row_refs.py.
Plain helpers, no fixtures, no GPU imports; numpy, float64 unless a name says otherwise.  Keep masks come from tests/dropout_refs.py.

make_case     one problem (rows, d, data class): x, g, dres [rows, d] float32, a2 = linspace(0.5, 1.5), b2 = linspace(-1, 1) (a column
              swap is an O(1) error), eps.  Classes: a N(0.3, 2) | b 1e-3 randn (std + eps and sqrt(var + eps) differ by tens of
              percent at eps = 1e-6) | c 100 + randn (cancellation) | d class a with eps = 1e-3 | e class a with one row of 0.5
              (forward only: every sum of that row is exact in float32, so mean = 0.5, std = 0, rstd = 1 / eps, y = b2, all finite).
fwd64         y, mean, rstd = 1 / (std_unbiased + eps) of a row matrix.
bwd64         dx (+ dres) by float64 autograd of oracle.mtn_oracle.layer_norm, da2 = sum_rows g (x - mean) rstd, db2 = sum_rows g, and
              the partial rows [ceil(rows / 8)][2 d] (the same sums over each block of 8 rows).
src64         the synthesised source row of ln_src: lut[tok] emb_scale + pe[row % seq_len] | x + pe[row % seq_len] | x, then
              keep / (1 - p) where a mask is given (p and emb_scale are the float32 values the descriptor carries).
handoff64     dx_lp = keep dx / (1 - p), rounded to the compute dtype.
finalize64    column sums of a partial buffer.
embed64       dlut + scatter of the streams' rows, and its bound.

THE BOUNDS.  u = 2^-24: one float32 operation (+ - * and, since the library is built without fast-math, / and sqrt too) rounds to
nearest and moves its own result by at most u relative.  A sum whose every addend passes through at most k additions, in any order
and grouping, is within k u sum |addend| of the exact sum to first order (no partial result exceeds sum |addend|).  A fused
multiply-add only removes a rounding, so where the compiler may or may not form one the unfused count stands.  All bounds are first
order in u except where said.  The remainder: in the full expansion each first-order term is multiplied by (1 + the relative
perturbations of the other quantities), and the largest such perturbation in any case here is the mean's bound against the row's
spread in class c (17 u 100 / 1 = 1e-4 at d = 2052) — below 2^-13; every bound is therefore multiplied by SECOND = 1 + 2^-12.  None
carries a margin factor.

Summation shape (forward and backward alike): lane l holds columns 4 l + 256 j .. + 3; a float4 is summed as (x + y) + (z + w), 2
additions; the lane's chain s += ... has nj = ceil(d / 256) additions (the first into 0 is exact; counted all the same); wave_sum
(common.h) is a 6-step xor butterfly, 6 additions.  A row sum is therefore K(d) = 8 + nj additions deep.

  x_out   tokens: lut s rounds (u |lut s|), + pe rounds (u |lut s + pe|); x + pe: one rounding; plain x: exact (bound 0: bit
          equality).  Under dropout the kept value is multiplied by the float32 scale 1 / (1 - p): 1 - p and the division round (2 u)
          and the product rounds (u): 3 u |x_out|, and the earlier error is scaled by 1 / (1 - p).  Dropped elements: bound 0.
          This bound bx enters everything below as an input perturbation.
  mean    K u sum |x| / d + u |mean| (the division) + mean(bx)                                                       =: bm
  rstd    q = sum (x - m)^2 around the COMPUTED mean m is sum e^2 + d (m - mean)^2 exactly: the mean's error enters std only in
          second order, but on a constant row that term is all there is, so it is kept in full:
              dstd_m = sqrt(std^2 + d / (d - 1) bm^2) - std.
          Each e_i rounds (2 u on e_i^2), the square rounds (u), the sum is K deep, / (d - 1) rounds (u): (4 + K) u relative on
          q / (d - 1); sqrt halves that and rounds once: ((4 + K) / 2 + 1) u std.  The input perturbation moves std by
          sum |e_i| bx_i / ((d - 1) std).  std + eps and 1 / (.) round: 2 u.  Altogether
              bstd = ((4 + K) / 2 + 1) u std + dstd_m + sum |e| bx / ((d - 1) std);   brstd = rstd (bstd rstd + 2 u).
  y_f32   o = a (x - m) r + b: e rounds, a e rounds, (a e) r rounds: 3 u |a e r|; + b rounds: u |y|; carried: |a| r (bx + bm) from e,
          |a e| brstd from r.       by = 3 u |a e r| + u |y| + |a| r (bx + bm) + |a e| brstd
  y_lp    float32: by.  bfloat16 (8 significant bits, round to nearest even, store_lp4): by + 2^-8 (|y| + by).
  dx      the kernel is handed float32 mean and rstd; the test hands it the float64 values rounded once, so dm = |mean32 - mean| and
          dr = |rstd32 - rstd| are known numbers, carried to first order.  Kb = 8 + nj as above.
              h = g a (u);  e = x - mu (u |e| + dm);  s1 = sum h: bs1 = (1 + Kb) u sum |h|
              s2 = sum h e: bs2 = (3 + Kb) u sum |h e| + dm |s1|
              std = 1 / r - eps: the division and the subtraction round, dr moves 1 / r by dr / r^2: bsd = u / r + u std + dr / r^2
              c1 = r s1 (1 / d): three roundings: bc1 = |c1| (3 u + dr / r) + r bs1 / d
              c2 = s2 r r / (std (d - 1)): four roundings: bc2 = |c2| (4 u + 2 dr / r + bsd / std) + r^2 bs2 / (std (d - 1))
              o = r h - c1 - c2 e + dres:  |r h| (2 u + dr / r) + bc1 + 2 u |c2 e| + |c2| dm + |e| bc2, the two subtractions
              u (|r h| + |c1|) + u (|r h| + |c1| + |c2 e|), and with dres u |dx|.
  dx_lp   v = dx scale under the mask: scale 2 u, product u: bv = bdx / (1 - p) + 3 u |v| (no mask: bv = bdx); rounding to bfloat16
          2^-8 (|v| + bv); the REFERENCE is rounded to the compute dtype too (2^-8 |v|, or u |v| for float32).
  partial each addend g e r of the gain's row: e, g e, (g e) r round (3 u), dm and dr carry (|g| r dm + |g e| dr); the bias's addend
          g is exact.  ln_bwd_small_kernel: one row per wave (0 + t), then ((w0 + w1) + (w2 + w3)) + ((w4 + w5) + (w6 + w7)) through
          LDS: 4 additions.  ln_bwd_kernel: two rows per wave, (w0 + w1) + (w2 + w3): 4 additions.  PART_ADDS = 4.
              bpa = sum_rows of the block [ (3 + 4) u |g e r| + |g| r dm + |g e| dr ];   bpb = 4 u sum_rows |g|
  da2/db2 ln_bwd_finalize_kernel deals the parts to 16 thread groups; a part passes through at most ceil(nparts / 16) additions of
          its group's chains, 2 of (s0 + s1) + (s2 + s3), and 6 of the combination of the 16 groups: FIN(nparts) = ceil(nparts / 16)
          + 8.     bda2 = sum_blocks bpa + FIN u sum_rows |g e r|;   bdb2 = sum_blocks bpb + FIN u sum_rows |g|.
          Fed synthetic partials directly: FIN u sum_parts |p|.  Finalize holds only additions, so emulate_finalize equals the kernel
          bit for bit.
  scatter an addend dx s keep / (1 - p) is at most 4 roundings away from exact (the product with emb_scale; under dropout the scale's
          2 and its product); an entry with n addends passes through at most n + EMB_W + 1 additions (its wave's chain; or, above
          EMB_HEAVY hits, the chains of eight waves, their 8 sums, and the += into the table), in any order, so the bound holds for
          the atomic kernel too:   (4 + n + EMB_W + 1) u (|dlut before| + sum |addend|).

Worst |float32 emulation - float64 reference| / bound over every case the GPU file runs (tests/test_ln_row_refs.py prints them; all
must stay below 1):
    x_out 0.704 | mean 0.131 | rstd 0.224 | y_f32 0.704 | y_lp 0.995 | dx 0.894 | dx_lp 0.873 | partial 0.99975 |
    da2 0.99973 | db2 0.168 | finalize 0.151
The ratios near 1 are no sign of a fitted bound: y_lp's bound is a bfloat16 half-ulp that a value near a rounding midpoint uses up,
and in class c (mean ~ 100) the partial rows' bound is all but the KNOWN rounding dm of the mean the kernel is handed — at rows = 1
the error of an addend g e r is exactly g r dm.

emulate_fwd / emulate_bwd / emulate_finalize   the float32 arithmetic of the kernels in their order (numpy float32, unfused); their
              keyword switches are the MUTATIONS tests/test_ln_row_refs.py requires the bounds to reject.  The small and the generic
              forward kernel perform the same operations in the same order (the generic one re-reads the row); the two backward
              kernels differ in how a block's eight rows meet in the partial row.
violations    elements of an output outside its bound (or not finite), and the worst |out - ref| / bound.  Every element is checked.
"""
from types import SimpleNamespace

import numpy as np
import torch

from oracle.mtn_oracle import layer_norm
from tests import dropout_refs as dr

U = 2.0 ** -24
BF = 2.0 ** -8
F32 = np.float32
PART_ADDS = 4
SECOND = 1 + 2.0 ** -12         # the second-order remainder of the first-order bounds (module docstring)
BWD_BLOCK = 8                  # rows per backward workgroup = rows per partial row
EMB_W, EMB_HEAVY, EMB_CH = 8, 24, 8192

FWD_D_SMALL = (4, 8, 252, 256, 260, 508, 512)
FWD_D_GENERIC = (516, 1020, 1028, 2048, 2052)
BWD_D_MAX = 2048
ROWS = (1, 3, 4, 5, 9, 17)
# about 20 (rows, d): every d, every row count (remainders 1, 3, 0, 1, 1, 1 of 4 and 1, 3, 4, 5, 1, 1 of 8), 17 rows at both kernels
PAIRS = [(1, 4), (17, 4), (3, 8), (4, 252), (5, 256), (9, 256), (17, 260), (1, 508), (3, 512), (17, 512), (4, 516), (9, 516),
         (5, 1020), (1, 1028), (17, 1028), (3, 2048), (9, 2048), (4, 2052), (17, 2052), (5, 4)]
CLASSES = "abcde"
FIN_NPARTS = (1, 15, 16, 17, 48, 49, 64, 65, 112, 113, 128, 129, 241)
FIN_D = (4, 36, 64)


def nblocks(rows):
    return (rows + BWD_BLOCK - 1) // BWD_BLOCK


def depth(d):
    """additions a row sum's addend passes through"""
    return 8 + (d + 255) // 256


def fin_depth(nparts):
    return (nparts + 15) // 16 + 8


def case_seed(rows, d, cls):
    return 1000 * rows + 7 * d + ord(cls)


def make_case(rows, d, cls, seed=None):
    g = np.random.default_rng(case_seed(rows, d, cls) if seed is None else seed)
    n = lambda: g.standard_normal((rows, d))
    if cls in "ade":
        x = 0.3 + 2.0 * n()
    elif cls == "b":
        x = 1e-3 * n()
    else:
        x = 100.0 + n()
    const_row = None
    if cls == "e":
        const_row = rows // 2
        x[const_row] = 0.5
    return SimpleNamespace(rows=rows, d=d, cls=cls, eps=float(F32(1e-3 if cls == "d" else 1e-6)), const_row=const_row,
                           x=x.astype(F32), g=n().astype(F32), dres=n().astype(F32),
                           a2=np.linspace(0.5, 1.5, d).astype(F32), b2=np.linspace(-1.0, 1.0, d).astype(F32))


def fwd_cases():
    """class e needs ordinary rows beside the constant one: not at rows = 1"""
    return [(r, d, k) for (r, d) in PAIRS for k in CLASSES if not (k == "e" and r == 1)]


def bwd_cases():
    return [(r, d, k) for (r, d) in PAIRS if d <= BWD_D_MAX for k in "abcd"]


def bwd_variant(i):
    """what the i-th backward case runs with: (dres present, hand-off dtype, hand-off dropout p or 0) — every combination occurs"""
    return i % 2 == 0, (torch.float32, torch.bfloat16)[(i // 2) % 2], (0.0, 0.1, 0.5)[i % 3]


SEED = 0x5DEECE66D1234567 & 0x7FFFFFFFFFFFFFFF        # device dropout seed of every test here (both words non-zero)
SRC_B, SRC_L = 3, 5                                   # source modes: 3 sequences of 5 positions, rows = 15
SRC_MODES = ("tokens_pe", "x_pe", "tokens_pe_noln")
SRC_D = (64, 512, 640)
SRC_P = (0.1, 0.5)
SRC_V = 11                                            # lut rows; only those a token names are finite


def src_cases():
    return [(m, d, p) for m in SRC_MODES for d in SRC_D for p in SRC_P]


def keep2d(salt, p, rows, d, per_row=False):
    """keep[row][c] = keep(row * d + c) of site `salt` under SEED; per_row: the MUTATION keep(c)"""
    if per_row:
        return np.tile(dr.keep_mask(SEED, salt, p, d), (rows, 1))
    return dr.keep_mask(SEED, salt, p, rows * d).reshape(rows, d)


def make_src(mode, d, p, seed=0):
    """One source-mode problem.  tokens_pe: lut [SRC_V, d] with NaN in the rows no token names; pe [rows, d] with NaN from row
    SRC_L on; tokens_pe_noln: the same row with no_ln = 1 (the target embedding): it goes to x_out and y unchanged.  The plain-x source
    is what every make_case problem runs."""
    rows = SRC_B * SRC_L
    g = np.random.default_rng(77 + 13 * d + int(100 * p) + seed)
    c = SimpleNamespace(mode=mode, rows=rows, d=d, p=p, salt=0x9000 + d + int(100 * p), eps=float(F32(1e-6)), seq_len=SRC_L,
                        a2=np.linspace(0.5, 1.5, d).astype(F32), b2=np.linspace(-1.0, 1.0, d).astype(F32),
                        x=None, tokens=None, lut=None, pe=None, keep=None, emb_scale=1.0, no_ln=mode == "tokens_pe_noln")
    if mode != "x_pe":
        c.tokens = g.integers(0, SRC_V, rows)
        c.tokens[:3] = (0, SRC_V - 1, 0)
        c.lut = np.full((SRC_V, d), np.nan, dtype=F32)
        used = np.unique(c.tokens)
        c.lut[used] = g.standard_normal((used.size, d)).astype(F32)
        c.emb_scale = float(F32(np.sqrt(d)))
    else:
        c.x = (0.3 + 2.0 * g.standard_normal((rows, d))).astype(F32)
    c.pe = np.full((rows, d), np.nan, dtype=F32)
    c.pe[:SRC_L] = g.standard_normal((SRC_L, d)).astype(F32)
    c.keep = keep2d(c.salt, p, rows, d)
    return c


def src_args(c, **kw):
    a = dict(x=c.x, tokens=c.tokens, lut=c.lut, emb_scale=c.emb_scale, pe=c.pe, seq_len=c.seq_len, keep=c.keep, p=c.p)
    a.update(kw)
    return a


# ------------------------------------------------------------------------------------------ float64 references
def _f(t):
    return np.asarray(t, dtype=np.float64)


def fwd64(x, a2, b2, eps):
    x = _f(x)
    d = x.shape[1]
    mean = x.sum(1) / d
    e = x - mean[:, None]
    std = np.sqrt((e * e).sum(1) / (d - 1))
    rstd = 1.0 / (std + eps)
    return _f(a2) * e * rstd[:, None] + _f(b2), mean, rstd


def bwd64(x, a2, g, eps, dres=None):
    """-> dx, da2, db2, partial [nblocks][2 d]"""
    xr = torch.from_numpy(_f(x)).clone().requires_grad_()
    a = torch.from_numpy(_f(a2))
    layer_norm(xr, a, torch.zeros_like(a), eps).backward(torch.from_numpy(_f(g)))
    dx = xr.grad.numpy()
    if dres is not None:
        dx = dx + _f(dres)
    _, mean, rstd = fwd64(x, a2, np.zeros_like(_f(a2)), eps)
    ta = _f(g) * (_f(x) - mean[:, None]) * rstd[:, None]
    rows, d = ta.shape
    part = np.zeros((nblocks(rows), 2 * d))
    for b in range(nblocks(rows)):
        part[b, :d] = ta[b * 8:b * 8 + 8].sum(0)
        part[b, d:] = _f(g)[b * 8:b * 8 + 8].sum(0)
    return dx, ta.sum(0), _f(g).sum(0), part


def src64(rows, d, x=None, tokens=None, lut=None, emb_scale=1.0, pe=None, seq_len=0, keep=None, p=0.0):
    """-> (row matrix [rows, d], bound bx).  keep: bool [rows, d] or None."""
    if tokens is not None:
        t = _f(lut)[np.asarray(tokens)] * float(F32(emb_scale))
        v, bx = t.copy(), U * np.abs(t)
    else:
        v, bx = _f(x).copy(), np.zeros((rows, d))
    if pe is not None:
        v = v + _f(pe)[np.arange(rows) % seq_len]
        bx = bx + U * np.abs(v)
        if keep is not None:
            s = 1.0 / (1.0 - float(F32(p)))
            v = np.where(keep, v * s, 0.0)
            bx = np.where(keep, bx * s + 3 * U * np.abs(v), 0.0)
    return v, SECOND * bx


def handoff64(dx, keep, p, dtype):
    """keep dx / (1 - p) rounded to the compute dtype (torch.float32 | torch.bfloat16); keep None: no dropout."""
    v = _f(dx) if keep is None else np.where(keep, _f(dx) / (1.0 - float(F32(p))), 0.0)
    return torch.from_numpy(v).to(dtype).double().numpy(), v


def finalize64(partial):
    return _f(partial).sum(0)


# ------------------------------------------------------------------------------------------ bounds
def fwd_bounds(x, bx, a2, b2, eps):
    """x: the exact row matrix, bx its input bound (0 for rows read from memory) -> dict mean, rstd, y_f32, y_bf16"""
    x, a2 = _f(x), _f(a2)
    d = x.shape[1]
    K = depth(d)
    y, mean, rstd = fwd64(x, a2, b2, eps)
    e = x - mean[:, None]
    std = 1.0 / rstd - eps
    bm = K * U * np.abs(x).sum(1) / d + U * np.abs(mean) + bx.sum(1) / d
    dstd_m = np.sqrt(std * std + d / (d - 1.0) * bm * bm) - std
    with np.errstate(divide="ignore", invalid="ignore"):
        dstd_x = np.where(std > 0, (np.abs(e) * bx).sum(1) / ((d - 1) * std), np.sqrt((bx * bx).sum(1) / (d - 1)))
    bstd = ((4 + K) / 2.0 + 1) * U * std + dstd_m + dstd_x
    brstd = rstd * (bstd * rstd + 2 * U)
    r = rstd[:, None]
    by = 3 * U * np.abs(a2 * e * r) + U * np.abs(y) + np.abs(a2) * r * (bx + bm[:, None]) + np.abs(a2 * e) * brstd[:, None]
    bm, brstd, by = SECOND * bm, SECOND * brstd, SECOND * by
    return dict(mean=bm, rstd=brstd, y_f32=by, y_bf16=by + BF * (np.abs(y) + by))


def bwd_bounds(x, a2, g, eps, mean32, rstd32, has_dres, dx_ref):
    """-> dict dx, partial, da2, db2 (mean32 / rstd32: the float32 statistics the kernel is handed)"""
    x, a2, g = _f(x), _f(a2), _f(g)
    rows, d = x.shape
    Kb = depth(d)
    _, mean, rstd = fwd64(x, a2, np.zeros(d), eps)
    dm, drr = np.abs(_f(mean32) - mean)[:, None], np.abs(_f(rstd32) - rstd)[:, None]
    r, e, h = rstd[:, None], x - mean[:, None], g * a2
    std = 1.0 / r - eps
    s1, s2 = h.sum(1, keepdims=True), (h * e).sum(1, keepdims=True)
    bs1 = (1 + Kb) * U * np.abs(h).sum(1, keepdims=True)
    bs2 = (3 + Kb) * U * np.abs(h * e).sum(1, keepdims=True) + dm * np.abs(s1)
    bsd = U / r + U * std + drr / (r * r)
    c1, c2 = r * s1 / d, s2 * r * r / (std * (d - 1))
    bc1 = np.abs(c1) * (3 * U + drr / r) + r * bs1 / d
    bc2 = np.abs(c2) * (4 * U + 2 * drr / r + bsd / std) + r * r * bs2 / (std * (d - 1))
    rh, c2e = np.abs(r * h), np.abs(c2 * e)
    bdx = rh * (2 * U + drr / r) + bc1 + 2 * U * c2e + np.abs(c2) * dm + np.abs(e) * bc2 + U * (rh + np.abs(c1)) + U * (rh + np.abs(c1) + c2e)
    if has_dres:
        bdx = bdx + U * np.abs(dx_ref)
    ta = np.abs(g * e * r)
    ba_row = (3 + PART_ADDS) * U * ta + np.abs(g) * r * dm + np.abs(g * e) * drr
    bb_row = PART_ADDS * U * np.abs(g)
    nb = nblocks(rows)
    bpart = np.zeros((nb, 2 * d))
    for b in range(nb):
        bpart[b, :d] = ba_row[b * 8:b * 8 + 8].sum(0)
        bpart[b, d:] = bb_row[b * 8:b * 8 + 8].sum(0)
    F = fin_depth(nb)
    return dict(dx=SECOND * bdx, partial=SECOND * bpart, da2=SECOND * (bpart[:, :d].sum(0) + F * U * ta.sum(0)),
                db2=SECOND * (bpart[:, d:].sum(0) + F * U * np.abs(g).sum(0)))


def handoff_bound(v, bdx, keep, p, dtype):
    """v: the unrounded float64 hand-off value -> bound on |kernel - reference rounded to dtype|"""
    bv = bdx if keep is None else np.where(keep, bdx / (1.0 - float(F32(p))) + 3 * U * np.abs(v), 0.0)
    if dtype == torch.bfloat16:
        return bv + BF * (np.abs(v) + bv) + BF * np.abs(v)
    return bv + U * np.abs(v)


def finalize_bound(partial):
    p = _f(partial)
    return SECOND * fin_depth(p.shape[0]) * U * np.abs(p).sum(0)


def embed64(dlut0, streams):
    """streams: dicts tokens [rows], dx [rows, d] float32, emb_scale, keep (bool [rows, d] or None), p -> (ref, bound, hits [V])"""
    ref = _f(dlut0).copy()
    mag = np.abs(ref)
    hits = np.zeros(ref.shape[0], dtype=np.int64)
    for s in streams:
        v = _f(s["dx"]) * float(F32(s["emb_scale"]))
        if s.get("keep") is not None:
            v = np.where(s["keep"], v / (1.0 - float(F32(s["p"]))), 0.0)
        tok = np.asarray(s["tokens"])
        np.add.at(ref, tok, v)
        np.add.at(mag, tok, np.abs(v))
        np.add.at(hits, tok, 1)
    return ref, SECOND * (4 + hits + EMB_W + 1)[:, None] * U * mag, hits


# ------------------------------------------------------------------------------------------ float32 emulation
_LANES = np.arange(64)


def _wave_sum(s):
    """common.h wave_sum: v += shfl_xor(v, o) for o = 32 .. 1; s [rows, 64] float32 -> [rows]"""
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, _LANES ^ o]
    return s[:, 0]


def _lanes(t, d):
    """[rows, d] -> [rows, nj, 64, 4] with column 256 j + 4 lane + k, zero padded; and the validity mask [nj, 64]"""
    rows = t.shape[0]
    nj = (d + 255) // 256
    p = np.zeros((rows, nj * 256), dtype=F32)
    p[:, :d] = t
    return p.reshape(rows, nj, 64, 4), (np.arange(nj * 256).reshape(nj, 64, 4)[:, :, 0] < d)


def _row_sum(t4):
    """lane chain s += (x + y) + (z + w) over j, then the butterfly; t4 [rows, nj, 64, 4] float32 (zeros where no column is)"""
    s = np.zeros((t4.shape[0], 64), dtype=F32)
    for j in range(t4.shape[1]):
        s = s + ((t4[:, j, :, 0] + t4[:, j, :, 1]) + (t4[:, j, :, 2] + t4[:, j, :, 3]))
    return _wave_sum(s)


def emulate_src(rows, d, x=None, tokens=None, lut=None, emb_scale=1.0, pe=None, seq_len=0, keep=None, p=0.0,
                pe_by_row=False, scale_after_pe=False):
    """ln_src in float32.  Mutations: pe_by_row (pe[row] for pe[row % seq_len]), scale_after_pe; a per-row dropout index is a
    different `keep` and is made by the caller."""
    es = F32(emb_scale)
    v = np.asarray(lut, dtype=F32)[np.asarray(tokens)] if tokens is not None else np.asarray(x, dtype=F32).copy()
    if tokens is not None and not scale_after_pe:
        v = v * es
    if pe is not None:
        idx = np.arange(rows) if pe_by_row else np.arange(rows) % seq_len
        v = v + np.asarray(pe, dtype=F32)[idx]
        if tokens is not None and scale_after_pe:
            v = v * es
        if keep is not None:
            v = np.where(keep, v * dr.scale(p), F32(0.0)).astype(F32)
    return v.astype(F32)


def emulate_fwd(v, a2, b2, eps, no_ln=False, biased=False, eps_in_sqrt=False, rstd_no_eps=False, mean_skip_last4=False, swap_a2=False):
    """v: the (synthesised) row matrix, float32 -> dict mean, rstd, y (float32; bfloat16 is one torch rounding of y)"""
    v = np.asarray(v, dtype=F32)
    rows, d = v.shape
    if no_ln:
        return dict(mean=None, rstd=None, y=v.copy())
    a2, b2, eps = np.asarray(a2, dtype=F32), np.asarray(b2, dtype=F32), F32(eps)
    if swap_a2:
        a2 = a2.copy()
        a2[[0, d - 1]] = a2[[d - 1, 0]]
    v4, valid = _lanes(v, d)
    s4 = v4
    if mean_skip_last4:
        s4 = v4.copy().reshape(rows, -1)
        s4[:, d - 4:d] = 0
        s4 = s4.reshape(v4.shape)
    mean = _row_sum(s4) / F32(d)
    e4 = np.where(valid[None, :, :, None], v4 - mean[:, None, None, None], F32(0.0)).astype(F32)
    q = _row_sum(e4 * e4) / F32(d if biased else d - 1)
    if eps_in_sqrt:
        rstd = F32(1.0) / np.sqrt(q + eps)
    else:
        rstd = F32(1.0) / (np.sqrt(q) + eps)
    y = (a2 * (v - mean[:, None])) * rstd[:, None] + b2
    out_rstd = F32(1.0) / np.sqrt(q) if rstd_no_eps else rstd
    return dict(mean=mean.astype(F32), rstd=out_rstd.astype(F32), y=y.astype(F32))


def emulate_bwd(x, a2, g, eps, mean32, rstd32, dres=None, generic=False, lp=None, drop_dres=False, c1_dm1=False, c2_d=False,
                std_no_eps=False, da2_no_rstd=False, clamp_counted=False, lp_before_dres=False):
    """ln_bwd_small_kernel (generic = False) / ln_bwd_kernel in float32 -> dict dx, partial [nblocks][2 d], dx_lp (float32 values of
    the hand-off copy; lp = dict(keep, p, dtype) or None)."""
    x, a2, g = np.asarray(x, dtype=F32), np.asarray(a2, dtype=F32), np.asarray(g, dtype=F32)
    rows, d = x.shape
    mu, r = np.asarray(mean32, dtype=F32)[:, None], np.asarray(rstd32, dtype=F32)[:, None]
    eps = F32(eps)
    std = np.maximum(F32(1.0) / r - (F32(0.0) if std_no_eps else eps), F32(1e-30))
    h, e = g * a2, x - mu
    h4, _ = _lanes(h, d)
    he4, _ = _lanes(h * e, d)
    s1, s2 = _row_sum(h4)[:, None], _row_sum(he4)[:, None]
    c1 = r * s1 * (F32(1.0) / F32(d - 1 if c1_dm1 else d))
    c2 = s2 * r * r / (std * F32(d if c2_d else d - 1))
    o = r * h - c1 - c2 * e
    pre = o
    if dres is not None and not drop_dres:
        o = o + np.asarray(dres, dtype=F32)
    out = dict(dx=o.astype(F32))
    if lp is not None:
        w = pre if lp_before_dres else o
        if lp.get("keep") is not None:
            w = np.where(lp["keep"], w * dr.scale(lp["p"]), F32(0.0)).astype(F32)
        out["dx_lp"] = torch.from_numpy(np.ascontiguousarray(w, dtype=F32)).to(lp["dtype"])
    ta = g * e if da2_no_rstd else g * e * r
    nb = nblocks(rows)
    part = np.zeros((nb, 2 * d), dtype=F32)
    for b in range(nb):
        w = []                                               # the eight rows' addends (gain | bias), zero where no row is
        for k in range(8):
            row = b * 8 + k
            if row < rows:
                w.append(np.concatenate([ta[row], g[row]]))
            elif clamp_counted:
                w.append(np.concatenate([ta[rows - 1], g[rows - 1]]))
            else:
                w.append(np.zeros(2 * d, dtype=F32))
        z = np.zeros(2 * d, dtype=F32)
        if generic:
            w = [(z + w[2 * i]) + w[2 * i + 1] for i in range(4)]
            part[b] = (w[0] + w[1]) + (w[2] + w[3])
        else:
            w = [z + t for t in w]
            part[b] = ((w[0] + w[1]) + (w[2] + w[3])) + ((w[4] + w[5]) + (w[6] + w[7]))
    out["partial"] = part
    return out


def emulate_finalize(partial, drop_tail=False, late64=False):
    """ln_bwd_finalize_kernel in its order -> [2 d] float32, bit-identical with the kernel.  Mutations: drop_tail (no 16-step tail
    loop), late64 (the 64-step loop starts one part of the thread group late)."""
    p = np.asarray(partial, dtype=F32)
    n, w = p.shape
    red = np.zeros((16, w), dtype=F32)
    for q in range(16):
        s = [np.zeros(w, dtype=F32) for _ in range(4)]
        i = q
        while i + 112 < n:
            for k in range(8):
                s[k % 4] = s[k % 4] + p[i + 16 * k]
            i += 128
        if late64:
            i += 16
        while i + 48 < n:
            for k in range(4):
                s[k] = s[k] + p[i + 16 * k]
            i += 64
        while i < n and not drop_tail:
            s[0] = s[0] + p[i]
            i += 16
        red[q] = (s[0] + s[1]) + (s[2] + s[3])
    t = np.zeros(w, dtype=F32)
    for k in range(0, 16, 4):
        t = t + ((red[k] + red[k + 1]) + (red[k + 2] + red[k + 3]))
    return t


def make_partials(nparts, d, seed):
    """a synthetic partial buffer [nparts][2 d]: N(0, 1) on a column ramp linspace(0.5, 1.5)"""
    g = np.random.default_rng(seed)
    return (g.standard_normal((nparts, 2 * d)) * np.linspace(0.5, 1.5, 2 * d)).astype(F32)


# ------------------------------------------------------------------------------------------ comparison
def violations(out, ref, bound):
    """-> (elements outside the bound or not finite, worst |out - ref| / bound over the finite ones; 0 / 0 counts as 0).  Every
    element is looked at."""
    if isinstance(out, torch.Tensor):
        out = out.detach().double().cpu().numpy()
    out, ref, bound = _f(out), _f(ref), _f(bound)
    assert out.shape == ref.shape == bound.shape, (out.shape, ref.shape, bound.shape)
    err = np.abs(out - ref)
    fin = np.isfinite(out)
    bad = ~fin | ~(err <= bound)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(fin & (err > 0), err / bound, 0.0)
    return int(bad.sum()), float(ratio.max()) if ratio.size else 0.0


def assert_within(out, ref, bound, what):
    n, worst = violations(out, ref, bound)
    assert n == 0, f"{what}: {n} of {np.size(ref)} elements outside the bound, worst |out - ref| / bound = {worst:.3g}"
    return worst
