"""Host references for the direct tests of LayerNorm backward "by linearity" (include/mtn_hip.h mtn_ln_epilogue: mtn_ln_fold, the
MTN_LN_EMIT and MTN_LN_CONSUME epilogues of mtn_gemm; tests/test_ln_epilogue_kernel_gpu.py); validated without a GPU by
tests/test_ln_epi_refs.py.  Plain helpers, no fixtures; everything is float64 unless its name says otherwise.

fold64               u = W a2, c = bias + W b2 of a Linear W [K, d] behind a LayerNorm (a2, b2).
consume64            what the consume epilogue must deliver: dx = float64 autograd of the oracle's layer_norm (+ dres),
                     da2 = sum_rows g (x - mean) rstd, db2 = sum_rows g.
row_sums64           the two row sums the epilogue is handed: S1 = sum_c a2 g, P2 = rstd sum_c a2 (x - mean) g.
consume64_from_sums  dx by the header's formula, given S1 and P2 (however they were obtained):
                         dx = rstd a2 g - rstd S1 / d - P2 rstd / (std (d - 1)) (x - mean) + dres,   std = 1 / rstd - eps.
emit64               part[M][N / 64][2]: over each 64-column block, pair 0 = sum v u, pair 1 = sum v (hid inv - c).
emit_f32             the same sums with IEEE float32 operations in the summation SHAPE of the emit kernels (see emit_bound).
emit_bound           a DERIVED first-order bound on |float32 partial - exact partial|.  Every emit kernel instance (64 x 64 tile on
                     8 or 16 waves, full or half stages) has four waves across the tile's 64 columns, each lane holding 4 consecutive
                     columns of one row.  An addend v_k u_k of pair 0 passes through
                         1  product
                         4  additions of the lane's chain p1 += v u (the first, into 0, is exact; counted all the same)
                         2  additions of fh_cross_sum (the four lane groups of a wave, pairwise)
                         4  additions across the four waves through LDS (again the first is into 0)
                     = EMIT_OPS[0] = 11 roundings, each at most 2^-24 relative to its own result, and no partial result exceeds
                     sum_k |v_k| |u_k|:   bound0 = 11 * 2^-24 * sum_k |v_k| |u_k|.
                     Pair 1 has two more per addend (hid * inv, then - c; |hid inv - c| <= |hid inv| + |c|):
                         bound1 = EMIT_OPS[1] * 2^-24 * sum_k |v_k| (|hid_k inv| + |c_k|),  EMIT_OPS[1] = 13.
                     A fused multiply-add only removes roundings.  v, hid (bf16 values), u, c, inv (float32 values) enter exactly.
deal_partials        splits each row sum into np addends in random proportions, some of them negative; the sum is preserved.
ffn_slice            a CONSISTENT feed-forward slice: q = W1 LN(x) + b1, hid = relu(q) mask / (1 - p), dh = (dy W2) gated by hid —
                     the only data on which the identity S1 = dh . u, P2 = dh . (q - c) holds.
"""
from types import SimpleNamespace

import numpy as np
import torch

from oracle.mtn_oracle import layer_norm
from tests.util import lp_round

EMIT_OPS = (11, 13)
BF16 = torch.bfloat16


def _d(t):
    return torch.as_tensor(t).detach().cpu().double()


def fold64(w_bf16, bias, a2, b2):
    """W [K, d] (bf16 values), bias [K] or None, a2 / b2 [d] -> (u [K], c [K])."""
    w = _d(w_bf16)
    u = w @ _d(a2)
    c = w @ _d(b2)
    return u, (c if bias is None else c + _d(bias))


def row_stats64(x, eps):
    """mean, rstd = 1 / (unbiased std + eps) per row; d = 1 has no unbiased std and is not a LayerNorm width."""
    x = _d(x)
    return x.mean(1), 1.0 / (x.std(1, unbiased=True) + eps)


def row_sums64(g, x, a2, mean, rstd):
    g, x, a2 = _d(g), _d(x), _d(a2)
    s1 = (a2 * g).sum(1)
    p2 = _d(rstd) * (a2 * (x - _d(mean).unsqueeze(1)) * g).sum(1)
    return s1, p2


def consume64(g, x, a2, mean, rstd, eps, dres):
    g, a2 = _d(g), _d(a2)
    xr = _d(x).clone().requires_grad_()
    layer_norm(xr, a2, torch.zeros_like(a2), eps).backward(g)
    dx = xr.grad if dres is None else xr.grad + _d(dres)
    xc = _d(x) - _d(mean).unsqueeze(1)
    return dx, (g * xc * _d(rstd).unsqueeze(1)).sum(0), g.sum(0)


def consume64_from_sums(s1, p2, g, x, a2, mean, rstd, eps, dres):
    g, x, a2 = _d(g), _d(x), _d(a2)
    r = _d(rstd).unsqueeze(1)
    d = x.size(1)
    std = 1.0 / r - eps
    dx = r * a2 * g - r * _d(s1).unsqueeze(1) / d - _d(p2).unsqueeze(1) * r / (std * (d - 1)) * (x - _d(mean).unsqueeze(1))
    return dx if dres is None else dx + _d(dres)


def _blocks(t):
    m, n = t.shape
    assert n % 64 == 0
    return t.reshape(m, n // 64, 64)


def emit64(v_stored, hid, gate_inv_scale, u, c):
    v, hid = _d(v_stored), _d(hid)
    p0 = _blocks(v * _d(u)).sum(2)
    p1 = _blocks(v * (hid * float(gate_inv_scale) - _d(c))).sum(2)
    return torch.stack([p0, p1], dim=2)


def emit_bound(v_stored, hid, gate_inv_scale, u, c):
    """[M][N / 64][2]: EMIT_OPS[pair] * 2^-24 * sum over the block of |v| |u|, resp. |v| (|hid inv| + |c|); the count of 11 / 13
    roundings per addend is derived in the module docstring."""
    v, hid = _d(v_stored).abs(), _d(hid).abs()
    b0 = _blocks(v * _d(u).abs()).sum(2)
    b1 = _blocks(v * (hid * abs(float(gate_inv_scale)) + _d(c).abs())).sum(2)
    return torch.stack([EMIT_OPS[0] * b0, EMIT_OPS[1] * b1], dim=2) * 2.0 ** -24


def emit_f32(v_stored, hid, gate_inv_scale, u, c):
    """float32 [M][N / 64][2]: numpy float32 arithmetic (every operation rounded, no fused multiply-add) in the shape of the emit
    kernels: per lane a chain over 4 consecutive columns, the 4 lane groups of a wave pairwise, the 4 waves of a block in order."""
    f = lambda t: torch.as_tensor(t).detach().cpu().float().numpy()
    v, hid, u, c, inv = f(v_stored), f(hid), f(u), f(c), np.float32(gate_inv_scale)
    m, n = v.shape
    out = np.zeros((m, n // 64, 2), np.float32)
    for pair, term in ((0, np.broadcast_to(u, v.shape)), (1, hid * inv - c)):
        assert term.dtype == np.float32
        prod = (v * term).reshape(m, n // 64, 4, 4, 4)                # [row][block][wave][lane group][column of the lane]
        lane = np.zeros(prod.shape[:-1], np.float32)
        for k in range(4):
            lane = lane + prod[..., k]
        wave = (lane[..., 0] + lane[..., 1]) + (lane[..., 2] + lane[..., 3])
        s = np.zeros(wave.shape[:-1], np.float32)
        for w in range(4):
            s = s + wave[..., w]
        assert s.dtype == np.float32
        out[..., pair] = s
    return torch.from_numpy(out)


def deal_partials(s1, p2, np_pairs, gen):
    """[M] , [M] -> float64 [M][np][2].  The first np - 1 shares are uniform in [-0.5, 1), the last takes the rest: their sum is 1
    whatever its sign, and no share exceeds np in size (what the float32 copy handed to the kernel then costs: np * 2^-24)."""
    s1, p2 = _d(s1), _d(p2)
    m = s1.numel()
    out = []
    for s in (s1, p2):
        share = torch.rand(m, np_pairs, generator=gen, dtype=torch.float64) * 1.5 - 0.5
        share[:, -1] = 1.0 - share[:, :-1].sum(1)
        out.append(s.unsqueeze(1) * share)
    return torch.stack(out, dim=2).contiguous()


def ffn_slice(rows, d, d_ff, p, seed, eps=1e-6):
    """Inputs as the kernels get them (x, a2, b2, b1, dres float32; w1 [d_ff, d], w2 [d, d_ff], dy bf16 values) and, in float64 from
    exactly those, mean, rstd, q, hid and dh.  `keep` is a plain Bernoulli mask: hid carries it, no kernel draws it."""
    gen = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=gen)
    x = rn(rows, d) * 2 + 0.3
    a2, b2 = 1 + 0.3 * rn(d), 0.2 * rn(d)
    w1, b1 = lp_round(rn(d_ff, d) * d ** -0.5, BF16), 0.1 * rn(d_ff)
    w2 = lp_round(rn(d, d_ff) * d_ff ** -0.5, BF16)
    dy, dres = lp_round(rn(rows, d), BF16), rn(rows, d)
    keep = torch.rand(rows, d_ff, generator=gen) >= p
    mean, rstd = row_stats64(x, eps)
    ln = _d(a2) * (_d(x) - mean.unsqueeze(1)) * rstd.unsqueeze(1) + _d(b2)
    q = ln @ _d(w1).t() + _d(b1)
    scale = 1.0 / (1.0 - p)
    hid = torch.relu(q) * keep.double() * scale
    dh = torch.where(hid > 0, (_d(dy) @ _d(w2)) * scale, torch.zeros_like(hid))
    return SimpleNamespace(rows=rows, d=d, d_ff=d_ff, p=p, eps=eps, scale=scale, x=x, a2=a2, b2=b2, w1=w1, b1=b1, w2=w2, dy=dy, dres=dres,
                           keep=keep, mean=mean, rstd=rstd, q=q, hid=hid, dh=dh)
