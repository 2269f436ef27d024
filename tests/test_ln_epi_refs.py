"""The host references of tests/ln_epi_refs.py, checked without a GPU: the identity LayerNorm backward "by linearity" rests on
(include/mtn_hip.h, mtn_ln_epilogue), the block partials against the row sums, the partial dealer, and the derived float32 bound."""
import pytest
import torch

from tests import ln_epi_refs as R

SLICES = [(70, 64, 640, 0.1), (33, 48, 192, 0.0), (135, 512, 192, 0.1), (1, 16, 64, 0.5)]       # (rows, d, d_ff, p)


@pytest.fixture(scope="module", params=SLICES, ids=lambda s: "x".join(str(v) for v in s))
def ffn(request):
    rows, d, d_ff, p = request.param
    s = R.ffn_slice(rows, d, d_ff, p, seed=rows + d)
    s.u, s.c = R.fold64(s.w1, s.b1, s.a2, s.b2)
    return s


def _close(a, b, rel):
    return float((a - b).abs().max()) <= rel * max(1e-300, float(b.abs().max()))


def test_slice_is_consistent(ffn):
    s = ffn
    assert bool((s.dh[s.hid <= 0] == 0).all()) and bool((s.hid >= 0).all())
    live = float((s.hid > 0).double().mean())
    assert 0.3 * (1 - s.p) < live < 0.7, live                      # about half the pre-activations are positive, a share p of those dropped
    kept = s.hid > 0
    assert _close((s.hid / s.scale)[kept], s.q[kept], 1e-15)       # hid * gate_inv_scale reads q back where dh is non-zero


def test_row_sums_are_linear_in_dq(ffn):
    """S1 = dh . u and P2 = dh . (q - c) are the row sums of g = dh W1, and LayerNorm backward from them is autograd's: the identity."""
    s = ffn
    g = s.dh @ s.w1.double()
    s1, p2 = (s.dh * s.u).sum(1), (s.dh * (s.q - s.c)).sum(1)
    t1, t2 = R.row_sums64(g, s.x, s.a2, s.mean, s.rstd)
    # q - c = rstd W1 (a2 (x - mean)) is a difference of numbers of size |q|, |c|: cancellation costs a few digits, not more
    assert _close(s1, t1, 1e-12) and _close(p2, t2, 1e-11)
    dx, da2, db2 = R.consume64(g, s.x, s.a2, s.mean, s.rstd, s.eps, s.dres)
    for dres in (s.dres, None):
        want = dx if dres is not None else dx - s.dres.double()
        assert _close(R.consume64_from_sums(s1, p2, g, s.x, s.a2, s.mean, s.rstd, s.eps, dres), want, 1e-11)
        assert _close(R.consume64_from_sums(t1, t2, g, s.x, s.a2, s.mean, s.rstd, s.eps, dres), want, 1e-12)
    assert _close(db2, g.sum(0), 1e-15)
    xhat = (s.x.double() - s.mean.unsqueeze(1)) * s.rstd.unsqueeze(1)
    assert _close(da2, (g * xhat).sum(0), 1e-15)


def test_consume64_without_dres_is_plain_autograd(ffn):
    s = ffn
    g = s.dh @ s.w1.double()
    with_, _, _ = R.consume64(g, s.x, s.a2, s.mean, s.rstd, s.eps, s.dres)
    without, _, _ = R.consume64(g, s.x, s.a2, s.mean, s.rstd, s.eps, None)
    assert _close(with_ - without, s.dres.double(), 1e-12)


def test_emit_blocks_add_up_to_the_row_sums(ffn):
    s = ffn
    inv = 1.0 / s.scale
    part = R.emit64(s.dh, s.hid, inv, s.u, s.c)
    assert part.shape == (s.rows, s.d_ff // 64, 2)
    assert _close(part[:, :, 0].sum(1), (s.dh * s.u).sum(1), 1e-13)
    assert _close(part[:, :, 1].sum(1), (s.dh * (s.q - s.c)).sum(1), 1e-11)
    # a block is its own 64 columns: moving one entry moves exactly one pair
    if s.d_ff >= 128:
        v = s.dh.clone()
        v[0, 64] += 1.0
        moved = (R.emit64(v, s.hid, inv, s.u, s.c) != part).any(dim=2)
        assert int(moved.sum()) == 1 and bool(moved[0, 1])


@pytest.mark.parametrize("np_pairs", [1, 3, 10])
def test_partial_dealer_preserves_the_sums(ffn, np_pairs):
    s = ffn
    g = s.dh @ s.w1.double()
    s1, p2 = R.row_sums64(g, s.x, s.a2, s.mean, s.rstd)
    part = R.deal_partials(s1, p2, np_pairs, torch.Generator().manual_seed(np_pairs))
    assert part.shape == (s.rows, np_pairs, 2) and part.dtype == torch.float64
    scale = part.abs().sum(1)                                                      # cancellation between shares of either sign
    assert bool(((part.sum(1) - torch.stack([s1, p2], 1)).abs() <= 1e-15 * scale).all())
    if np_pairs >= 3 and s.rows >= 33:
        share = part[:, :, 0] / s1.unsqueeze(1)
        assert bool((share < 0).any()) and float(share.abs().max()) <= np_pairs


def test_emit_bound_dominates_float32_evaluation(ffn):
    """The bound against float32 arithmetic in the kernels' summation shape, on operands as the kernel sees them: v and hid bf16
    values, u, c and the inverse scale float32 values."""
    s = ffn
    v, hid = R.lp_round(s.dh.float(), R.BF16), R.lp_round(s.hid.float(), R.BF16)
    u, c, inv = s.u.float(), s.c.float(), float(torch.tensor(1.0 / s.scale, dtype=torch.float32))
    exact, bound = R.emit64(v, hid, inv, u, c), R.emit_bound(v, hid, inv, u, c)
    got = R.emit_f32(v, hid, inv, u, c)
    assert got.dtype == torch.float32 and got.shape == exact.shape == bound.shape
    err = (got.double() - exact).abs()
    assert bool((err <= bound).all()), float((err / bound.clamp_min(1e-300)).max())
    assert float(err.max()) > 0                                                      # float32 did round: the comparison is not vacuous
    # and the bound is no blanket: a few float32 ulps of the absolute sums, far below the partials themselves
    assert float((bound / exact.abs().clamp_min(1e-30)).median()) < 1e-4
