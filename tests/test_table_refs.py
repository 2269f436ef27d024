"""The host references of tests/test_table_aux_gpu.py (tests/table_refs.py) checked without a GPU: the float32 emulation of
ln_bwd_finalize_kernel's summation order stays inside its derived bound, depends on its order (so the bitwise GPU check can fail),
and the flat-buffer layouts the GPU tests use are what they claim to be."""
import pytest
import torch

from tests import table_refs as tr
from tests.test_row_kernels_gpu import CHUNK_LENS


@pytest.mark.parametrize("nparts", tr.NPARTS)
def test_finalize_f32_stays_inside_the_derived_bound(nparts):
    x = tr.partials(nparts, tr.REF_COLS, 100 + nparts)
    got, ref, bound = tr.finalize_f32(x), tr.finalize_f64(x), tr.finalize_bound(x)
    assert got.dtype == torch.float32 and got.shape == (tr.REF_COLS,)
    frac = float(((got.double() - ref).abs() / bound).max())
    print(f"nparts {nparts}: worst |f32 - f64| / bound = {frac:.3f}")
    assert frac <= 1.0
    assert float((ref - x.double().sum(0)).abs().max()) <= 1e-12 * float(x.double().abs().sum(0).max())
    if nparts == 1:
        assert torch.equal(got, x[0])                      # 0 + x is exact


def test_finalize_f32_counts_every_row_once():
    """Integer-valued rows sum exactly in any order: every row is taken, none twice, for every way through the three loops."""
    for nparts in range(1, 300):
        x = torch.arange(1, nparts + 1, dtype=torch.float32).view(-1, 1).repeat(1, 3)
        x[:, 1] *= 2
        assert tr.finalize_f32(x).tolist() == [nparts * (nparts + 1) / 2 * k for k in (1, 2, 1)], nparts


@pytest.mark.parametrize("nparts", [n for n in tr.NPARTS if n >= 65])
def test_finalize_f32_depends_on_its_order(nparts):
    x = tr.partials(nparts, tr.REF_COLS, 100 + nparts)
    a, b = tr.finalize_f32(x), tr.index_order_f32(x)
    assert not torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert bool(((b.double() - tr.finalize_f64(x)).abs() <= nparts * 2.0 ** -24 * x.double().abs().sum(0)).all())


def test_finalize_depth_is_the_longest_chain():
    """Count the additions on the way of every row through the emulation's order, symbolically: chain length + 2 + 2 + 4."""
    for n in (1, 16, 17, 49, 64, 65, 113, 128, 129, 300, 513, 4096):
        worst = 0
        for q in range(min(16, n)):
            s = [0, 0, 0, 0]
            i = q
            while i + 112 < n:
                for k in range(8):
                    s[k & 3] += 1
                i += 128
            while i + 48 < n:
                for k in range(4):
                    s[k] += 1
                i += 64
            while i < n:
                s[0] += 1
                i += 16
            worst = max(worst, max(s))
        assert worst + 8 <= tr.finalize_depth(n), (n, worst)


LAYOUTS = [dict(ln_widths=(8, 96, 136, 512, 640)), dict(chunk_lens=tuple(CHUNK_LENS), ln_widths=(136,)),
           dict(bias_sizes=(8, 200, 384, 128)), dict(ln_widths=(136, 8, 512), bias_sizes=(200, 8), chunk_lens=tuple(CHUNK_LENS[:6])),
           dict(chunk_lens=tuple(tr.MANY_CHUNKS), ln_widths=(640,))]


@pytest.mark.parametrize("seed", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("spec", LAYOUTS, ids=["ln", "chunks", "bias", "all", "many_chunks"])
def test_layouts_are_disjoint_aligned_and_inside(spec, seed):
    lay = tr.build_layout(seed, **spec)
    lay.check()
    m = lay.masks
    total = sum(int(x.sum()) for x in m.values()) + int(lay.untouched.sum())
    assert total == lay.n_flat and all(x.numel() == lay.n_flat for x in m.values())
    assert not bool((m["ln"] & m["bias"]).any() or (m["ln"] & m["chunk"]).any() or (m["bias"] & m["chunk"]).any())
    for c in lay.chunks:
        assert 0 < c.len <= 4096 and c.len % 4 == 0 and c.off % 4 == 0 and c.off + c.len <= lay.n_flat
    assert [c.len for c in lay.chunks] == list(spec.get("chunk_lens", ()))
    assert [s.d for s in lay.ln] == list(spec.get("ln_widths", ())) and [s.n for s in lay.bias] == list(spec.get("bias_sizes", ()))
    for s in lay.ln:
        assert s.a_off + s.d <= lay.n_flat and s.b_off + s.d <= lay.n_flat and abs(s.a_off - s.b_off) > s.d
    if lay.ln:
        assert lay.ln[0].b_off < lay.ln[0].a_off
    if len(lay.chunks) > 1:                                  # holes between the chunks, slack behind the last
        ends = [c.off + c.len for c in lay.chunks]
        assert all(nxt.off > end for nxt, end in zip(lay.chunks[1:], ends))
        assert lay.n_flat - max(ends) >= tr.SLACK
    assert bool(lay.untouched[-tr.SLACK:].all())


def test_front_unit_counts():
    assert tr.front_units((8, 96, 136, 512, 640), 0) == (1 + 1 + 2 + 4 + 5, 16)
    assert tr.front_units((), 20) == (0, 24)
    assert tr.front_units((136,), 14) == (2, 16)
    assert tr.front_units((640,), len(tr.MANY_CHUNKS)) == (5, 2048) and len(tr.MANY_CHUNKS) == 2040
