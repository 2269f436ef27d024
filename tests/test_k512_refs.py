"""The host references of tests/k512_refs.py, checked without a GPU: the case builder, the float32 emulation of the kernels' arithmetic
against the derived bound at every shape the GPU tests use, and — a reference that cannot be failed is not accepted — five mutations of
that arithmetic, each of which the bound must reject."""
import pytest
import torch

from tests import k512_refs as R

ALL_SHAPES = sorted({s for group in R.CASES.values() for s in group} | {R.QUEUE_SHAPE} | set(R.FORMS))
# the mutation cases: with a bias, from one row to three row tiles
MUTATION_SHAPES = [s for s in ALL_SHAPES if s[5] and s[0] <= 384]
_id = lambda s: "x".join(str(int(v)) for v in s)


@pytest.fixture(scope="module")
def cases():
    cache = {}

    def get(shape):
        if shape not in cache:
            cache[shape] = R.with_refs(R.make_case(shape, seed=ALL_SHAPES.index(shape)))
        return cache[shape]
    return get


def test_case_tables_cover_the_edges():
    flat = [s for group in R.CASES.values() for s in group]
    assert {s[0] for s in flat} >= {1, 16, 127, 128, 129, 257, 384}
    assert {s[1] for s in flat} == {256, 512, 768} and {s[2] for s in flat} == {512, 520, 1024} and {s[3] for s in flat} == {512, 528}
    for rel in (lambda n: n, lambda n: n + 8, lambda n: 2 * n):
        assert any(s[4] == rel(s[1]) for s in flat)
    assert {s[5] for s in flat} == {True, False}
    assert any(s[0] == 384 and s[1] == 768 for s in flat)                       # three row tiles x three column tiles
    assert max(s[0] for s in flat) <= 384 and len(R.CASES) >= 1 and all(len(g) >= 2 for g in R.CASES.values())
    assert R.tiles([R.QUEUE_SHAPE], 256) == 1
    # the set of the three forms: every N fills wide tiles; the 128 x 128 count is the smallest from the 512-tile minimum on (it is even:
    # every N is a multiple of 256) at which the three forms' workgroup counts are pairwise distinct, so that the census tells them apart
    f = R.FORMS
    assert all(s[1] % 256 == 0 for s in f) and R.tiles(f, 128) == 514 and R.tiles(f, 256) == 257
    assert len({R.tiles(f, 128), R.tiles(f, 256), R.PERSISTENT_GRID}) == 3
    assert {s[1] for s in f} == {256, 768, 1024}
    assert any(s[0] % 64 for s in f) and any(s[0] < 8 for s in f) and any(s[2] > 512 for s in f) and any(s[4] > s[1] for s in f)
    assert any(not s[5] for s in f)


def test_case_builder(cases):
    c = cases((129, 512, 520, 528, 1024, True))
    assert c.x.dtype == c.w.dtype == torch.bfloat16 and c.bias.dtype == torch.float32
    assert c.x.shape == (129, 520) and c.w.shape == (512, 528) and c.bias.shape == (512,)
    assert bool(torch.isnan(c.x[:, 512:]).all()) and bool(torch.isnan(c.w[:, 512:]).all())
    assert bool(torch.isfinite(c.x[:, :512]).all()) and bool(torch.isfinite(c.w[:, :512]).all())
    # the ramps: the last rows are three times the first in scale
    rms = lambda t: t.double().pow(2).mean(1).sqrt()
    assert 2.5 < float(rms(c.x[-8:, :512]).mean() / rms(c.x[:8, :512]).mean()) < 3.5
    assert 2.5 < float(rms(c.w[-32:, :512]).mean() / rms(c.w[:32, :512]).mean()) < 3.5
    assert bool(torch.isfinite(c.ref).all()) and bool((c.bound > 0).all())
    assert cases((16, 256, 520, 528, 264, False)).bias is None


@pytest.mark.parametrize("shape", ALL_SHAPES, ids=_id)
def test_emulation_is_inside_the_bound(cases, shape):
    c = cases(shape)
    n, worst = R.violations(R.emulate(c), c.ref, c.bound)
    assert n == 0 and 0.0 < worst <= 1.0, (n, worst)


@pytest.mark.parametrize("shape", MUTATION_SHAPES, ids=_id)
def test_bound_rejects_every_mutation(cases, shape):
    c = cases(shape)
    good = R.emulate(c)
    swapped = good.clone()
    swapped[:, [4, 5]] = good[:, [5, 4]]
    mutants = dict(last_step_dropped=R.emulate(c, drop_last_step=True), first_product_dropped=R.emulate(c, drop_product=0),
                   product_300_dropped=R.emulate(c, drop_product=300), bias_dropped=R.emulate(c, drop_bias=True), columns_swapped=swapped)
    for name, out in mutants.items():
        n, worst = R.violations(out, c.ref, c.bound)
        assert n >= 1 and worst > 1.0, (name, n, worst)


@pytest.mark.parametrize("shape", MUTATION_SHAPES, ids=_id)
def test_bound_rejects_truncation(cases, shape):
    """Truncation errs by up to a whole unit in the last place, rounding by half of one: of a few hundred elements some lose more than
    the bound allows."""
    c = cases(shape)
    out = R.emulate(c, truncate=True)
    assert bool((out.double().abs() <= R.emulate(c).double().abs()).all())
    n, worst = R.violations(out, c.ref, c.bound)
    assert n >= 1 and worst > 1.0, (n, worst)


def test_violations_counts_non_finite_elements(cases):
    c = cases(R.QUEUE_SHAPE)
    out = R.emulate(c)
    out[3, 7] = float("nan")
    out[0, 0] = float("inf")
    assert R.violations(out, c.ref, c.bound)[0] == 2
    with pytest.raises(AssertionError):
        R.assert_within(out, c, "poisoned")
