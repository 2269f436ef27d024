"""mtn_grad_sumsq + mtn_clip_scale (csrc/gradnorm.hip) against tests/clip_refs.py on the cases that file lists: sizes around every path
of the kernel (below one vector, the scalar tail, more than one workgroup, the two sizes around the grid cap — the smallest at which some
threads loop twice and others once — and 3 * 2^20 + 7), N(0, 1) times 1, 1e-25 and 1e25, zeros, one NaN, one inf.
  * the norm lies within RELATIVE 1e-12 of math.fsum: derived, not measured — at these sizes a thread's chain plus the two reduction
    trees is under a hundred double additions, each within 2^-53, about 1e-14;
  * the scale is within one float32 ulp of the reference, and exactly the base's bits when not clipping;
  * the stats block over a sequence of calls; two launches give identical bytes; nothing is written outside what the header names."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import clip_refs as R

pytestmark = pytest.mark.gpu
GUARD = 8                                               # doubles behind the partials that must stay as they were


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


def _launch(x, max_norm, base=None, stats=None, alias=False):
    """One mtn_grad_sumsq + mtn_clip_scale over the device buffer x.  Returns (partial incl. guard, scale, norm) device tensors."""
    from mtn_amd import lib as L
    h = L.load()
    n, dev = x.numel(), x.device
    npart = h.mtn_grad_sumsq_partials(n)
    assert npart == R.partials(n)
    partial = torch.full((npart + GUARD,), -7.0, device=dev, dtype=torch.float64)
    norm = torch.full((1,), -7.0, device=dev, dtype=torch.float64)
    b = None if base is None else torch.tensor([base], device=dev, dtype=torch.float32)
    scale = b if alias else torch.full((1,), -7.0, device=dev, dtype=torch.float32)
    L.check(h.mtn_grad_sumsq(n, x.data_ptr(), partial.data_ptr(), L.stream_ptr()))
    L.check(h.mtn_clip_scale(npart, partial.data_ptr(), C.c_float(max_norm), L.ptr(b), scale.data_ptr(), norm.data_ptr(), L.ptr(stats),
                             L.stream_ptr()))
    return partial, scale, norm


def _check(norm, scale, want_norm, want_coef, want_scale, base):
    if not math.isfinite(want_norm):
        assert (math.isnan(norm) and math.isnan(want_norm)) or norm == want_norm
        assert math.isnan(scale)
        return
    print("norm %.17g reference %.17g relative error %.3g; scale %.9g reference %.9g" %
          (norm, want_norm, abs(norm - want_norm) / want_norm if want_norm else 0.0, scale, float(want_scale)))
    assert abs(norm - want_norm) <= 1e-12 * want_norm
    if want_coef == 1.0:
        assert np.float32(scale).view(np.int32) == np.float32(1.0 if base is None else base).view(np.int32)
    else:
        assert abs(np.float32(scale) - want_scale) <= np.spacing(np.abs(want_scale))


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c["id"])
def test_norm_and_scale_match_the_reference(dev, case):
    x = torch.from_numpy(R.data(case)).to(dev)
    want_norm, want_coef, want_scale = R.expected(case["id"])
    partial, scale, norm = _launch(x, case["max_norm"], case["base"])
    again = _launch(x, case["max_norm"], case["base"])
    torch.cuda.synchronize()
    npart = partial.numel() - GUARD
    assert bool((partial[npart:] == -7.0).all())                                          # one double per workgroup, no more
    for a, b in zip((partial, scale, norm), again):                                       # two launches, identical bytes
        assert torch.equal(a.view(torch.int64 if a.dtype == torch.float64 else torch.int32),
                           b.view(torch.int64 if b.dtype == torch.float64 else torch.int32))
    _check(float(norm), float(scale), want_norm, want_coef, want_scale, case["base"])
    if case["kind"] == "randn":                                                           # the partials are the workgroups' own sums
        assert bool((partial[:npart] >= 0).all())
        b32 = 1.0 if case["base"] is None else abs(float(np.float32(case["base"])))
        assert abs(math.sqrt(math.fsum(partial[:npart].cpu().tolist())) * b32 - want_norm) <= 1e-12 * want_norm


def test_scale_out_may_be_the_base_itself(dev):
    case = next(c for c in R.CASES if c["base"] is not None and R.expected(c["id"])[1] < 1.0)
    x = torch.from_numpy(R.data(case)).to(dev)
    _, apart, _ = _launch(x, case["max_norm"], case["base"])
    _, same, _ = _launch(x, case["max_norm"], case["base"], alias=True)
    assert torch.equal(apart.view(torch.int32), same.view(torch.int32)) and float(same) != case["base"]


def test_the_stats_block_over_a_sequence_of_calls(dev):
    ids = ["n1025-randn-s1-f0.5-b0.125", "n1025-randn-s1-f2-b-3", "n5-zeros-s1-f1", "n3-nan-s1-f0.5", "n4-inf-s1-f0.5"]
    seq = [next(c for c in R.CASES if c["id"] == i) for i in ids]
    seq += [c for c in R.CASES if c["n"] == 1023 and c["kind"] == "randn"]
    stats = torch.zeros(5, device=dev, dtype=torch.float64)
    want = [0.0] * 5
    for k, case in enumerate(seq * 2):
        x = torch.from_numpy(R.data(case)).to(dev)
        _launch(x, case["max_norm"], case["base"], stats=stats)
        norm, coef, _ = R.expected(case["id"])
        R.stats_update(want, norm, coef)
        if k == len(seq) - 1:
            mid = stats.cpu().tolist()
            assert mid[2:] == want[2:] and mid[2] == len(seq)
    got = stats.cpu().tolist()
    print("stats", got, "reference", want)
    assert got[2:] == want[2:] and got[4] == 4 and 0 < got[3] < got[2]
    assert abs(got[0] - want[0]) <= 1e-12 * want[0] and abs(got[1] - want[1]) <= 1e-12 * want[1]


def test_the_calls_are_capturable(dev):
    """Both launches inside a hipGraph: the replay computes what the eager call computes, and follows the buffer's contents."""
    from mtn_amd import lib as L
    h = L.load()
    case = next(c for c in R.CASES if c["id"] == "n1025-randn-s1-f0.5-b0.125")
    x = torch.from_numpy(R.data(case)).to(dev)
    _, e_scale, e_norm = _launch(x, case["max_norm"], case["base"])
    npart = R.partials(x.numel())
    partial = torch.zeros(npart, device=dev, dtype=torch.float64)
    out = torch.zeros(2, device=dev, dtype=torch.float64)
    scale = torch.zeros(1, device=dev, dtype=torch.float32)
    base = torch.tensor([case["base"]], device=dev, dtype=torch.float32)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        L.check(h.mtn_grad_sumsq(x.numel(), x.data_ptr(), partial.data_ptr(), L.stream_ptr()))
        L.check(h.mtn_clip_scale(npart, partial.data_ptr(), C.c_float(case["max_norm"]), base.data_ptr(), scale.data_ptr(), out.data_ptr(),
                                 None, L.stream_ptr()))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out[:1].view(torch.int64), e_norm.view(torch.int64)) and torch.equal(scale.view(torch.int32), e_scale.view(torch.int32))
    x.mul_(2.0)
    g.replay()
    torch.cuda.synchronize()
    assert float(out[0]) == 2.0 * float(e_norm)                                            # doubling is exact at every step of the sum
