"""mtn_grad_accum (csrc/gradaccum.hip) against tests/accum_refs.py, bit for bit, on the cases that file lists: sizes below one vector,
with and without the scalar tail, more than one workgroup, and one above the grid cap with a tail (every thread loops twice, the first
ones three times); windows of K = 2 (FIRST / LAST) and K = 3 (FIRST / ADD / LAST); magnitudes 1, 1e-30 and 1e30, a NaN and an inf.
  * every launch's buffer and total equal numpy float32's, bit for bit (a NaN is a NaN: the hardware's default NaN is not numpy's);
  * LAST with partials writes the bytes of a mtn_grad_sumsq launch over the g it wrote;
  * two identical windows give identical bytes; acc is unchanged by LAST; g is unchanged by FIRST and ADD;
  * guard elements around every buffer stay as they were."""
import numpy as np
import pytest
import torch

from tests import accum_refs as R

pytestmark = pytest.mark.gpu
GUARD = 8                                                # elements on either side of every buffer that must stay as they were
MARK = -7.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


def _guarded(x, dev, dtype=torch.float32):
    """A device buffer with GUARD marked elements on either side of a copy of x (GUARD * 4 bytes keep the 16-byte alignment)."""
    buf = torch.full((x.numel() + 2 * GUARD,), MARK, device=dev, dtype=dtype)
    buf[GUARD:GUARD + x.numel()] = x
    return buf


def _inner(buf):
    return buf[GUARD:buf.numel() - GUARD]


def _guards_intact(buf):
    return bool((buf[:GUARD] == MARK).all()) and bool((buf[buf.numel() - GUARD:] == MARK).all())


def _bits(t):
    return t.detach().contiguous().view({8: torch.int64, 4: torch.int32}[t.element_size()])


def _accum(mode, acc, g, w, tin, tout, partial=None):
    from mtn_amd import lib as L
    n = _inner(g).numel()
    L.check(L.load().mtn_grad_accum(mode, n, _inner(acc).data_ptr(), _inner(g).data_ptr(), w.data_ptr(), L.ptr(tin), tout.data_ptr(),
                                    L.ptr(None if partial is None else _inner(partial)), L.stream_ptr()))


def _window(case, dev, with_partial):
    """One window on the device, checked launch by launch.  Returns (g, acc, totals, partial) as left behind."""
    from mtn_amd import lib as L
    h = L.load()
    gs, ws = R.data(case)
    n, K = case["n"], case["K"]
    acc = _guarded(torch.zeros(n), dev)
    acc_want, tot_want = None, None
    totals = torch.full((2 + 2 * GUARD,), MARK, device=dev)          # the two slots the caller alternates, guarded
    slot = [totals[GUARD:GUARD + 1], totals[GUARD + 1:GUARD + 2]]
    partial = _guarded(torch.zeros(h.mtn_grad_sumsq_partials(n), dtype=torch.float64), dev, torch.float64) if with_partial else None
    g_last = None
    for k in range(K):
        g = _guarded(torch.from_numpy(gs[k]), dev)
        w = torch.tensor([float(ws[k])], device=dev)
        tin, tout = (None if k == 0 else slot[(k - 1) & 1]), slot[k & 1]
        if k < K - 1:
            _accum(R.FIRST if k == 0 else R.ADD, acc, g, w, tin, tout)
            acc_want, tot_want = R.first(gs[0], ws[0]) if k == 0 else R.add(acc_want, gs[k], ws[k], tot_want)
            torch.cuda.synchronize()
            assert R.same_bytes(_inner(acc).cpu().numpy(), acc_want), "acc after micro-step %d" % (k + 1)
            assert np.array_equal(_inner(g).cpu().numpy().view(np.int32), gs[k].view(np.int32))          # g is read only here
        else:
            before = _bits(_inner(acc)).clone()
            _accum(R.LAST, acc, g, w, tin, tout, partial)
            g_want, tot_want = R.last(acc_want, gs[k], ws[k], tot_want)
            torch.cuda.synchronize()
            assert R.same_bytes(_inner(g).cpu().numpy(), g_want), "g after LAST"
            assert torch.equal(_bits(_inner(acc)), before)                                              # acc is read only here
            g_last = g
        assert float(tout) == float(tot_want)
        assert _guards_intact(g) and _guards_intact(acc) and _guards_intact(totals)
    assert float(tot_want) == sum(float(w) for w in ws)
    if partial is not None:
        assert _guards_intact(partial)
    return g_last, acc, totals, partial


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c["id"])
def test_a_window_matches_numpy_bit_for_bit(dev, case):
    from mtn_amd import lib as L
    h = L.load()
    g, acc, totals, none = _window(case, dev, with_partial=False)
    g2, acc2, totals2, partial = _window(case, dev, with_partial=True)
    torch.cuda.synchronize()
    assert none is None
    for a, b in ((g, g2), (acc, acc2), (totals, totals2)):                 # two identical windows, identical bytes; partials change nothing
        assert torch.equal(_bits(a), _bits(b))
    n = case["n"]
    npart = h.mtn_grad_sumsq_partials(n)
    sep = _guarded(torch.zeros(npart, dtype=torch.float64), dev, torch.float64)
    L.check(h.mtn_grad_sumsq(n, _inner(g2).data_ptr(), _inner(sep).data_ptr(), L.stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(_bits(partial), _bits(sep))                         # the bytes of a mtn_grad_sumsq launch over the written g


def test_partials_of_finite_data_are_the_norm(dev):
    """Without the NaN and the inf the partials are numbers: they sum to the float64 norm of the g that LAST wrote."""
    import math
    from mtn_amd import lib as L
    h = L.load()
    n = 256 * 1024 + 7
    rng = np.random.default_rng(5)
    g1, g2 = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    acc, g = _guarded(torch.zeros(n), dev), _guarded(torch.from_numpy(g2), dev)
    w = torch.tensor([300.0, 700.0], device=dev)
    tot = torch.zeros(2, device=dev)
    partial = _guarded(torch.zeros(h.mtn_grad_sumsq_partials(n), dtype=torch.float64), dev, torch.float64)
    _accum(R.FIRST, acc, _guarded(torch.from_numpy(g1), dev), w[0:1], None, tot[0:1])
    _accum(R.LAST, acc, g, w[1:2], tot[0:1], tot[1:2], partial)
    torch.cuda.synchronize()
    want, total = R.window([g1, g2], [300.0, 700.0])
    assert R.same_bytes(_inner(g).cpu().numpy(), want) and tot.cpu().tolist() == [300.0, 1000.0] == [300.0, float(total)]
    norm = math.sqrt(math.fsum((want.astype(np.float64) ** 2).tolist()))
    got = math.sqrt(math.fsum(_inner(partial).cpu().tolist()))
    assert abs(got - norm) <= 1e-12 * norm and _guards_intact(partial)


def test_the_launches_are_capturable(dev):
    """A K = 3 window inside a hipGraph: the replay computes what numpy computes, and follows the buffers' contents."""
    case = dict(id="capture", n=1023, K=3)
    gs, ws = R.data(case)
    n = case["n"]
    acc = _guarded(torch.zeros(n), dev)
    g = [_guarded(torch.from_numpy(x), dev) for x in gs]
    w = torch.tensor([float(x) for x in ws], device=dev)
    tot = torch.zeros(2, device=dev)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _accum(R.FIRST, acc, g[0], w[0:1], None, tot[0:1])
        _accum(R.ADD, acc, g[1], w[1:2], tot[0:1], tot[1:2])
        _accum(R.LAST, acc, g[2], w[2:3], tot[1:2], tot[0:1])
    for rep in range(2):
        graph.replay()
        torch.cuda.synchronize()
        want, total = R.window(gs, ws)
        assert R.same_bytes(_inner(g[2]).cpu().numpy(), want) and float(tot[0]) == float(total)
        gs[2] = want.copy()                                # LAST wrote g_3 in place: the next replay reads that
