"""mtn_ensemble_rows (csrc/ensemble.hip) through the C ABI against the float64 restatement of its definitions (tests/ensemble_refs.py), on
the IDENTICAL float32 inputs, in both modes.

Bounds.  The -inf pattern: exact; no NaN.  Finite outputs: 4 x ensemble_refs.CPU_F32_ENSEMBLE_ABS, the error torch's float32 evaluation of
the same closed form shows on these cases on a CPU (tests/test_ensemble_refs.py re-measures it); the factor 4 is the margin the project gives
fast-math intrinsics and another summation order (tests/test_row_kernels_gpu.py, tests/test_score_kernel_gpu.py).  Guard regions around out
and the inputs themselves: bitwise unchanged.  Two launches: bitwise equal."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import ensemble_refs as er

pytestmark = pytest.mark.gpu
CASES = er.ens_cases()
GUARD = 64
BOUND = 4 * er.CPU_F32_ENSEMBLE_ABS


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    from mtn_amd import lib
    lib.load()
    return torch.device("cuda:0")


class _Out:
    """out (rows, ldo) inside a NaN-filled buffer with GUARD sentinel elements on either side; columns V..ldo-1 are sentinels too."""

    def __init__(self, dev, rows, V, ldo):
        self.rows, self.V, self.ldo = rows, V, ldo
        self.buf = torch.full((rows * ldo + 2 * GUARD,), float("nan"), device=dev)

    def ptr(self):
        return self.buf.data_ptr() + GUARD * 4

    def get(self):
        return self.buf[GUARD:GUARD + self.rows * self.ldo].view(self.rows, self.ldo)[:, :self.V].cpu()

    def untouched(self, whole=False):
        b = self.buf.cpu()
        if whole:
            return bool(torch.isnan(b).all())
        body = b[GUARD:GUARD + self.rows * self.ldo].view(self.rows, self.ldo)
        return bool(torch.isnan(b[:GUARD]).all() and torch.isnan(b[-GUARD:]).all() and torch.isnan(body[:, self.V:]).all())


def _args(xs, w, mode, dst, case, over=None):
    from mtn_amd import lib
    a = lib.EnsembleArgs()
    a.rows, a.V, a.M, a.mode, a.out, a.ldo = case.rows, case.V, case.M, mode, dst.ptr(), dst.ldo
    for m, x in enumerate(xs):
        a.x[m], a.ld[m], a.w[m] = x.data_ptr(), case.lds[m], float(w[m])
    for k, v in (over or {}).items():
        if isinstance(k, tuple):                       # ("w", 1) -> a.w[1]
            getattr(a, k[0])[k[1]] = v
        else:
            setattr(a, k, v)
    return a


def _launch(a):
    from mtn_amd import lib
    rc = lib.load().mtn_ensemble_rows(C.byref(a), lib.stream_ptr())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("idx", range(len(CASES)), ids=[er.ens_case_id(c) for c in CASES])
def test_ensemble_rows_matches_float64(dev, idx):
    c = CASES[idx]
    bufs, xs64, w = er.case_views(c, er.ENS_SEED + idx)
    xd = [b.to(dev) for b in bufs]
    before = [x.clone() for x in xd]
    for mode_i, mode in enumerate(er.MODES):
        ref = er.ensemble_ref64(xs64, w, mode)
        runs = []
        for ldo in (c.V, c.V + 3):                     # the second launch also with another (odd) out stride
            for _ in range(2 if ldo == c.V else 1):
                out = _Out(dev, c.rows, c.V, ldo)
                assert _launch(_args(xd, w, mode_i, out, c)) == 0
                assert out.untouched(), "a write outside the output rows"
                runs.append(out.get())
        got = runs[0].numpy()
        assert not np.isnan(got).any()
        assert np.array_equal(np.isneginf(got), np.isneginf(ref)) and not np.isposinf(got).any()
        err = er.worst_abs_error(got, ref)
        print(f"{er.ens_case_id(c)} {mode}: worst |error| {err:.3g} (bound {BOUND:.3g})")
        assert err <= BOUND, err
        assert torch.equal(runs[0].view(torch.int32), runs[1].view(torch.int32))              # two launches: the same bits
        err2 = er.worst_abs_error(runs[2].numpy(), ref)
        assert np.array_equal(np.isneginf(runs[2].numpy()), np.isneginf(ref)) and err2 <= BOUND, err2
    for x, b in zip(xd, before):                                                              # the inputs: bitwise unchanged
        assert torch.equal(x.view(torch.int32), b.view(torch.int32))


def test_ops_wrapper_and_unaligned_base(dev):
    """ops.ensemble_rows on rows that start at an odd element offset of their buffers, default and given weights, out given or not."""
    from mtn_amd import ops
    rows, V, M = 5, 301, 3
    g = torch.Generator().manual_seed(21)
    hosts = [(torch.rand(rows, V, generator=g) * 80 - 40).float() for _ in range(M)]
    xs64 = [h.double().numpy() for h in hosts]
    devs = []
    for m, h in enumerate(hosts):
        buf = torch.full((rows * (V + m) + 3,), float("nan"), device=dev)
        view = buf[m + 1:m + 1 + rows * (V + m)].view(rows, V + m)[:, :V]
        view.copy_(h.to(dev))
        devs.append(view)
    for weights, mode in ((None, "prob"), ([3, 1, 0], "logprob"), ([0.2, 0.3, 0.5], "prob")):
        w = ops.ensemble_weights(M, weights)
        assert abs(w.sum() - 1.0) < 1e-15
        ref = er.ensemble_ref64(xs64, w, mode)
        got = ops.ensemble_rows(devs, weights, mode)
        out = torch.full((rows, V + 5), float("nan"), device=dev)
        got2 = ops.ensemble_rows(devs, weights, mode, out=out[:, :V])
        torch.cuda.synchronize()
        assert got2.data_ptr() == out.data_ptr() and bool(torch.isnan(out[:, V:]).all())
        for t in (got, got2):
            assert er.worst_abs_error(t.cpu().numpy(), ref) <= BOUND
    one = ops.ensemble_rows(devs[:1]).cpu().numpy()                                           # M = 1: log_softmax
    assert er.worst_abs_error(one, torch.log_softmax(hosts[0].double(), 1).numpy()) <= BOUND


def test_bad_arguments_are_refused(dev):
    from mtn_amd import lib, ops
    c = er.EnsCase(3, 2, 64, (64, 66), "uniform", "logits")
    bufs, _, w = er.case_views(c, 5)
    xd = [b.to(dev) for b in bufs]
    bad = [dict(out=None), {("x", 0): None}, {("x", 1): None}, dict(M=0), dict(M=9), dict(M=-1), {("ld", 1): 63}, dict(ldo=63),
           dict(V=1 << 24), {("w", 0): -0.5}, {("w", 1): float("nan")}, {("w", 0): float("inf")}, {("w", 0): 0.0, ("w", 1): 0.0},
           dict(mode=2), dict(mode=-1), dict(rows=0), dict(V=0)]
    for over in bad:
        out = _Out(dev, c.rows, c.V, c.V)
        rc = _launch(_args(xd, w, 0, out, c, over))
        assert rc == 1, over                                          # MTN_ERR_ARG
        with pytest.raises(lib.MtnHipError):
            lib.check(rc)
        assert out.untouched(whole=True), over
    rc = lib.load().mtn_ensemble_rows(None, lib.stream_ptr())
    assert rc == 1
    out = _Out(dev, c.rows, c.V, c.V)
    assert _launch(_args(xd, w, 0, out, c)) == 0                      # ... and the good call goes through
    xs = [x[:, :c.V] for x in xd]
    with pytest.raises(lib.MtnHipError):
        ops.ensemble_rows([b[:, :c.V] for b in bufs])                 # CPU tensors
    misuse = [
        lambda: ops.ensemble_rows([]),
        lambda: ops.ensemble_rows(xs * 5),                            # 10 members
        lambda: ops.ensemble_rows(xs, mode="mean"),
        lambda: ops.ensemble_rows(xs, weights=[1.0]),
        lambda: ops.ensemble_rows(xs, weights=[1.0, -1.0]),
        lambda: ops.ensemble_rows(xs, weights=[0.0, 0.0]),
        lambda: ops.ensemble_rows(xs, weights=[float("nan"), 1.0]),
        lambda: ops.ensemble_rows([xs[0], xs[1][:, :32]]),            # another shape
        lambda: ops.ensemble_rows([xs[0], xs[1].double()]),           # another dtype
        lambda: ops.ensemble_rows([xs[0], xs[1][:2]]),
        lambda: ops.ensemble_rows([xs[0].t()[:, :3], xs[1].t()[:, :3]]),      # column stride
        lambda: ops.ensemble_rows(xs, out=xs[0]),                     # out is an input
        lambda: ops.ensemble_rows(xs, out=xd[1][:, 1:c.V + 1]),       # out overlaps an input
        lambda: ops.ensemble_rows(xs, out=torch.empty(c.rows, c.V, device=dev, dtype=torch.float64)),
        lambda: ops.ensemble_rows(xs, out=torch.empty(c.rows, c.V + 1, device=dev)),
    ]
    for i, f in enumerate(misuse):
        with pytest.raises(ValueError):
            f()
            pytest.fail(f"misuse {i} was accepted")
    for x, b in zip(xd, bufs):                                        # nothing wrote into the inputs
        assert torch.equal(x.cpu()[:, :c.V], b[:, :c.V])


def test_abi_version(dev):
    from mtn_amd import lib
    assert lib.load().mtn_version() >= 118
