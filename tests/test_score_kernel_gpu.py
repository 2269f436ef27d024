"""mtn_score_rows (csrc/score.hip) through the C ABI against the float64 restatement of its definitions (tests/score_refs.py), on the
IDENTICAL float32 logits.

Bounds.  tok_rank: exact — integer logic on the same float32 values.  tok_logp: 4 x score_refs.CPU_F32_TOK_LOGP_ABS, the error torch's
float32 evaluation of the same closed form shows on these cases on a CPU (tests/test_score_refs.py re-measures it); the factor 4 is the
margin the project gives fast-math intrinsics and another summation order (tests/test_row_kernels_gpu.py).  seq_logp: bitwise the
float64 sum of the kernel's own tok_logp in ascending position.  Two launches: bitwise equal."""
import ctypes as C

import pytest
import torch

from tests import score_refs as sr

pytestmark = pytest.mark.gpu
CASES = sr.score_cases()
GUARD = 64


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    from mtn_amd import lib
    lib.load()
    return torch.device("cuda:0")


class _Out:
    """The four outputs, each inside a buffer with GUARD sentinel elements on either side."""

    def __init__(self, dev, n, L):
        mk = lambda numel, dtype, fill: torch.full((numel + 2 * GUARD,), fill, dtype=dtype, device=dev)
        self.fills = (float("nan"), -77, float("nan"), -77)
        self.bufs = (mk(n * L, torch.float32, self.fills[0]), mk(n * L, torch.int32, self.fills[1]), mk(n, torch.float64, self.fills[2]),
                     mk(n, torch.int32, self.fills[3]))
        self.shapes = ((n, L), (n, L), (n,), (n,))

    def ptr(self, i):
        return self.bufs[i].data_ptr() + GUARD * self.bufs[i].element_size()

    def get(self, i):
        return self.bufs[i][GUARD:-GUARD].view(self.shapes[i]).cpu()

    def untouched(self, i, whole=False):
        b = self.bufs[i].cpu()
        g = b if whole else torch.cat([b[:GUARD], b[-GUARD:]])
        return bool(torch.isnan(g).all()) if b.is_floating_point() else bool((g == self.fills[i]).all())


def _args(z, t, out, case, **over):
    from mtn_amd import lib
    a = lib.ScoreArgs()
    a.n_seq, a.L, a.V, a.pad, a.ldz = case.n_seq, case.L, case.V, sr.PAD, case.ldz
    a.logits, a.target = z.data_ptr(), t.data_ptr()
    a.tok_logp, a.tok_rank, a.seq_logp, a.seq_len = (out.ptr(i) for i in range(4))
    for k, v in over.items():
        setattr(a, k, v)
    return a


def _launch(a):
    from mtn_amd import lib
    rc = lib.load().mtn_score_rows(C.byref(a), lib.stream_ptr())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("idx", range(len(CASES)), ids=[sr.score_case_id(c) for c in CASES])
def test_score_rows_matches_float64(dev, idx):
    c = CASES[idx]
    z, t, _ = sr.score_inputs(c, sr.SCORE_SEED + idx)
    ref_logp, ref_rank, ref_seq, ref_len = sr.score_ref64(z, t, c.V)
    zd, td = z.to(dev), t.to(dev)
    runs = []
    for _ in range(2):
        out = _Out(dev, c.n_seq, c.L)
        assert _launch(_args(zd, td, out, c)) == 0
        assert all(out.untouched(i) for i in range(4)), "a write outside the outputs"
        runs.append(tuple(out.get(i) for i in range(4)))
    logp, rank, seq, n = runs[0]
    assert not bool(torch.isnan(logp).any()) and not bool(torch.isnan(seq).any())
    assert torch.equal(rank, ref_rank), (rank, ref_rank)
    assert torch.equal(n, ref_len)
    err = float((logp.double() - ref_logp).abs().max())
    print(f"{sr.score_case_id(c)}: tok_logp worst |error| {err:.3g} (bound {4 * sr.CPU_F32_TOK_LOGP_ABS:.3g})")
    assert err <= 4 * sr.CPU_F32_TOK_LOGP_ABS, err
    ok = sr.valid_targets(t, c.V)
    assert bool((logp[~ok] == 0).all()) and bool((rank[~ok] == -1).all())
    assert torch.equal(seq.view(torch.int64), sr.seq_sum64(logp).view(torch.int64))          # bitwise
    if c.n_seq >= 2:                                                                          # the all-<pad> sequence
        assert int(n[-1]) == 0 and float(seq[-1]) == 0.0 and not bool(torch.signbit(seq[-1]))
    for a_, b_ in zip(runs[0], runs[1]):                                                      # two launches: the same bits
        assert torch.equal(a_.view(torch.int64 if a_.element_size() == 8 else torch.int32),
                           b_.view(torch.int64 if b_.element_size() == 8 else torch.int32))


def test_misaligned_rows_and_ops_wrapper(dev):
    """Rows that start at any of the four 16-byte phases (odd ldz, an offset base) through ops.score_rows: the same numbers."""
    from mtn_amd import ops
    n, L, V, ldz = 2, 6, 301, 303
    g = torch.Generator().manual_seed(11)
    buf = torch.full((n * L * ldz + 3,), float("nan"))
    z = buf[3:].view(n * L, ldz)
    z[:, :V] = torch.randn(n * L, V, generator=g) * 8.0
    t = torch.randint(2, V, (n, L), generator=g)
    t[1, 4:] = sr.PAD
    ref = sr.score_ref64(z, t, V)
    zd = buf.to(dev)[3:].view(n * L, ldz)[:, :V]
    logp, rank, seq, cnt = ops.score_rows(zd, t.to(dev), sr.PAD)
    torch.cuda.synchronize()
    assert torch.equal(rank.cpu(), ref[1]) and torch.equal(cnt.cpu(), ref[3])
    assert float((logp.cpu().double() - ref[0]).abs().max()) <= 4 * sr.CPU_F32_TOK_LOGP_ABS
    assert torch.equal(seq.cpu().view(torch.int64), sr.seq_sum64(logp.cpu()).view(torch.int64))


def test_bad_arguments_are_refused(dev):
    from mtn_amd import lib, ops
    c = sr.ScoreCase(2, 3, 64, 64, 0.0)
    z, t, _ = sr.score_inputs(c, 5)
    zd, td = z.to(dev), t.to(dev)
    bad = [dict(logits=None), dict(target=None), dict(tok_logp=None), dict(tok_rank=None), dict(seq_logp=None), dict(seq_len=None),
           dict(V=1), dict(V=1 << 24, ldz=1 << 24), dict(ldz=63), dict(L=0), dict(n_seq=0)]
    for over in bad:
        out = _Out(dev, c.n_seq, c.L)
        rc = _launch(_args(zd, td, out, c, **over))
        assert rc != 0, over
        with pytest.raises(lib.MtnHipError):
            lib.check(rc)
        assert all(out.untouched(i, whole=True) for i in range(4)), over
    with pytest.raises(lib.MtnHipError):
        ops.score_rows(z, t, sr.PAD)                                  # CPU tensors
    with pytest.raises(ValueError):
        ops.score_rows(zd, td[:1], sr.PAD)                            # one row of logits per target position
    out = _Out(dev, c.n_seq, c.L)
    assert _launch(_args(zd, td, out, c)) == 0                        # ... and the good call goes through


def test_abi_version(dev):
    from mtn_amd import lib
    assert lib.load().mtn_version() >= 116
