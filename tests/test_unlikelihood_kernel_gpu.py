"""mtn_ulosshead_fwd / mtn_ulosshead_bwd (csrc/losshead.hip) through the C ABI against the float64 definition of
tests/unlikelihood_refs.py (validated without a GPU by tests/test_unlikelihood_refs.py), outputs and guard regions pre-filled with NaN,
1e30 in the padding columns of the logits, inputs compared bytewise afterwards.

Where the bounds come from (none was obtained by running the kernel): the kernel is float32 with __expf / __logf.  The SAME closed form
evaluated in float32 with torch on the CPU (unlikelihood_refs.closed_form_f32) against the float64 reference, worst over
unlikelihood_refs.ul_cases(), measures
    lse 8.0e-7 absolute | rowloss 2.5e-7 of the case's largest |rowloss| | rowul 3.3e-7 of max(1, the case's largest ul) |
    dlogits 3.5e-7 of max |ref|
(unlikelihood_refs.CPU_F32_UL_*; tests/test_unlikelihood_refs.py re-measures them, and checks that every unclamped candidate has
p_c <= 0.9 and the clamped one 1 - p_c <= 1e-9).  The kernel gets 4x each — fast-math intrinsics and another summation order, the margin
tests/test_row_kernels_gpu.py and tests/test_distill_kernel_gpu.py give.  bfloat16 dlogits are ONE rounding of the float32 value: + 1
bfloat16 ulp of the reference element (row_refs.bf16_ulp), as for the plain loss head.
"""
import ctypes as C

import pytest
import torch

from tests import row_refs as rr
from tests import unlikelihood_refs as ur

pytestmark = pytest.mark.gpu

LSE_ABS = 4 * ur.CPU_F32_UL_LSE
ROWLOSS_REL = 4 * ur.CPU_F32_UL_ROWLOSS
ROWUL_REL = 4 * ur.CPU_F32_UL_ROWUL
DLOGITS_REL = 4 * ur.CPU_F32_UL_DLOGITS
NAN = float("nan")
PAD_SENTINEL = 1e30
CASES = ur.ul_cases()
IDS = [ur.ul_case_id(c) for c in CASES]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def hip():
    from mtn_amd import lib as L
    return L, L.load()


@pytest.fixture(scope="module")
def refs():
    """inputs and the float64 reference of every case, computed once"""
    out = []
    for i, c in enumerate(CASES):
        z, targets = ur.ul_inputs(c, ur.UL_SEED + i)
        out.append((z, targets, ur.composed_ul(z, targets, c)))
    return out


def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _all_nan(t):
    return bool(torch.isnan(t).all())


class _Run:
    """Device buffers of one case.  lse / rowloss / rowul carry 4 extra elements and dlogits one extra row, all NaN; the padding columns
    of the logits hold 1e30.  ``A`` is the unlikelihood block, ``H`` the plain loss head's on the SAME buffers."""

    def __init__(self, L, dev, case, z, targets, dtype=torch.float32, ul_alpha=None, seq_len=None):
        self.case, segs = case, ur.seg_rows(case)
        self.rows = sum(segs)
        self.ldz, self.ldd = case.V + case.ldz_pad, case.V + case.ldd_pad
        zb = torch.full((self.rows, self.ldz), PAD_SENTINEL)
        zb[:, :case.V] = z
        self.z0, self.z = zb, zb.to(dev)
        self.t0, self.targets = targets, [t.to(dev) for t in targets]
        self.norm = torch.tensor(rr.NORM, device=dev)
        self.gloss = torch.tensor([rr.GLOSS], device=dev)
        self.lse = torch.full((self.rows + 4,), NAN, device=dev)
        self.rowloss = torch.full((self.rows + 4,), NAN, device=dev)
        self.rowul = torch.full((self.rows + 4,), NAN, device=dev)
        self.dz = torch.full((self.rows + 1, self.ldd), NAN, device=dev, dtype=dtype)
        self.A, self.H = L.ULossHeadArgs(), L.LossHeadArgs()
        for A in (self.A, self.H):
            A.n_seg = len(segs)
            for s, n in enumerate(segs):
                A.rows[s], A.target[s], A.norm[s], A.coef[s] = n, self.targets[s].data_ptr(), self.norm.data_ptr() + 4 * s, rr.COEF[s]
            A.V, A.ldz, A.pad, A.smoothing = case.V, self.ldz, case.pad, case.smoothing
            A.logits, A.lse, A.rowloss = self.z.data_ptr(), self.lse.data_ptr(), self.rowloss.data_ptr()
            A.gloss, A.dlogits, A.ldd = self.gloss.data_ptr(), self.dz.data_ptr(), self.ldd
        for s, T in enumerate(ur.seq_lens(case) if seq_len is None else seq_len):
            self.A.seq_len[s] = T
        self.A.ul_alpha, self.A.rowul = case.ul_alpha if ul_alpha is None else ul_alpha, self.rowul.data_ptr()

    def new_dz(self, dev, dtype):
        self.dz = torch.full((self.rows + 1, self.ldd), NAN, device=dev, dtype=dtype)
        self.A.dlogits = self.H.dlogits = self.dz.data_ptr()

    def inputs_unchanged(self):
        return _same_bits(self.z.cpu(), self.z0) and all(_same_bits(t.cpu(), t0) for t, t0 in zip(self.targets, self.t0))


@pytest.mark.parametrize("idx", range(len(CASES)), ids=IDS)
def test_unlikelihood_forward_and_backward(dev, hip, refs, idx):
    """lse, rowloss, rowul row by row and their sums, dlogits in float32 and bfloat16, against the float64 reference; exact +0.0 where the
    contract says so; guards and inputs untouched; two launches, equal bytes."""
    L, lib = hip
    c = CASES[idx]
    z, targets, ref = refs[idx]
    R = _Run(L, dev, c, z, targets)
    L.check(lib.mtn_ulosshead_fwd(C.byref(R.A), L.stream_ptr()))
    torch.cuda.synchronize()
    n, V = R.rows, c.V
    lse, rowloss, rowul = R.lse.cpu(), R.rowloss.cpu(), R.rowul.cpu()
    assert _all_nan(lse[n:]) and _all_nan(rowloss[n:]) and _all_nan(rowul[n:])
    assert not torch.isnan(lse[:n]).any() and not torch.isnan(rowloss[:n]).any() and not torch.isnan(rowul[:n]).any()
    big, bigul = float(ref["rowloss"].abs().max()), max(1.0, float(ref["rowul"].abs().max()))
    e_lse = float((lse[:n].double() - ref["lse"]).abs().max())
    e_row = float((rowloss[:n].double() - ref["rowloss"]).abs().max()) / max(big, 1e-30)
    e_ul = float((rowul[:n].double() - ref["rowul"]).abs().max()) / bigul
    e_sum = abs(float(rowloss[:n].double().sum()) - ref["total"])
    e_ulsum = abs(float(rowul[:n].double().sum()) - float(ref["rowul"].sum()))
    print(f"lse abs {e_lse:.3e} (bound {LSE_ABS:.3e})  rowloss rel {e_row:.3e} (bound {ROWLOSS_REL:.3e})  rowul rel {e_ul:.3e} "
          f"(bound {ROWUL_REL:.3e})  sum abs {e_sum:.3e}  ul sum abs {e_ulsum:.3e}")
    ok = [e_lse <= LSE_ABS, e_row <= ROWLOSS_REL, e_ul <= ROWUL_REL]
    ok.append(e_sum <= ROWLOSS_REL * big * n and e_ulsum <= ROWUL_REL * bigul * n)       # n rows, each within its bound
    zero = ref["zero"]
    has_c = ur.candidate_mask(c, targets).any(1)
    no_ul = torch.cat([(t == c.pad) | (torch.arange(t.numel()) % max(T, 1) == 0) | (T == 0) for t, T in zip(targets, ur.seq_lens(c))])
    assert not bool((has_c & no_ul).any())
    assert bool((_bits(rowloss[:n][zero]) == 0).all())
    assert bool((_bits(rowul[:n][no_ul]) == 0).all())                                    # <pad> rows, t = 0 rows, non-UL segments: +0.0
    assert R.inputs_unchanged()

    dmax = float(ref["dlogits"].abs().max())
    for dtype in (torch.float32, torch.bfloat16):
        if dtype == torch.bfloat16:
            R.new_dz(dev, dtype)
        L.check(lib.mtn_ulosshead_bwd(L.dtype_code(dtype), C.byref(R.A), L.stream_ptr()))
        torch.cuda.synchronize()
        dz = R.dz.cpu()
        assert _all_nan(dz[n])
        assert bool((_bits(dz[:n, V:]) == 0).all())                                      # columns V..ldd-1: +0.0 in every row
        assert bool((_bits(dz[:n][zero]) == 0).all())
        got = dz[:n, :V].double()
        assert not torch.isnan(got).any()
        if dtype == torch.float32:
            want, tol = ref["dlogits"], torch.full_like(got, DLOGITS_REL * dmax)
        else:
            want, tol = ref["dlogits"].to(torch.bfloat16).double(), rr.bf16_ulp(ref["dlogits"]) + DLOGITS_REL * dmax
        err = (got - want).abs()
        print(f"{dtype}: dlogits worst err / bound {float((err / tol).max()):.3f}, rel to max {float(err.max()) / max(dmax, 1e-30):.3e}")
        ok.append(bool((err <= tol).all()))
        again = torch.full_like(R.dz, NAN)
        R.A.dlogits = again.data_ptr()
        L.check(lib.mtn_ulosshead_bwd(L.dtype_code(dtype), C.byref(R.A), L.stream_ptr()))
        torch.cuda.synchronize()
        assert _same_bits(again.cpu(), dz)
        assert R.inputs_unchanged() and _same_bits(R.lse.cpu()[:n], lse[:n])
    L.check(lib.mtn_ulosshead_fwd(C.byref(R.A), L.stream_ptr()))
    torch.cuda.synchronize()
    assert _same_bits(R.lse.cpu(), lse) and _same_bits(R.rowloss.cpu(), rowloss) and _same_bits(R.rowul.cpu(), rowul)
    assert all(ok), ok


@pytest.mark.parametrize("idx", range(len(CASES)), ids=IDS)
@pytest.mark.parametrize("how", ["alpha0", "seq_len0"])
def test_without_candidates_the_bits_are_the_loss_heads(dev, hip, refs, idx, how):
    """ul_alpha = 0 with the sequence lengths given, and the case's ul_alpha with every seq_len 0: lse, rowloss and dlogits (float32 and
    bfloat16) equal mtn_losshead_fwd / _bwd on the same buffers bit for bit, and rowul is +0.0."""
    L, lib = hip
    c = CASES[idx]
    z, targets, _ = refs[idx]
    if how == "alpha0":
        R = _Run(L, dev, c, z, targets, ul_alpha=0.0)
    else:
        R = _Run(L, dev, c, z, targets, seq_len=[0] * len(c.layout))
    n = R.rows
    L.check(lib.mtn_losshead_fwd(C.byref(R.H), L.stream_ptr()))
    torch.cuda.synchronize()
    lse_h, row_h = R.lse.clone(), R.rowloss.clone()
    R.lse.fill_(NAN); R.rowloss.fill_(NAN)
    L.check(lib.mtn_ulosshead_fwd(C.byref(R.A), L.stream_ptr()))
    torch.cuda.synchronize()
    assert _same_bits(R.lse, lse_h) and _same_bits(R.rowloss, row_h)
    assert bool((_bits(R.rowul[:n]) == 0).all()) and _all_nan(R.rowul[n:])
    for dtype in (torch.float32, torch.bfloat16):
        R.new_dz(dev, dtype)
        L.check(lib.mtn_losshead_bwd(L.dtype_code(dtype), C.byref(R.H), L.stream_ptr()))
        torch.cuda.synchronize()
        dz_h = R.dz
        R.new_dz(dev, dtype)
        L.check(lib.mtn_ulosshead_bwd(L.dtype_code(dtype), C.byref(R.A), L.stream_ptr()))
        torch.cuda.synchronize()
        assert _same_bits(R.dz, dz_h)


def test_rows_without_candidates_inside_a_ul_launch_are_the_loss_heads(dev, hip, refs):
    """The segments with seq_len 0 next to an unlikelihood segment (row base offset), and the <pad> and t = 0 rows of the unlikelihood
    segment itself: their lse, rowloss and dlogits rows are the plain loss head's bit for bit."""
    L, lib = hip
    for idx in (7, 12):
        c = CASES[idx]
        z, targets, _ = refs[idx]
        R = _Run(L, dev, c, z, targets)
        n = R.rows
        plain = ~ur.candidate_mask(c, targets).any(1)
        assert bool(plain[:ur.seg_rows(c)[0]].all()) and not bool(plain.all())
        L.check(lib.mtn_losshead_fwd(C.byref(R.H), L.stream_ptr()))
        L.check(lib.mtn_losshead_bwd(L.MTN_F32, C.byref(R.H), L.stream_ptr()))
        torch.cuda.synchronize()
        lse_h, row_h, dz_h = R.lse.cpu(), R.rowloss.cpu(), R.dz.cpu()
        R.lse.fill_(NAN); R.rowloss.fill_(NAN)
        R.new_dz(dev, torch.float32)
        L.check(lib.mtn_ulosshead_fwd(C.byref(R.A), L.stream_ptr()))
        L.check(lib.mtn_ulosshead_bwd(L.MTN_F32, C.byref(R.A), L.stream_ptr()))
        torch.cuda.synchronize()
        assert _same_bits(R.lse.cpu(), lse_h)                                              # lse does not depend on the candidates at all
        assert _same_bits(R.rowloss.cpu()[:n][plain], row_h[:n][plain]) and _same_bits(R.dz.cpu()[:n][plain], dz_h[:n][plain])
        assert not _same_bits(R.rowloss.cpu()[:n][~plain], row_h[:n][~plain])


def test_unlikelihood_argument_checks_leave_the_guards(dev, hip, refs):
    """Bad arguments raise and launch nothing: every output keeps its NaN."""
    L, lib = hip
    c = CASES[8]
    z, targets, _ = refs[8]

    def run(**kw):
        R = _Run(L, dev, c, z, targets)
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(R.A, k)[v[0]] = v[1]
            else:
                setattr(R.A, k, v)
        with pytest.raises(L.MtnHipError):
            L.check(lib.mtn_ulosshead_fwd(C.byref(R.A), L.stream_ptr()))
        for code in (L.MTN_F32, L.MTN_BF16):
            with pytest.raises(L.MtnHipError):
                L.check(lib.mtn_ulosshead_bwd(code, C.byref(R.A), L.stream_ptr()))
        torch.cuda.synchronize()
        assert _all_nan(R.dz) and _all_nan(R.lse) and _all_nan(R.rowloss) and _all_nan(R.rowul)

    for kw in (dict(ul_alpha=-0.5), dict(ul_alpha=NAN), dict(ul_alpha=float("inf")), dict(seq_len=(0, -1)), dict(seq_len=(0, 4)),
               dict(seq_len=(1, 60)), dict(V=258), dict(V=0), dict(n_seg=5), dict(n_seg=0), dict(rows=(1, 0)), dict(ldz=256), dict(pad=260),
               dict(pad=-1)):
        run(**kw)
