"""mtn_rlosshead_fwd / mtn_rlosshead_bwd (csrc/losshead.hip) through the C ABI against the float64 definition of tests/rdrop_refs.py
(validated without a GPU by tests/test_rdrop_refs.py), outputs and guard regions pre-filled with NaN, 1e30 in the padding columns of the
logits, inputs compared bytewise afterwards.

Where the bounds come from (none was obtained by running the kernel): the kernel is float32 with __expf / __logf.  The SAME formulas
evaluated in float32 with numpy on the CPU (rdrop_refs.closed_form_f32) against the float64 definition, worst over rdrop_refs.rd_cases(),
measure
    lse 2.1e-6 absolute | rowloss 7.1e-7 of the case's largest |rowloss| | rowrd 1.6e-7 and rowkl 7.5e-7 of max(1, the case's largest) |
    dlogits 1.7e-6 of g scale max(1, the case's largest |bracket|)
(rdrop_refs.CPU_F32_RD_*; tests/test_rdrop_refs.py re-measures them).  The kernel gets 4x each — fast-math intrinsics and another summation
order, the margin tests/test_row_kernels_gpu.py and tests/test_distill_kernel_gpu.py give.  bfloat16 dlogits are ONE rounding of the
float32 value: + 1 bfloat16 ulp of the reference element (row_refs.bf16_ulp), as for the other heads.
"""
import ctypes as C

import pytest
import torch

from tests import rdrop_refs as rd
from tests import row_refs as rr

pytestmark = pytest.mark.gpu

LSE_ABS = 4 * rd.CPU_F32_RD_LSE
ROWLOSS_REL = 4 * rd.CPU_F32_RD_ROWLOSS
ROWRD_REL = 4 * rd.CPU_F32_RD_ROWRD
ROWKL_REL = 4 * rd.CPU_F32_RD_ROWKL
DLOGITS = 4 * rd.CPU_F32_RD_DLOGITS
NAN = float("nan")
PAD_SENTINEL = 1e30
CASES = rd.rd_cases()
IDS = [rd.rd_case_id(c) for c in CASES]


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
    """inputs and the float64 definition of every case, computed once"""
    out = []
    for i, c in enumerate(CASES):
        z, targets = rd.rd_inputs(c, rd.RD_SEED + i)
        out.append((z, targets, rd.composed_rd(z, targets, c)))
    return out


def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _all_nan(t):
    return bool(torch.isnan(t).all())


class _Run:
    """Device buffers of one case.  lse / rowloss / rowrd / rowkl carry 4 extra elements and dlogits one extra row, all NaN; the padding
    columns of the logits hold 1e30.  ``A`` is the paired block, ``H`` the plain loss head's on the SAME buffers."""

    def __init__(self, L, dev, case, z, targets, dtype=torch.float32, rd_alpha=None, pair=None):
        self.case, segs = case, rd.seg_rows(case)
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
        self.rowrd = torch.full((self.rows + 4,), NAN, device=dev)
        self.rowkl = torch.full((self.rows + 4,), NAN, device=dev)
        self.dz = torch.full((self.rows + 1, self.ldd), NAN, device=dev, dtype=dtype)
        self.A, self.H = L.RLossHeadArgs(), L.LossHeadArgs()
        for A in (self.A, self.H):
            A.n_seg = len(segs)
            for s, n in enumerate(segs):
                A.rows[s], A.target[s], A.norm[s], A.coef[s] = n, self.targets[s].data_ptr(), self.norm.data_ptr() + 4 * s, rr.COEF[s]
            A.V, A.ldz, A.pad, A.smoothing = case.V, self.ldz, case.pad, case.smoothing
            A.logits, A.lse, A.rowloss = self.z.data_ptr(), self.lse.data_ptr(), self.rowloss.data_ptr()
            A.gloss, A.dlogits, A.ldd = self.gloss.data_ptr(), self.dz.data_ptr(), self.ldd
        for s, N in enumerate(rd.pairs(case) if pair is None else pair):
            self.A.pair[s] = N
        self.A.rd_alpha = case.rd_alpha if rd_alpha is None else rd_alpha
        self.A.rowrd, self.A.rowkl = self.rowrd.data_ptr(), self.rowkl.data_ptr()

    def new_dz(self, dev, dtype):
        self.dz = torch.full((self.rows + 1, self.ldd), NAN, device=dev, dtype=dtype)
        self.A.dlogits = self.H.dlogits = self.dz.data_ptr()

    def inputs_unchanged(self):
        return _same_bits(self.z.cpu(), self.z0) and all(_same_bits(t.cpu(), t0) for t, t0 in zip(self.targets, self.t0))


def _dz_check(case, ref, dz, dtype):
    """(all within the bound, worst error / bound) of a dlogits block [rows, V] against the definition"""
    got = dz.double()
    unit = (rr.GLOSS * rd.seg_scale(case)).unsqueeze(1) * max(1.0, ref["bracket"])
    if dtype == torch.float32:
        want, tol = ref["dlogits"], (DLOGITS * unit).expand_as(got)
    else:
        want, tol = ref["dlogits"].to(torch.bfloat16).double(), rr.bf16_ulp(ref["dlogits"]) + DLOGITS * unit
    err = (got - want).abs()
    return bool((err <= tol).all()), float((err / tol).max())


@pytest.mark.parametrize("idx", range(len(CASES)), ids=IDS)
def test_paired_forward_and_backward(dev, hip, refs, idx):
    """lse, rowloss, rowrd, rowkl row by row and their sums, dlogits in float32 and bfloat16, against the float64 definition; the pair's
    rowrd equal bit for bit; exact +0.0 where the contract says so; guards and inputs untouched; two launches, equal bytes."""
    L, lib = hip
    c = CASES[idx]
    z, targets, ref = refs[idx]
    R = _Run(L, dev, c, z, targets)
    L.check(lib.mtn_rlosshead_fwd(C.byref(R.A), L.stream_ptr()))
    torch.cuda.synchronize()
    n, V = R.rows, c.V
    lse, rowloss, rowrd, rowkl = R.lse.cpu(), R.rowloss.cpu(), R.rowrd.cpu(), R.rowkl.cpu()
    for t in (lse, rowloss, rowrd, rowkl):
        assert _all_nan(t[n:]) and not torch.isnan(t[:n]).any()
    e_lse, e_row, e_rd, e_kl, _ = rd.rd_errors(lse[:n], rowloss[:n], rowrd[:n], rowkl[:n], ref["dlogits"], ref, c)
    big, bigrd = float(ref["rowloss"].abs().max()), max(1.0, float(ref["rowrd"].abs().max()))
    e_sum = abs(float(rowloss[:n].double().sum()) - ref["total"])
    e_rdsum = abs(float(rowrd[:n].double().sum()) - float(ref["rowrd"].sum()))
    print(f"lse abs {e_lse:.3e} (bound {LSE_ABS:.3e})  rowloss rel {e_row:.3e} (bound {ROWLOSS_REL:.3e})  rowrd rel {e_rd:.3e} "
          f"(bound {ROWRD_REL:.3e})  rowkl rel {e_kl:.3e} (bound {ROWKL_REL:.3e})  sum abs {e_sum:.3e}  rd sum abs {e_rdsum:.3e}")
    ok = [e_lse <= LSE_ABS, e_row <= ROWLOSS_REL, e_rd <= ROWRD_REL, e_kl <= ROWKL_REL]
    ok.append(e_sum <= ROWLOSS_REL * big * n and e_rdsum <= ROWRD_REL * bigrd * n)         # n rows, each within its bound
    mask, j, zero = ref["mask"], rd.partner_index(c), ref["zero"]
    both = mask & mask[j]
    assert torch.equal(_bits(rowrd[:n])[both], _bits(rowrd[:n])[j][both])                  # the pair: equal bit for bit
    assert bool((rowrd[:n] >= 0).all())
    assert bool((_bits(rowloss[:n][zero]) == 0).all())
    assert bool((_bits(rowrd[:n][~mask]) == 0).all()) and bool((_bits(rowkl[:n][~mask]) == 0).all())   # <pad> rows, unpaired segments: +0.0
    if c.form in ("self", "off+", "off-"):
        assert float(rowrd[:n].max()) <= rd.RD_FLOOR
    assert R.inputs_unchanged()

    for dtype in (torch.float32, torch.bfloat16):
        if dtype == torch.bfloat16:
            R.new_dz(dev, dtype)
        L.check(lib.mtn_rlosshead_bwd(L.dtype_code(dtype), C.byref(R.A), L.stream_ptr()))
        torch.cuda.synchronize()
        dz = R.dz.cpu()
        assert _all_nan(dz[n])
        assert bool((_bits(dz[:n, V:]) == 0).all())                                      # columns V..ldd-1: +0.0 in every row
        assert bool((_bits(dz[:n][zero]) == 0).all())
        assert not torch.isnan(dz[:n, :V]).any()
        good, worst = _dz_check(c, ref, dz[:n, :V], dtype)
        print(f"{dtype}: dlogits worst err / bound {worst:.3f}")
        ok.append(good)
        again = torch.full_like(R.dz, NAN)
        R.A.dlogits = again.data_ptr()
        L.check(lib.mtn_rlosshead_bwd(L.dtype_code(dtype), C.byref(R.A), L.stream_ptr()))
        torch.cuda.synchronize()
        assert _same_bits(again.cpu(), dz)
        assert R.inputs_unchanged() and _same_bits(R.lse.cpu()[:n], lse[:n]) and _same_bits(R.rowkl.cpu()[:n], rowkl[:n])
    L.check(lib.mtn_rlosshead_fwd(C.byref(R.A), L.stream_ptr()))
    torch.cuda.synchronize()
    assert _same_bits(R.lse.cpu(), lse) and _same_bits(R.rowloss.cpu(), rowloss) and _same_bits(R.rowrd.cpu(), rowrd)
    assert _same_bits(R.rowkl.cpu(), rowkl)
    assert all(ok), ok


@pytest.mark.parametrize("idx", range(len(CASES)), ids=IDS)
@pytest.mark.parametrize("how", ["alpha0", "pair0"])
def test_without_pairs_the_bits_are_the_loss_heads(dev, hip, refs, idx, how):
    """rd_alpha = 0 with the pair distances given, and the case's rd_alpha with every pair 0: lse, rowloss and dlogits (float32 and
    bfloat16) equal mtn_losshead_fwd / _bwd on the same buffers bit for bit, and rowrd is +0.0."""
    L, lib = hip
    c = CASES[idx]
    z, targets, _ = refs[idx]
    if how == "alpha0":
        R = _Run(L, dev, c, z, targets, rd_alpha=0.0)
        R.A.rowkl = None                                                                  # (not required without a pair that counts)
    else:
        R = _Run(L, dev, c, z, targets, pair=[0] * len(c.layout))
    n = R.rows
    L.check(lib.mtn_losshead_fwd(C.byref(R.H), L.stream_ptr()))
    torch.cuda.synchronize()
    lse_h, row_h = R.lse.clone(), R.rowloss.clone()
    R.lse.fill_(NAN); R.rowloss.fill_(NAN)
    L.check(lib.mtn_rlosshead_fwd(C.byref(R.A), L.stream_ptr()))
    torch.cuda.synchronize()
    assert _same_bits(R.lse, lse_h) and _same_bits(R.rowloss, row_h)
    assert bool((_bits(R.rowrd[:n]) == 0).all()) and _all_nan(R.rowrd[n:])
    for dtype in (torch.float32, torch.bfloat16):
        R.new_dz(dev, dtype)
        L.check(lib.mtn_losshead_bwd(L.dtype_code(dtype), C.byref(R.H), L.stream_ptr()))
        torch.cuda.synchronize()
        dz_h = R.dz
        R.new_dz(dev, dtype)
        L.check(lib.mtn_rlosshead_bwd(L.dtype_code(dtype), C.byref(R.A), L.stream_ptr()))
        torch.cuda.synchronize()
        assert _same_bits(R.dz, dz_h)


def test_plain_rows_inside_a_paired_launch_are_the_loss_heads(dev, hip, refs):
    """The unpaired segments next to a paired one (before and behind it: the row base offset) and the <pad> rows of the paired segment
    itself, the quirk row included: their lse, rowloss and dlogits rows are the plain loss head's bit for bit."""
    L, lib = hip
    picked = [i for i, c in enumerate(CASES) if len(c.layout) > 1 and c.form in ("near", "indep", "x8")]
    picked += [i for i, c in enumerate(CASES) if c.pads == "lone0" and c.form in ("near", "indep", "x8") and i not in picked]
    assert {CASES[i].layout[0] < 0 for i in picked} == {False, True} and any(CASES[i].pads == "lone0" for i in picked)
    for idx in picked:
        c = CASES[idx]
        z, targets, ref = refs[idx]
        R = _Run(L, dev, c, z, targets)
        n = R.rows
        plain = ~ref["mask"]
        assert bool(plain.any()) and not bool(plain.all())
        L.check(lib.mtn_losshead_fwd(C.byref(R.H), L.stream_ptr()))
        L.check(lib.mtn_losshead_bwd(L.MTN_F32, C.byref(R.H), L.stream_ptr()))
        torch.cuda.synchronize()
        lse_h, row_h, dz_h = R.lse.cpu(), R.rowloss.cpu(), R.dz.cpu()
        R.lse.fill_(NAN); R.rowloss.fill_(NAN)
        R.new_dz(dev, torch.float32)
        L.check(lib.mtn_rlosshead_fwd(C.byref(R.A), L.stream_ptr()))
        L.check(lib.mtn_rlosshead_bwd(L.MTN_F32, C.byref(R.A), L.stream_ptr()))
        torch.cuda.synchronize()
        assert _same_bits(R.lse.cpu(), lse_h)                                              # lse does not depend on the partner at all
        assert _same_bits(R.rowloss.cpu()[:n][plain], row_h[:n][plain]) and _same_bits(R.dz.cpu()[:n][plain], dz_h[:n][plain])
        assert not _same_bits(R.rowloss.cpu()[:n][~plain], row_h[:n][~plain])


def test_self_pairs_add_nothing(dev, hip, refs):
    """z_j = z_i: |rd| under the floor and dlogits equal to the plain head's within DLOGITS * g * scale."""
    L, lib = hip
    picked = [i for i, c in enumerate(CASES) if c.form == "self"]
    assert len(picked) >= 3
    for idx in picked:
        c = CASES[idx]
        z, targets, _ = refs[idx]
        R = _Run(L, dev, c, z, targets)
        n = R.rows
        L.check(lib.mtn_losshead_fwd(C.byref(R.H), L.stream_ptr()))
        L.check(lib.mtn_losshead_bwd(L.MTN_F32, C.byref(R.H), L.stream_ptr()))
        torch.cuda.synchronize()
        dz_h = R.dz.cpu()
        R.new_dz(dev, torch.float32)
        L.check(lib.mtn_rlosshead_fwd(C.byref(R.A), L.stream_ptr()))
        L.check(lib.mtn_rlosshead_bwd(L.MTN_F32, C.byref(R.A), L.stream_ptr()))
        torch.cuda.synchronize()
        assert float(R.rowrd[:n].abs().max()) <= rd.RD_FLOOR
        unit = (rr.GLOSS * rd.seg_scale(c)).unsqueeze(1)
        err = (R.dz.cpu()[:n, :c.V].double() - dz_h[:n, :c.V].double()).abs() / unit
        print(f"{IDS[idx]}: dlogits against the plain head's, worst / (g scale) {float(err.max()):.3e} (bound {DLOGITS:.3e})")
        assert float(err.max()) <= DLOGITS


def test_paired_argument_checks_leave_the_guards(dev, hip, refs):
    """Bad arguments raise and launch nothing: every output keeps its NaN."""
    L, lib = hip
    idx = next(i for i, c in enumerate(CASES) if c.layout == (5, -3))
    c = CASES[idx]
    z, targets, _ = refs[idx]

    def run(**kw):
        R = _Run(L, dev, c, z, targets)
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(R.A, k)[v[0]] = v[1]
            else:
                setattr(R.A, k, v)
        with pytest.raises(L.MtnHipError):
            L.check(lib.mtn_rlosshead_fwd(C.byref(R.A), L.stream_ptr()))
        for code in (L.MTN_F32, L.MTN_BF16):
            with pytest.raises(L.MtnHipError):
                L.check(lib.mtn_rlosshead_bwd(code, C.byref(R.A), L.stream_ptr()))
        torch.cuda.synchronize()
        assert _all_nan(R.dz) and _all_nan(R.lse) and _all_nan(R.rowloss) and _all_nan(R.rowrd) and _all_nan(R.rowkl)

    for kw in (dict(rd_alpha=-0.5), dict(rd_alpha=NAN), dict(rd_alpha=float("inf")), dict(pair=(0, -1)), dict(pair=(0, 4)),
               dict(pair=(1, 3)), dict(rowkl=None), dict(V=c.V - 2), dict(V=0), dict(n_seg=5), dict(n_seg=0), dict(rows=(1, 0)),
               dict(ldz=c.V - 4), dict(pad=c.V), dict(pad=-1)):
        run(**kw)
