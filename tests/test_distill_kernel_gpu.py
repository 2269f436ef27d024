"""mtn_distill_fwd / mtn_distill_bwd (csrc/losshead.hip) through the C ABI against the float64 composed reference of
tests/distill_refs.py (validated without a GPU by tests/test_distill_refs.py), outputs and guard regions pre-filled with NaN.

Where the bounds come from (none was obtained by running the kernel): the kernel is float32 with __expf / __logf.  The SAME closed form
(row maxima taken out of every term) evaluated in float32 with torch on the CPU (distill_refs.closed_form_f32) against the float64
reference, worst over distill_refs.dist_cases(), measures
    lse 2.16e-6 absolute | rowloss 1.28e-6 of the case's largest |rowloss| | rowkd 4.71e-7 of max(1, the case's largest kd) |
    dlogits 1.34e-6 of max |ref|
(distill_refs.CPU_F32_DISTILL_*; tests/test_distill_refs.py re-measures them).  The kernel gets 4x each — fast-math intrinsics and
another summation order, the margin tests/test_row_kernels_gpu.py and tests/test_ensemble_kernel_gpu.py give.  bfloat16 dlogits are ONE
rounding of the float32 value: + 1 bfloat16 ulp of the reference element (row_refs.bf16_ulp), as for the plain loss head.
Self-teacher (teacher row = student row, alpha = 1, T = 1, smoothing 0): kd = 0 and dlogits = 0 in exact arithmetic, so the same
bounds apply with nothing to be relative to: rowkd <= ROWKD (the max(1, .) floor) and |dlogits| <= DLOGITS * g * scale, the size one
probability's worth of gradient has (g scale alpha T |pS - pT| with pS, pT <= 1).
"""
import ctypes as C

import pytest
import torch

from tests import distill_refs as dr
from tests import row_refs as rr

pytestmark = pytest.mark.gpu

LSE_ABS = 4 * dr.CPU_F32_DISTILL_LSE
ROWLOSS_REL = 4 * dr.CPU_F32_DISTILL_ROWLOSS
ROWKD_REL = 4 * dr.CPU_F32_DISTILL_ROWKD
DLOGITS_REL = 4 * dr.CPU_F32_DISTILL_DLOGITS
NAN = float("nan")
PAD_SENTINEL = 1e30
CASES = dr.dist_cases()
IDS = [dr.dist_case_id(c) for c in CASES]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def hip():
    from mtn_amd import lib as L
    return L, L.load()


def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _all_nan(t):
    return bool(torch.isnan(t).all())


class _Run:
    """Device buffers of one case.  lse / rowloss / rowkd carry 4 extra elements and dlogits one extra row, all NaN; the padding columns
    of the logits and of the teacher rows hold 1e30.  ``A`` is the distillation block, ``H`` the plain loss head's on the SAME buffers."""

    def __init__(self, L, dev, case, z, targets, teachers, dtype=torch.float32, alpha=None, with_teacher=True):
        self.case, self.rows = case, sum(case.segs)
        self.ldz, self.ldq, self.ldd = case.V + case.ldz_pad, case.V + case.ldq_pad, case.V + case.ldd_pad
        zb = torch.full((self.rows, self.ldz), PAD_SENTINEL)
        zb[:, :case.V] = z
        self.z0, self.z = zb, zb.to(dev)
        self.q0, self.q = [], []
        for t in teachers:
            if t is None:
                self.q0.append(None); self.q.append(None)
                continue
            qb = torch.full((t.size(0), self.ldq), PAD_SENTINEL)
            qb[:, :case.V] = t
            self.q0.append(qb); self.q.append(qb.to(dev))
        self.targets = [t.to(dev) for t in targets]
        self.norm = torch.tensor(rr.NORM, device=dev)
        self.gloss = torch.tensor([rr.GLOSS], device=dev)
        self.lse = torch.full((self.rows + 4,), NAN, device=dev)
        self.rowloss = torch.full((self.rows + 4,), NAN, device=dev)
        self.rowkd = torch.full((self.rows + 4,), NAN, device=dev)
        self.dz = torch.full((self.rows + 1, self.ldd), NAN, device=dev, dtype=dtype)
        self.A, self.H = L.DistillHeadArgs(), L.LossHeadArgs()
        for A in (self.A, self.H):
            A.n_seg = len(case.segs)
            for s, n in enumerate(case.segs):
                A.rows[s], A.target[s], A.norm[s], A.coef[s] = n, self.targets[s].data_ptr(), self.norm.data_ptr() + 4 * s, rr.COEF[s]
            A.V, A.ldz, A.pad, A.smoothing = case.V, self.ldz, case.pad, case.smoothing
            A.logits, A.lse, A.rowloss = self.z.data_ptr(), self.lse.data_ptr(), self.rowloss.data_ptr()
            A.gloss, A.dlogits, A.ldd = self.gloss.data_ptr(), self.dz.data_ptr(), self.ldd
        for s, q in enumerate(self.q):
            if q is not None and with_teacher:
                self.A.teacher[s], self.A.ldq[s] = q.data_ptr(), self.ldq
        self.A.alpha, self.A.temperature, self.A.rowkd = case.alpha if alpha is None else alpha, case.T, self.rowkd.data_ptr()

    def new_dz(self, dev, dtype):
        self.dz = torch.full((self.rows + 1, self.ldd), NAN, device=dev, dtype=dtype)
        self.A.dlogits = self.H.dlogits = self.dz.data_ptr()

    def inputs_unchanged(self):
        return _same_bits(self.z.cpu(), self.z0) and all(q is None or _same_bits(q.cpu(), q0) for q, q0 in zip(self.q, self.q0))


@pytest.mark.parametrize("idx", range(len(CASES)), ids=IDS)
def test_distill_forward_and_backward(dev, hip, idx):
    """lse, rowloss, rowkd row by row and their sums, dlogits in float32 and bfloat16, against the float64 reference; exact zeros where
    the reference zeroes; no NaN from -inf teacher columns; guards, logits and teacher rows untouched; two launches, equal bytes."""
    L, lib = hip
    c = CASES[idx]
    z, targets, teachers = dr.dist_inputs(c, dr.DIST_SEED + idx)
    ref = dr.composed_distill(z, targets, teachers, c)
    R = _Run(L, dev, c, z, targets, teachers)
    L.check(lib.mtn_distill_fwd(C.byref(R.A), L.stream_ptr()))
    torch.cuda.synchronize()
    n, V = R.rows, c.V
    lse, rowloss, rowkd = R.lse.cpu(), R.rowloss.cpu(), R.rowkd.cpu()
    assert _all_nan(lse[n:]) and _all_nan(rowloss[n:]) and _all_nan(rowkd[n:])
    assert not torch.isnan(lse[:n]).any() and not torch.isnan(rowloss[:n]).any() and not torch.isnan(rowkd[:n]).any()
    big, bigkd = float(ref["rowloss"].abs().max()), max(1.0, float(ref["rowkd"].abs().max()))
    e_lse = float((lse[:n].double() - ref["lse"]).abs().max())
    e_row = float((rowloss[:n].double() - ref["rowloss"]).abs().max()) / max(big, 1e-30)
    e_kd = float((rowkd[:n].double() - ref["rowkd"]).abs().max()) / bigkd
    e_sum = abs(float(rowloss[:n].double().sum()) - ref["total"])
    e_kdsum = abs(float(rowkd[:n].double().sum()) - float(ref["rowkd"].sum()))
    print(f"lse abs {e_lse:.3e} (bound {LSE_ABS:.3e})  rowloss rel {e_row:.3e} (bound {ROWLOSS_REL:.3e})  rowkd rel {e_kd:.3e} "
          f"(bound {ROWKD_REL:.3e})  sum abs {e_sum:.3e}  kd sum abs {e_kdsum:.3e}")
    assert e_lse <= LSE_ABS
    assert e_row <= ROWLOSS_REL
    assert e_kd <= ROWKD_REL
    assert e_sum <= ROWLOSS_REL * big * n and e_kdsum <= ROWKD_REL * bigkd * n          # n rows, each within its bound
    zero, mask = ref["zero"], dr.kd_rows_mask(c, targets)
    assert bool((rowloss[:n][zero] == 0.0).all())
    assert bool((_bits(rowkd[:n][~mask]) == 0).all())                                    # <pad> targets, segments without a teacher: +0.0
    assert R.inputs_unchanged()

    dmax = float(ref["dlogits"].abs().max())
    for dtype in (torch.float32, torch.bfloat16):
        if dtype == torch.bfloat16:
            R.new_dz(dev, dtype)
        L.check(lib.mtn_distill_bwd(L.dtype_code(dtype), C.byref(R.A), L.stream_ptr()))
        torch.cuda.synchronize()
        dz = R.dz.cpu()
        assert _all_nan(dz[n])
        assert bool((_bits(dz[:n, V:]) == 0).all())                                      # columns V..ldd-1: +0.0 in every row
        assert bool((dz[:n][zero] == 0.0).all())
        got = dz[:n, :V].double()
        assert not torch.isnan(got).any()
        if dtype == torch.float32:
            want, tol = ref["dlogits"], torch.full_like(got, DLOGITS_REL * dmax)
        else:
            want, tol = ref["dlogits"].to(torch.bfloat16).double(), rr.bf16_ulp(ref["dlogits"]) + DLOGITS_REL * dmax
        err = (got - want).abs()
        print(f"{dtype}: dlogits worst err / bound {float((err / tol).max()):.3f}, rel to max {float(err.max()) / max(dmax, 1e-30):.3e}")
        assert bool((err <= tol).all())
        again = torch.full_like(R.dz, NAN)
        R.A.dlogits = again.data_ptr()
        L.check(lib.mtn_distill_bwd(L.dtype_code(dtype), C.byref(R.A), L.stream_ptr()))
        torch.cuda.synchronize()
        assert _same_bits(again.cpu(), dz)
        assert R.inputs_unchanged() and _same_bits(R.lse.cpu()[:n], lse[:n])
    L.check(lib.mtn_distill_fwd(C.byref(R.A), L.stream_ptr()))
    torch.cuda.synchronize()
    assert _same_bits(R.lse.cpu(), lse) and _same_bits(R.rowloss.cpu(), rowloss) and _same_bits(R.rowkd.cpu(), rowkd)


BITWISE = [i for i, c in enumerate(CASES) if c.alpha == 0] + [i for i, c in enumerate(CASES) if c.alpha == 0.3][::3]


@pytest.mark.parametrize("idx", BITWISE, ids=[IDS[i] for i in BITWISE])
@pytest.mark.parametrize("how", ["alpha0", "null_teacher"])
def test_without_soft_term_the_bits_are_the_loss_heads(dev, hip, idx, how):
    """alpha = 0 with the teachers given, and alpha = 0.3 with every teacher NULL: lse, rowloss and dlogits (float32 and bfloat16) equal
    mtn_losshead_fwd / _bwd on the same buffers bit for bit, rowkd is +0.0, and NaN-filled teacher rows show that nothing read them."""
    L, lib = hip
    c = CASES[idx]
    z, targets, teachers = dr.dist_inputs(c, dr.DIST_SEED + idx)
    poison = [None if t is None else torch.full_like(t, NAN) for t in teachers]
    R = _Run(L, dev, c, z, targets, poison, alpha=0.0 if how == "alpha0" else 0.3, with_teacher=how == "alpha0")
    n = R.rows
    L.check(lib.mtn_losshead_fwd(C.byref(R.H), L.stream_ptr()))
    torch.cuda.synchronize()
    lse_h, row_h = R.lse.clone(), R.rowloss.clone()
    R.lse.fill_(NAN); R.rowloss.fill_(NAN)
    L.check(lib.mtn_distill_fwd(C.byref(R.A), L.stream_ptr()))
    torch.cuda.synchronize()
    assert _same_bits(R.lse, lse_h) and _same_bits(R.rowloss, row_h)
    assert bool((_bits(R.rowkd[:n]) == 0).all()) and _all_nan(R.rowkd[n:])
    for dtype in (torch.float32, torch.bfloat16):
        R.new_dz(dev, dtype)
        L.check(lib.mtn_losshead_bwd(L.dtype_code(dtype), C.byref(R.H), L.stream_ptr()))
        torch.cuda.synchronize()
        dz_h = R.dz
        R.new_dz(dev, dtype)
        L.check(lib.mtn_distill_bwd(L.dtype_code(dtype), C.byref(R.A), L.stream_ptr()))
        torch.cuda.synchronize()
        assert _same_bits(R.dz, dz_h)


SELF = [i for i, c in enumerate(CASES) if c.V in (8, 260, 3000, 3004)][::2]


@pytest.mark.parametrize("idx", SELF, ids=[IDS[i] for i in SELF])
def test_self_teacher_has_no_soft_loss_and_no_gradient(dev, hip, idx):
    L, lib = hip
    c = CASES[idx]._replace(alpha=1.0, T=1.0, smoothing=0.0)
    z, targets, _ = dr.dist_inputs(c, dr.DIST_SEED + idx)
    teachers, base = [], 0
    for s, m in enumerate(c.segs):
        teachers.append(z[base:base + m].clone() if s in c.teach else None)
        base += m
    R = _Run(L, dev, c, z, targets, teachers)
    L.check(lib.mtn_distill_fwd(C.byref(R.A), L.stream_ptr()))
    L.check(lib.mtn_distill_bwd(L.MTN_F32, C.byref(R.A), L.stream_ptr()))
    torch.cuda.synchronize()
    n = R.rows
    mask = dr.kd_rows_mask(c, targets)
    kd, dz = R.rowkd.cpu()[:n], R.dz.cpu()[:n, :c.V].double()
    gs = rr.GLOSS * dr.seg_scale(c)
    print(f"max |kd| {float(kd.abs().max()):.3e} (bound {ROWKD_REL:.3e})  max |dz| / (g scale) {float((dz.abs().max(1).values / gs)[mask].max()) if mask.any() else 0:.3e}")
    assert bool((kd.abs() <= ROWKD_REL).all())
    assert bool((dz.abs()[mask] <= (DLOGITS_REL * gs).unsqueeze(1)[mask]).all())
    # alpha = 1 leaves the <pad>-target rows of a distilled segment without any loss
    dist = dr.seg_distilled(c)
    assert bool((R.rowloss.cpu()[:n][dist & ~mask] == 0).all()) and bool((dz[dist & ~mask] == 0).all())


def test_distill_argument_checks_leave_the_guards(dev, hip):
    """Bad arguments raise and launch nothing: every output keeps its NaN."""
    L, lib = hip
    c = dr.DistCase(104, (6, 5), (0,), 0, 12, 4, "tail", 0.1, 2.0, 0.5, "logp", 1, 1.0, 0.0)
    z, targets, teachers = dr.dist_inputs(c, 3)

    def run(**kw):
        R = _Run(L, dev, c, z, targets, teachers)
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(R.A, k)[v[0]] = v[1]
            else:
                setattr(R.A, k, v)
        with pytest.raises(L.MtnHipError):
            L.check(lib.mtn_distill_fwd(C.byref(R.A), L.stream_ptr()))
        for code in (L.MTN_F32, L.MTN_BF16):
            with pytest.raises(L.MtnHipError):
                L.check(lib.mtn_distill_bwd(code, C.byref(R.A), L.stream_ptr()))
        torch.cuda.synchronize()
        assert _all_nan(R.dz) and _all_nan(R.lse) and _all_nan(R.rowloss) and _all_nan(R.rowkd)

    for kw in (dict(alpha=-0.5), dict(alpha=1.01), dict(alpha=NAN), dict(temperature=0.0), dict(temperature=-2.0), dict(temperature=float("inf")),
               dict(temperature=NAN), dict(ldq=(0, 100)), dict(ldq=(0, 106)), dict(V=102), dict(V=0), dict(n_seg=5), dict(n_seg=0),
               dict(rows=(1, 0)), dict(ldz=100), dict(pad=104), dict(pad=-1)):
        run(**kw)
    R = _Run(L, dev, c, z, targets, teachers)
    for ldd in (100, 106):
        R.A.ldd = ldd
        with pytest.raises(L.MtnHipError):
            L.check(lib.mtn_distill_bwd(L.MTN_F32, C.byref(R.A), L.stream_ptr()))
    R.A.ldd = R.ldd
    torch.cuda.synchronize()
    assert _all_nan(R.dz)
    L.check(lib.mtn_distill_fwd(C.byref(R.A), L.stream_ptr()))                            # and the unmodified arguments do run
    L.check(lib.mtn_distill_bwd(L.MTN_F32, C.byref(R.A), L.stream_ptr()))
    torch.cuda.synchronize()
    assert not torch.isnan(R.rowloss[:11]).any() and not torch.isnan(R.dz[:11]).any() and lib.mtn_version() >= 123
