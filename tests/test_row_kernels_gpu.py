"""Direct parity tests, through the C ABI, of the kernels around the GEMM / attention path: the loss head (csrc/losshead.hip),
Adam / chunked Adam / the Noam tick, the grouped cast and the grouped transpose (csrc/elementwise.hip, common.h) and the
inference generator's log-softmax (csrc/select.hip).  Each against a float64 reference on the CPU (tests/row_refs.py, validated
without a GPU by tests/test_row_refs.py), outputs pre-filled with NaN or a sentinel.

Where the bounds come from (none was obtained by running a kernel):
  loss head   the kernel is float32 with __expf / __logf.  The SAME closed form evaluated in float32 with torch on the CPU
              (row_refs.closed_form_f32) against the float64 composed reference, worst over row_refs.loss_cases(), measures
                  lse 2.15e-6 absolute | rowloss 8.54e-7 of the case's largest |rowloss| | dlogits 2.03e-6 of max |ref|
              (row_refs.CPU_F32_*; tests/test_row_refs.py re-measures them).  The kernel gets 4x each - fast-math intrinsics and
              another summation order: 8.6e-6 | 3.42e-6 | 8.12e-6, all far below the 1e-4 tests/test_model_gpu.py::
              test_fused_loss_head_matches_composed_loss allows a float32 loss.  Logits with a common offset of +-50 (lse ~ 58,
              half an ulp is 1.9e-6) cost float32 no more than N(0, 8^2) logits do (lse ~ 36): one set of bounds, all cases kept.
              bfloat16 dlogits are ONE rounding of the float32 value x, |x - ref| <= d: |bf16(x) - bf16(ref)| <= |x - ref| +
              ulp(x) / 2 + ulp(ref) / 2 <= d + 1 bfloat16 ulp of the reference element (x and ref in one binade).
  Adam        adam_update is four fmas, one sqrt, one division on coefficients (lr / bc1, rsqrt(bc2)) that are one or two roundings
              each: a few float32 ulps (6e-8) per quantity and step, plus the float betas of the C ABI (1 - 0.98f is 0.02 to
              9.5e-7).  tests/test_kernels_gpu.py::test_gemm_tt_table_form states that as 1e-5 relative (to the largest) on m, v
              and 2e-6 * max(1, max |p|) absolute on p: reused here.  Copies and the three forms of the kernel: bit equality.
  Noam        state[0] exact.  lr = factor * rsqrt(model_size) * min(rsqrt(step), step * warmup^-1.5): three float32 factors good to
              a few ulps each and two products: 1e-6 relative.  1 - beta^step carries a few ulps of 1 absolute: 4 * 2^-24, i.e.
              relative 4 * 2^-24 / (1 - beta^step) (1.2e-5 for beta2 at step 1, 2.4e-6 for beta1, shrinking with the step).
  log-softmax 4x what torch.log_softmax does in float32 on the CPU against float64 on the same inputs without a common offset:
              3.82e-6 (half an ulp of the -80 of a dominant-logit row; row_refs.CPU_F32_LSM_ABS) -> 1.53e-5 absolute.  With a common
              offset of +-1e4 the kernel forms lse = max + log(sum) ~ 1e4 in float32, where the spacing is 2^-10: that rounding adds
              at most 2^-11; x - max and x - lse are exact there (both operands on the 2^-10 grid, small difference).
  casts, transposes: bit equality.
"""
import ctypes as C
import math

import pytest
import torch

from tests import row_refs as rr
from tests.util import absmax, relmax

pytestmark = pytest.mark.gpu

LSE_ABS = 4 * rr.CPU_F32_LSE_ABS                  # 8.6e-6
ROWLOSS_REL = 4 * rr.CPU_F32_ROWLOSS_REL          # 3.42e-6 of the case's largest |rowloss|
DLOGITS_REL = 4 * rr.CPU_F32_DLOGITS_REL          # 8.12e-6 of max |ref dlogits|
assert max(LSE_ABS, ROWLOSS_REL, DLOGITS_REL) < 1e-4          # the ceiling: test_fused_loss_head_matches_composed_loss, float32
ADAM_MV_REL, ADAM_P_ABS = 1e-5, 2e-6              # test_gemm_tt_table_form
NOAM_LR_REL, NOAM_BC_ABS = 1e-6, 4 * 2.0 ** -24
LSM_ABS = 4 * rr.CPU_F32_LSM_ABS                  # 1.53e-5
LSM_OFFSET_ABS = 2.0 ** -11                       # rounding of lse ~ 1e4 to the float32 grid there
NAN = float("nan")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def hip():
    from mtn_amd import lib as L
    return L, L.load()


def _bits(t):
    """integer view: equality of bits (tells -0.0 from 0.0, compares NaN sentinels)"""
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _all_nan(t):
    return bool(torch.isnan(t).all())


# ------------------------------------------------------------------------------------------ loss head
LOSS_CASES = rr.loss_cases()
PAD_SENTINEL = 1e30                               # in the padding columns of the logits: a kernel that read them would show it


class _LossRun:
    """Device buffers of one loss-head case.  lse / rowloss carry 4 extra elements and dlogits one extra row, all NaN."""

    def __init__(self, L, dev, case, z, targets, ldd_dtype=torch.float32):
        self.case, self.rows = case, sum(case.segs)
        self.ldz, self.ldd = case.V + case.ldz_pad, case.V + case.ldd_pad
        zb = torch.full((self.rows, self.ldz), PAD_SENTINEL)
        zb[:, :case.V] = z
        self.z0 = zb
        self.z = zb.to(dev)
        self.targets = [t.to(dev) for t in targets]
        self.norm = torch.tensor(rr.NORM, device=dev)
        self.gloss = torch.tensor([rr.GLOSS], device=dev)
        self.lse = torch.full((self.rows + 4,), NAN, device=dev)
        self.rowloss = torch.full((self.rows + 4,), NAN, device=dev)
        self.dz = torch.full((self.rows + 1, self.ldd), NAN, device=dev, dtype=ldd_dtype)
        A = L.LossHeadArgs()
        A.n_seg = len(case.segs)
        for s, n in enumerate(case.segs):
            A.rows[s], A.target[s], A.norm[s], A.coef[s] = n, self.targets[s].data_ptr(), self.norm.data_ptr() + 4 * s, rr.COEF[s]
        A.V, A.ldz, A.pad, A.smoothing = case.V, self.ldz, case.pad, case.smoothing
        A.logits, A.lse, A.rowloss = self.z.data_ptr(), self.lse.data_ptr(), self.rowloss.data_ptr()
        A.gloss, A.dlogits, A.ldd = self.gloss.data_ptr(), self.dz.data_ptr(), self.ldd
        self.A = A


@pytest.mark.parametrize("idx", range(len(LOSS_CASES)), ids=[rr.loss_case_id(c) for c in LOSS_CASES])
def test_losshead_forward_and_backward(dev, hip, idx):
    """mtn_losshead_fwd / mtn_losshead_bwd (float32 and bfloat16 gradients) against the composed float64 reference: lse and
    rowloss row by row, their sum, the gradient, exact zeros where the reference zeroes (rows of <pad> targets, columns V..ldd-1),
    the <pad> column of live rows, and nothing written or changed outside."""
    L, lib = hip
    c = LOSS_CASES[idx]
    z, targets = rr.loss_inputs(c, rr.LOSS_SEED + idx)
    ref = rr.composed_loss(z, targets, c)
    R = _LossRun(L, dev, c, z, targets)
    L.check(lib.mtn_losshead_fwd(C.byref(R.A), L.stream_ptr()))
    torch.cuda.synchronize()
    n, V = R.rows, c.V
    lse, rowloss = R.lse.cpu(), R.rowloss.cpu()
    assert _all_nan(lse[n:]) and _all_nan(rowloss[n:])
    e_lse = float((lse[:n].double() - ref["lse"]).abs().max())
    big = float(ref["rowloss"].abs().max())
    e_row = float((rowloss[:n].double() - ref["rowloss"]).abs().max()) / max(big, 1e-30)
    e_sum = abs(float(rowloss[:n].double().sum()) - ref["total"])
    print(f"lse abs {e_lse:.3e} (bound {LSE_ABS:.3e})  rowloss rel {e_row:.3e} (bound {ROWLOSS_REL:.3e})  sum abs {e_sum:.3e}")
    assert e_lse <= LSE_ABS
    assert e_row <= ROWLOSS_REL
    assert e_sum <= ROWLOSS_REL * big * n                          # the sum of n rows, each within its bound
    zero = ref["zero"]
    assert bool((rowloss[:n][zero] == 0.0).all())
    if c.smoothing > 0:
        assert bool((rowloss[:n][~zero] != 0.0).all())             # a live row (the lone <pad> at a segment's row 0 included) has a loss
    assert _same_bits(R.z.cpu(), R.z0)

    dmax = float(ref["dlogits"].abs().max())
    scale = torch.cat([torch.full((m,), rr.COEF[s] / rr.NORM[s], dtype=torch.float64) for s, m in enumerate(c.segs)])
    pad_col = rr.GLOSS * scale * ref["softmax"][:, c.pad] * ref["sum_td"]        # td of the <pad> column is 0 in every row
    assert float((pad_col - ref["dlogits"][:, c.pad]).abs().max()) <= 1e-12 * dmax
    for dtype in (torch.float32, torch.bfloat16):
        if dtype == torch.bfloat16:
            R.dz = torch.full((n + 1, R.ldd), NAN, device=dev, dtype=dtype)
            R.A.dlogits = R.dz.data_ptr()
        L.check(lib.mtn_losshead_bwd(L.dtype_code(dtype), C.byref(R.A), L.stream_ptr()))
        torch.cuda.synchronize()
        dz = R.dz.cpu()
        assert _all_nan(dz[n])                                                  # the row past the last
        assert bool((_bits(dz[:n, V:]) == 0).all())                             # columns V..ldd-1: +0.0 in every row
        assert bool((dz[:n][zero] == 0.0).all())
        got = dz[:n, :V].double()
        if dtype == torch.float32:
            tol = torch.full_like(got, DLOGITS_REL * dmax)
            want = ref["dlogits"]
            want_pad = pad_col
        else:
            want = ref["dlogits"].to(torch.bfloat16).double()
            tol = rr.bf16_ulp(ref["dlogits"]) + DLOGITS_REL * dmax
            want_pad = pad_col.to(torch.bfloat16).double()
        err = (got - want).abs()
        print(f"{dtype}: dlogits worst err / bound {float((err / tol).max()):.3f}, rel to max {float(err.max()) / dmax:.3e}")
        assert bool((err <= tol).all())
        live = ~zero
        assert bool(((got[:, c.pad] - want_pad).abs()[live] <= tol[:, c.pad][live]).all())
        if c.smoothing > 0 and live.any():
            assert bool((got[:, c.pad][live] > 0).all())               # g * softmax * sum(td) > 0: never -g * eps, never 0
        assert _same_bits(R.z.cpu(), R.z0)                             # logits and their padding columns: unchanged
        assert _same_bits(R.lse.cpu()[:n], lse[:n])


def test_losshead_argument_checks(dev, hip):
    """Bad arguments raise and launch nothing: the outputs keep their NaN."""
    L, lib = hip
    c = rr.LossCase(104, (6, 5), 0, 4, "tail", 0.1, 1.0, 0.0, 1)
    z, targets = rr.loss_inputs(c, 3)

    def run(mutate, bwd_only=False):
        R = _LossRun(L, dev, c, z, targets)
        if bwd_only:
            L.check(lib.mtn_losshead_fwd(C.byref(R.A), L.stream_ptr()))
        mutate(R.A)
        if not bwd_only:
            with pytest.raises(L.MtnHipError):
                L.check(lib.mtn_losshead_fwd(C.byref(R.A), L.stream_ptr()))
        for code in (L.MTN_F32, L.MTN_BF16):
            with pytest.raises(L.MtnHipError):
                L.check(lib.mtn_losshead_bwd(code, C.byref(R.A), L.stream_ptr()))
        torch.cuda.synchronize()
        assert _all_nan(R.dz)
        if not bwd_only:
            assert _all_nan(R.lse) and _all_nan(R.rowloss)

    def set_(**kw):
        def f(A):
            for k, v in kw.items():
                setattr(A, k, v)
        return f

    def zero_rows(A):
        A.rows[1] = 0

    run(set_(V=102))                     # V % 4 != 0 (ldz = 104 still covers it)
    run(set_(V=0))
    run(set_(n_seg=5))
    run(set_(n_seg=0))
    run(zero_rows)
    run(set_(ldz=100))                   # ldz < V: rows would overlap
    run(set_(pad=104))                   # the <pad> column is read and written by index
    run(set_(pad=-1))
    run(set_(ldd=100), bwd_only=True)    # ldd < V
    run(set_(ldd=106), bwd_only=True)    # ldd % 4 != 0
    # and the unmodified arguments do run
    R = _LossRun(L, dev, c, z, targets)
    L.check(lib.mtn_losshead_fwd(C.byref(R.A), L.stream_ptr()))
    L.check(lib.mtn_losshead_bwd(L.MTN_F32, C.byref(R.A), L.stream_ptr()))
    torch.cuda.synchronize()
    assert not torch.isnan(R.rowloss[:11]).any() and not torch.isnan(R.dz[:11]).any()


# ------------------------------------------------------------------------------------------ Adam / Noam
NOAM = (128, 10, 2.0)                  # (model_size, warmup, factor): lr ~ 5.6e-3 at step 1, so that a step moves p by ~1e-2


def _tick(L, lib, state, model_size, warmup, factor):
    L.check(lib.mtn_noam_tick(state.data_ptr(), factor, model_size, warmup, rr.BETA1, rr.BETA2, L.stream_ptr()))


def _adam(L, lib, n, p, g, m, v, lp, state, gs, off=0):
    code = L.MTN_F32 if lp is None else L.dtype_code(lp.dtype)
    lp_ptr = None if lp is None else lp.data_ptr() + lp.element_size() * off
    L.check(lib.mtn_adam_step(code, n, p.data_ptr() + 4 * off, g.data_ptr() + 4 * off, m.data_ptr() + 4 * off, v.data_ptr() + 4 * off,
                              lp_ptr, state.data_ptr(), L.ptr(gs), rr.BETA1, rr.BETA2, rr.ADAM_EPS, L.stream_ptr()))


def _adam_chunks(L, lib, offs, lens, p, g, m, v, lp, state, gs):
    dev = p.device
    off_d, len_d = torch.tensor(offs, dtype=torch.int64).to(dev), torch.tensor(lens, dtype=torch.int32).to(dev)
    code = L.MTN_F32 if lp is None else L.dtype_code(lp.dtype)
    L.check(lib.mtn_adam_step_chunks(code, len(offs), off_d.data_ptr(), len_d.data_ptr(), p.data_ptr(), g.data_ptr(), m.data_ptr(),
                                     v.data_ptr(), L.ptr(lp), state.data_ptr(), L.ptr(gs), rr.BETA1, rr.BETA2, rr.ADAM_EPS,
                                     L.stream_ptr()))
    torch.cuda.synchronize()


def _check_adam(p, m, v, p64, m64, v64, what):
    e_m, e_v, e_p = relmax(m, m64), relmax(v, v64), absmax(p, p64)
    bound_p = ADAM_P_ABS * max(1.0, float(p64.abs().max()))
    print(f"{what}: m rel {e_m:.3e}  v rel {e_v:.3e} (bound {ADAM_MV_REL:.0e})  p abs {e_p:.3e} (bound {bound_p:.3e})")
    assert e_m < ADAM_MV_REL and e_v < ADAM_MV_REL
    assert e_p < bound_p


@pytest.mark.parametrize("n,lp_dtype,grad_scale", [(4, torch.bfloat16, None), (1024, torch.float32, 0.125), (4100, None, None),
                                                   (4100, torch.bfloat16, 3.0), (3 * 2 ** 20 + 8, torch.bfloat16, 0.125),
                                                   (3 * 2 ** 20 + 8, torch.float32, None)])
def test_adam_step_matches_float64_adam(dev, hip, n, lp_dtype, grad_scale):
    """Three consecutive mtn_adam_step calls, the schedule advanced by mtn_noam_tick between them, against the free-running float64
    recurrence.  3 * 2^20 + 8 elements are more float4s than 2048 workgroups x 256 lanes: the grid-stride loop iterates."""
    L, lib = hip
    p0, _, m0, v0 = rr.adam_inputs(n, 11)
    p, m, v = p0.to(dev), m0.to(dev), v0.to(dev)
    lp = None if lp_dtype is None else torch.full((n,), 7.0, device=dev, dtype=lp_dtype)
    gs = None if grad_scale is None else torch.tensor([grad_scale], device=dev)
    state = torch.zeros(8, device=dev)
    p64, m64, v64 = p0.double(), m0.double(), v0.double()
    for step in (1, 2, 3):
        g = rr.adam_inputs(n, 11 + step)[1]
        _tick(L, lib, state, *NOAM)
        _adam(L, lib, n, p, g.to(dev), m, v, lp, state, gs)
        torch.cuda.synchronize()
        st = rr.noam_state64(step, *NOAM)
        p64, m64, v64 = rr.adam_step64(p64, g.double(), m64, v64, st[1], st[2], st[3], grad_scale or 1.0)
        _check_adam(p, m, v, p64, m64, v64, f"step {step}")
        if lp is not None:
            assert _same_bits(lp, p.to(lp_dtype))               # round-to-nearest-even of the kernel's own p
    assert float(p[0]) == float(p0[0])                          # g = m = v = 0 throughout: 0 / eps


@pytest.mark.parametrize("off,n,lp_dtype", [(4, 1024, torch.bfloat16), (12, 4100, torch.bfloat16), (4100, 4, torch.float32),
                                            (12, 1028, None)])
def test_adam_step_on_a_sub_range(dev, hip, off, n, lp_dtype):
    """What FusedAdam.step_range does: the call on [off, off + n) through pointer offsets that are multiples of 4 elements but not
    of 64.  Inside: the float64 step; outside, in p, m, v and the compute-dtype copy: not a bit changes."""
    L, lib = hip
    total = off + n + 60
    p0, g0, m0, v0 = rr.adam_inputs(total, 23)
    p, g, m, v = p0.to(dev), g0.to(dev), m0.to(dev), v0.to(dev)
    lp = None if lp_dtype is None else torch.full((total,), 7.0, device=dev, dtype=lp_dtype)
    state = torch.tensor(rr.noam_state64(5, *NOAM) + [0.0] * 4, dtype=torch.float32).to(dev)
    st = [float(x) for x in state.cpu().double()[:4]]           # the float32 state the kernel reads
    _adam(L, lib, n, p, g, m, v, lp, state, None, off=off)
    torch.cuda.synchronize()
    sl = slice(off, off + n)
    p64, m64, v64 = rr.adam_step64(p0[sl].double(), g0[sl].double(), m0[sl].double(), v0[sl].double(), st[1], st[2], st[3])
    _check_adam(p[sl], m[sl], v[sl], p64, m64, v64, f"[{off}, {off + n})")
    assert not torch.equal(p[sl].cpu(), p0[sl])
    for got, was in ((p, p0), (m, m0), (v, v0), (g, g0)):
        keep = torch.ones(total, dtype=torch.bool)
        keep[sl] = got is g                                     # the gradient is read only
        assert torch.equal(_bits(got.cpu())[keep], _bits(was)[keep])
    if lp is not None:
        assert _same_bits(lp[sl], p[sl].to(lp_dtype))
        assert bool((lp[:off] == 7.0).all()) and bool((lp[off + n:] == 7.0).all())


CHUNK_LENS = [4096, 4, 1020, 8, 4092, 252, 1024, 4096, 1020, 4, 4092, 1024, 252, 8, 4096, 8, 1024, 4, 252, 4092]


@pytest.mark.parametrize("lp_dtype", [torch.bfloat16, torch.float32, None])
@pytest.mark.parametrize("gaps", [False, True], ids=["tiling", "gaps"])
def test_adam_forms_give_the_same_bits(dev, hip, lp_dtype, gaps):
    """common.h: adam_kernel and adam_chunks_kernel produce the same bits.  One mtn_adam_step over the whole range against
    mtn_adam_step_chunks over a chunk list of mixed lengths (one float4 .. 4096 elements: every way through the chunk kernel's
    clamped loads and skipped stores) that tiles it - or, with gaps, leaves holes that must stay untouched."""
    L, lib = hip
    offs, cur = [], 0
    for k, n in enumerate(CHUNK_LENS):
        offs.append(cur)
        cur += n + ((4, 8, 64)[k % 3] if gaps else 0)
    total = cur + 64                                             # slack behind the last chunk: part of the allocation, never listed
    p0, g0, m0, v0 = rr.adam_inputs(total, 31)
    state = torch.tensor(rr.noam_state64(2, *NOAM) + [0.0] * 4, dtype=torch.float32).to(dev)
    gs = torch.tensor([0.25], device=dev)
    g = g0.to(dev)
    whole = [t.to(dev) for t in (p0, m0, v0)]
    chunk = [t.to(dev) for t in (p0, m0, v0)]
    lp_w = None if lp_dtype is None else torch.full((total,), 7.0, device=dev, dtype=lp_dtype)
    lp_c = None if lp_dtype is None else torch.full((total,), 7.0, device=dev, dtype=lp_dtype)
    _adam(L, lib, total, whole[0], g, whole[1], whole[2], lp_w, state, gs)
    _adam_chunks(L, lib, offs, CHUNK_LENS, chunk[0], g, chunk[1], chunk[2], lp_c, state, gs)
    listed = torch.zeros(total, dtype=torch.bool)
    for o, n in zip(offs, CHUNK_LENS):
        listed[o:o + n] = True
    assert int(listed.sum()) == sum(CHUNK_LENS) and (gaps or bool(listed[:cur].all()))
    for w, c, was in zip(whole, chunk, (p0, m0, v0)):
        w, c = _bits(w.cpu()), _bits(c.cpu())
        assert torch.equal(c[listed], w[listed])
        assert torch.equal(c[~listed], _bits(was)[~listed])      # holes and the slack: untouched
        assert not torch.equal(w[listed], _bits(was)[listed])
    if lp_dtype is not None:
        assert torch.equal(_bits(lp_c.cpu())[listed], _bits(lp_w.cpu())[listed])
        assert bool((lp_c.cpu()[~listed] == 7.0).all())
        assert _same_bits(lp_w, whole[0].to(lp_dtype))
    assert _same_bits(g.cpu(), g0)


@pytest.mark.parametrize("name", ["cfg1_query", "small_shared"])
def test_rest_tables_tile_the_flat_buffer(dev, name):
    """Model.rest_tables builds the chunk lists of mtn_adam_step_chunks, which drops whatever a chunk holds past 4096 elements and
    cannot check a device array: every length in (0, 4096] and a multiple of 4, every offset a multiple of 4, and the chunks
    together with the covered matrices tile [0, flat.numel()) exactly once, in order."""
    from oracle import fixtures as fx
    from tests.test_model_gpu import build_model
    model = build_model(fx.GOLDEN_CONFIGS[name], torch.bfloat16, dev)
    flat, _, _ = model.flat_buffers()
    total = flat.numel()
    every = frozenset(t[0] for t in model._fusable)
    assert every
    for covered in (frozenset(), every, every - model._fusable_optional):
        (off, ln, count), _ = model.rest_tables(covered)
        off, ln = off.cpu().tolist(), ln.cpu().tolist()
        assert count == len(off) == len(ln)
        assert all(0 < n <= 4096 and n % 4 == 0 for n in ln) and all(o % 4 == 0 for o in off)
        assert off == sorted(off)
        pieces = sorted(list(zip(off, ln)) + [(o, r * c) for o, r, c in model._fusable if o in covered])
        cur = 0
        for o, n in pieces:
            assert o == cur, (o, cur)
            cur += n
        assert cur == total
        assert sum(ln) == total - sum(r * c for o, r, c in model._fusable if o in covered)


NOAM_CONFIGS = [(512, 4000, 1.0), (128, 10, 2.0)]


@pytest.mark.parametrize("model_size,warmup,factor", NOAM_CONFIGS)
def test_noam_tick_against_float64(dev, hip, model_size, warmup, factor):
    """state[0] = s - 1 written from the host, one tick: the step count exactly, the learning rate against
    oracle.mtn_oracle.noam_rate and both bias corrections against 1 - beta^s in float64 (beta: the float the C ABI carries), at the
    warm-up boundary and at the step counts of a real run."""
    L, lib = hip
    b1, b2 = (float(torch.tensor(b, dtype=torch.float32)) for b in (rr.BETA1, rr.BETA2))
    for s in (1, 2, warmup - 1, warmup, warmup + 1, 300, 10 ** 4, 10 ** 5, 2 ** 24 - 1):
        host = torch.full((8,), NAN)
        host[0] = float(s - 1)
        state = host.to(dev)
        _tick(L, lib, state, model_size, warmup, factor)
        got = state.cpu().double()
        want = rr.noam_state64(s, model_size, warmup, factor, b1, b2)
        assert float(got[0]) == float(s)
        e_lr = abs(float(got[1]) - want[1]) / want[1]
        e_b1, e_b2 = abs(float(got[2]) - want[2]), abs(float(got[3]) - want[3])
        print(f"s {s}: lr rel {e_lr:.3e} (bound {NOAM_LR_REL:.0e})  bc1 abs {e_b1:.3e}  bc2 abs {e_b2:.3e} (bound {NOAM_BC_ABS:.3e}; "
              f"relative {e_b1 / want[2]:.3e} / {e_b2 / want[3]:.3e})")
        assert e_lr <= NOAM_LR_REL
        assert e_b1 <= NOAM_BC_ABS and e_b2 <= NOAM_BC_ABS      # relative: 4 * 2^-24 / (1 - beta^s)
        assert _all_nan(got[4:])                                 # the tick owns four floats


def test_noam_300_ticks_equal_one_tick_at_300(dev, hip):
    L, lib = hip
    for cfg in NOAM_CONFIGS:
        run = torch.zeros(8, device=dev)
        for _ in range(300):
            _tick(L, lib, run, *cfg)
        one = torch.zeros(8)
        one[0] = 299.0
        one = one.to(dev)
        _tick(L, lib, one, *cfg)
        torch.cuda.synchronize()
        assert float(run[0]) == 300.0
        assert _same_bits(run.cpu(), one.cpu())


def test_adam_and_noam_argument_checks(dev, hip):
    L, lib = hip
    p0, g0, m0, v0 = rr.adam_inputs(64, 1)
    p, g, m, v = (t.to(dev) for t in (p0, g0, m0, v0))
    state = torch.tensor(rr.noam_state64(3, *NOAM) + [0.0] * 4, dtype=torch.float32).to(dev)
    for n in (0, 6, -4):
        with pytest.raises(L.MtnHipError):
            _adam(L, lib, n, p, g, m, v, None, state, None)
    with pytest.raises(L.MtnHipError):
        L.check(lib.mtn_adam_step(7, 64, p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), None, state.data_ptr(), None,
                                  rr.BETA1, rr.BETA2, rr.ADAM_EPS, L.stream_ptr()))
    with pytest.raises(L.MtnHipError):
        L.check(lib.mtn_adam_step_chunks(L.MTN_F32, 0, p.data_ptr(), p.data_ptr(), p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(),
                                         None, state.data_ptr(), None, rr.BETA1, rr.BETA2, rr.ADAM_EPS, L.stream_ptr()))
    for ms, wu in ((0, 10), (128, 0)):
        with pytest.raises(L.MtnHipError):
            _tick(L, lib, state, ms, wu, 1.0)
    torch.cuda.synchronize()
    assert _same_bits(p.cpu(), p0) and _same_bits(m.cpu(), m0) and _same_bits(v.cpu(), v0)
    assert float(state[0]) == 3.0


# ------------------------------------------------------------------------------------------ cast group
SPECIALS = [0.0, -0.0, 1e-40, -1e-40, 1.4e-45,                   # zeros, float32 subnormals
            1.9999999, -0.99999994, 255.99998,                   # round up across a binade
            1.00390625, 1.01171875, -1.00390625,                 # ties: 1 + 2^-8 (to even: down), 1 + 3 * 2^-8 (to even: up)
            float("inf"), float("-inf"), 3.4028235e38, -3.3961775e38,      # inf; the largest floats round to inf / stay finite
            9.18e-41]                                            # a float32 subnormal that is a bfloat16 subnormal
CAST_SENTINEL = 12345.0
CAST_GROUPS = {1: [1023], 3: [3, 2 ** 23 + 1, 4096], 8: [1, 3, 4, 5, 1023, 4096, 2 ** 20 + 3, 2 ** 23 + 1]}


def _cast_src(n, gen, specials=True):
    src = torch.randn(n, generator=gen)
    if specials:
        sp = torch.tensor(SPECIALS)
        k = min(n, len(sp))
        src[:k] = sp[:k]
        src[n - k:] = sp[:k].flip(0)                             # the scalar tail (n % 4 elements) gets them too
    return src


def _cast_launch(L, lib, dtype, jobs, dev):
    """jobs: [(src cpu, gate cpu | None, Dropout | None)] -> [dst cpu, 8 sentinel elements behind n]"""
    descs = (L.CastDesc * len(jobs))()
    keep, dsts = [], []
    for d, (src, gate, drop) in zip(descs, jobs):
        s = src.to(dev)
        gt = None if gate is None else gate.to(dev)
        dst = torch.full((src.numel() + 8,), CAST_SENTINEL, device=dev, dtype=dtype)
        d.n, d.src, d.dst, d.gate = src.numel(), s.data_ptr(), dst.data_ptr(), L.ptr(gt)
        d.drop = drop if drop is not None else L.Dropout(0.0, 0, None)
        keep += [s, gt]
        dsts.append(dst)
    L.check(lib.mtn_cast_group(L.dtype_code(dtype), len(jobs), descs, L.stream_ptr()))
    torch.cuda.synchronize()
    for (src, _, _), s in zip(jobs, keep[::2]):
        assert _same_bits(s.cpu(), src)
    return [d.cpu() for d in dsts]


def _check_cast(dst, want):
    n = want.numel()
    assert torch.equal(_bits(dst[:n]), _bits(want))
    assert bool((dst[n:] == CAST_SENTINEL).all())


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("group", [1, 3, 8])
@pytest.mark.parametrize("gated", [False, True], ids=["plain", "gate"])
def test_cast_group(dev, hip, dtype, group, gated):
    """mtn_cast_group without dropout: dst == src.to(dtype) bit for bit (signed zeros, subnormals, ties, values that round up across
    a binade or to inf), descriptors of very different lengths in one launch (the grid is sized by the longest: 2^23 + 1 elements
    need the grid-stride loop, the short ones idle most workgroups), the scalar tail, nothing written past n.  With a gate:
    gate <= 0 (0.0 and -0.0 included) zeroes."""
    L, lib = hip
    gen = torch.Generator().manual_seed(100 * group + gated)
    jobs = []
    for n in CAST_GROUPS[group]:
        src = _cast_src(n, gen)
        gate = None
        if gated:
            gate = torch.randn(n, generator=gen)
            gate[::7] = 0.0
            gate[3::11] = -0.0
            gate[n - 1] = 0.0 if n % 2 else 2.0
        jobs.append((src, gate, None))
    for dst, (src, gate, _) in zip(_cast_launch(L, lib, dtype, jobs, dev), jobs):
        want = src if gate is None else torch.where(gate > 0, src, torch.zeros(()))
        _check_cast(dst, want.to(dtype))


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_cast_group_dropout(dev, hip, p):
    """The dropout keep of the cast: the float32 output on ones under the same (seed, salt) gives the mask and the scale
    (one float32 factor 1 / (1 - p)); the bfloat16 output is (src * mask * scale) in float32, rounded once; a gate applies on top;
    the scalar tail continues the element index stream of the vector body."""
    L, lib = hip
    seed = torch.full((1,), 0x1234567812345678, device=dev, dtype=torch.int64)
    gen = torch.Generator().manual_seed(int(p * 100))
    ns = [2 ** 20 + 3, 1023, 5, 1027, 2 ** 20 + 7]               # 1027 = 1023 + 4, 2^20 + 7 = 2^20 + 3 + 4: the same salts below
    salts = [41, 42, 43, 42, 41]
    drops = [L.Dropout(p, s, seed.data_ptr()) for s in salts]
    ones = _cast_launch(L, lib, torch.float32, [(torch.ones(n), None, d) for n, d in zip(ns, drops)], dev)
    scale = torch.tensor(1.0) / (torch.tensor(1.0) - torch.tensor(p))         # float32, as common.h drop_init
    masks = []
    for n, o in zip(ns, ones):
        keep = o[:n] != 0
        assert bool((o[:n][keep] == scale).all()) and bool((o[n:] == CAST_SENTINEL).all())
        if n > 1000:                                             # 4 sigma of a binomial keep rate: 0.016 * 4 at n ~ 1000, 0.0005 * 4 at 2^20
            assert abs(float(keep.double().mean()) - (1 - p)) < (0.064 if n < 2000 else 0.002)
        masks.append(keep)
    assert torch.equal(masks[1], masks[3][:1023]) and torch.equal(masks[0], masks[4][:2 ** 20 + 3])    # tail = the next indices
    assert not torch.equal(masks[0][:1023], masks[1])                                                  # another salt, another mask
    srcs = [_cast_src(n, gen, specials=False) for n in ns]
    gates = [None, torch.randn(1023, generator=gen), None, None, torch.randn(ns[4], generator=gen)]
    gates[1][::5] = 0.0
    jobs = list(zip(srcs, gates, drops))
    for dtype in (torch.bfloat16, torch.float32):
        for dst, src, gate, keep in zip(_cast_launch(L, lib, dtype, jobs, dev), srcs, gates, masks):
            want = torch.where(keep, src * scale, torch.zeros(()))
            if gate is not None:
                want = torch.where(gate > 0, want, torch.zeros(()))
            _check_cast(dst, want.to(dtype))


def test_cast_argument_checks(dev, hip):
    L, lib = hip
    src = torch.ones(16, device=dev)
    dst = torch.full((16,), CAST_SENTINEL, device=dev)
    descs = (L.CastDesc * 9)()
    for d in descs:
        d.n, d.src, d.dst = 16, src.data_ptr(), dst.data_ptr()
    for count in (0, 9, -1):
        with pytest.raises(L.MtnHipError):
            L.check(lib.mtn_cast_group(L.MTN_F32, count, descs, L.stream_ptr()))
    descs[1].n = 0
    with pytest.raises(L.MtnHipError):
        L.check(lib.mtn_cast_group(L.MTN_F32, 2, descs, L.stream_ptr()))
    with pytest.raises(L.MtnHipError):
        L.check(lib.mtn_cast_f32_to_lp(L.MTN_BF16, 0, src.data_ptr(), dst.data_ptr(), L.stream_ptr()))
    with pytest.raises(L.MtnHipError):
        L.check(lib.mtn_cast_group(5, 1, descs, L.stream_ptr()))
    torch.cuda.synchronize()
    assert bool((dst == CAST_SENTINEL).all())
    L.check(lib.mtn_cast_f32_to_lp(L.MTN_F32, 16, src.data_ptr(), dst.data_ptr(), L.stream_ptr()))
    torch.cuda.synchronize()
    assert bool((dst == 1.0).all())


# ------------------------------------------------------------------------------------------ transpose group
T_SHAPES = [(64, 64), (512, 2048), (1, 1), (3, 200), (200, 3), (65, 129), (72, 136), (520, 64)]
# element offset of each block past a multiple of 8, (source, destination): 0 = 16-byte aligned in both dtypes, 4 = aligned for
# float32 only, odd = never.  Layout 0 lets the shapes that allow the vector path take it; layout 1 forces the scalar path on them
# (and aligns the ragged ones, whose partial tiles still go the scalar way).
T_ALIGN = [[(0, 0), (0, 0), (1, 3), (0, 1), (5, 0), (0, 0), (0, 0), (0, 0)],
           [(1, 0), (0, 7), (0, 0), (4, 4), (0, 4), (3, 5), (1, 0), (4, 0)]]
T_SENTINEL = 12352.0                                             # representable in bfloat16; N(0, 1) sources never hold it


def _t_layout(align):
    src_off, dst_off, cs, cd = [], [], 0, 0
    for (r, c), (a, b) in zip(T_SHAPES, align):
        cs = (cs + 7) // 8 * 8 + a
        cd = (cd + 7) // 8 * 8 + b
        src_off.append(cs); dst_off.append(cd)
        cs += r * c + 3
        cd += r * c + 5
    return src_off, dst_off, cs + 16, cd + 16


def _t_table(L, dev, which, src_off, dst_off):
    arr = (L.TransposeDesc * len(which))()
    tiles = 0
    for d, i in zip(arr, which):
        r, c = T_SHAPES[i]
        d.off, d.dst_off, d.rows, d.cols, d.tile_start = src_off[i], dst_off[i], r, c, tiles
        tiles += ((r + 63) // 64) * ((c + 63) // 64)
    raw = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)
    return raw, len(which), tiles


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("layout", [0, 1], ids=["aligned", "misaligned"])
def test_transpose_group(dev, hip, dtype, layout):
    """One mtn_transpose_group launch over eight matrices (full tiles, partial tiles, single rows / columns / elements), block
    offsets 16-byte aligned for some and odd for others: every block == .t() of its source, every other destination element keeps
    its sentinel, the source is unchanged.  Then a SUBSET table (what Model.rest_tables builds) rewrites only its own blocks."""
    L, lib = hip
    src_off, dst_off, n_src, n_dst = _t_layout(T_ALIGN[layout])
    gen = torch.Generator().manual_seed(5 + layout)
    src0 = torch.randn(n_src, generator=gen).to(dtype)
    src = src0.to(dev)
    for which in (list(range(len(T_SHAPES))), [1, 3, 6], [7], [2, 5]):
        dst = torch.full((n_dst,), T_SENTINEL, device=dev, dtype=dtype)
        raw, count, tiles = _t_table(L, dev, which, src_off, dst_off)
        L.check(lib.mtn_transpose_group(L.dtype_code(dtype), src.data_ptr(), dst.data_ptr(), raw.data_ptr(), count, tiles, L.stream_ptr()))
        torch.cuda.synchronize()
        got = dst.cpu()
        untouched = torch.ones(n_dst, dtype=torch.bool)
        for i in which:
            r, c = T_SHAPES[i]
            want = src0[src_off[i]:src_off[i] + r * c].view(r, c).t().contiguous()
            assert torch.equal(_bits(got[dst_off[i]:dst_off[i] + r * c]), _bits(want).view(-1)), (which, i)
            untouched[dst_off[i]:dst_off[i] + r * c] = False
        assert bool((got[untouched] == T_SENTINEL).all()), which
        assert _same_bits(src.cpu(), src0)
    with pytest.raises(L.MtnHipError):
        L.check(lib.mtn_transpose_group(L.dtype_code(dtype), src.data_ptr(), dst.data_ptr(), raw.data_ptr(), 0, tiles, L.stream_ptr()))
    with pytest.raises(L.MtnHipError):
        L.check(lib.mtn_transpose_group(L.dtype_code(dtype), src.data_ptr(), dst.data_ptr(), raw.data_ptr(), count, 0, L.stream_ptr()))


# ------------------------------------------------------------------------------------------ log-softmax rows
LSM_CASES = rr.lsm_cases()
LSM_SENTINEL = -777.0


@pytest.mark.parametrize("idx", range(len(LSM_CASES)), ids=[f"r{c.rows}-V{c.V}-ldx{c.ldx_pad}-ldo{c.ldo_pad}-{'in' if c.inplace else 'out'}"
                                                            f"place-o{c.offset:g}" for c in LSM_CASES])
def test_log_softmax_rows(dev, hip, idx):
    """mtn_log_softmax_rows against float64 log_softmax: a dominant logit, a large common offset, row strides wider than V, in
    place; exp(out) sums to 1; the padding columns of the output (and, out of place, the whole input) are untouched."""
    L, lib = hip
    c = LSM_CASES[idx]
    x = rr.lsm_inputs(c, rr.LSM_SEED + idx)
    ldx = c.V + c.ldx_pad
    ldo = ldx if c.inplace else c.V + c.ldo_pad
    xb0 = torch.full((c.rows, ldx), LSM_SENTINEL)
    xb0[:, :c.V] = x
    xb = xb0.to(dev)
    out = xb if c.inplace else torch.full((c.rows, ldo), LSM_SENTINEL, device=dev)
    L.check(lib.mtn_log_softmax_rows(xb.data_ptr(), c.rows, c.V, ldx, out.data_ptr(), ldo, L.stream_ptr()))
    torch.cuda.synchronize()
    got = out.cpu()
    ref = torch.log_softmax(x.double(), dim=1)
    bound = LSM_ABS + (LSM_OFFSET_ABS if c.offset != 0 else 0.0)
    err = float((got[:, :c.V].double() - ref).abs().max())
    esum = float((got[:, :c.V].double().exp().sum(1) - 1.0).abs().max())
    print(f"abs err {err:.3e} (bound {bound:.3e})  |sum exp - 1| {esum:.3e}")
    assert err <= bound
    assert esum <= math.expm1(bound)                 # every term within exp(+-bound) of its share
    assert bool((got[:, c.V:] == LSM_SENTINEL).all())
    if not c.inplace:
        assert _same_bits(xb.cpu(), xb0)
    if c.V == 1:
        assert bool((got[:, 0] == 0.0).all())


def test_log_softmax_rows_argument_checks(dev, hip):
    L, lib = hip
    x = torch.zeros(4, 8, device=dev)
    out = torch.full((4, 8), NAN, device=dev)
    for rows, V, ldx, ldo in ((0, 8, 8, 8), (4, 0, 8, 8), (4, 8, 7, 8), (4, 8, 8, 7)):
        with pytest.raises(L.MtnHipError):
            L.check(lib.mtn_log_softmax_rows(x.data_ptr(), rows, V, ldx, out.data_ptr(), ldo, L.stream_ptr()))
    torch.cuda.synchronize()
    assert _all_nan(out)
