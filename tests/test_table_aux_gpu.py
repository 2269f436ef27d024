"""Direct parity tests of the table launch's optimiser front tiles: mtn_gemm_tt_table_aux (csrc/gemm.hip: tt_front_tile, the
BiasAdam block of tt128_tile, the host staging code), through the C ABI with hand-built mtn_tt_aux / mtn_tt_ln_unit /
mtn_gemm_problem / mtn_adam_fuse.  References on the host: tests/table_refs.py (validated without a GPU by
tests/test_table_refs.py) and tests/row_refs.py.

For every range a launch updates, four checks (_check_flat):
  1 the stored gradient   LayerNorm slots: the bits of mtn_layernorm_bwd_finalize on the same partial rows, the bits of
                          table_refs.finalize_f32 (IEEE float32 additions in the kernel's order), and within
                          table_refs.finalize_bound (derived: (ceil(nparts / 64) + 11) * 2^-24 * sum |partial|) of the float64 sum.
                          Linear biases: rowsum_out against the float64 row sums of the bf16-rounded operand, relmax < 1e-4
                          (tests/test_kernels_gpu.py::test_gemm_tt_table_form).  Chunks: g is read only.
  2 Adam against float64  row_refs.adam_step64 on the kernel's own stored gradient (times grad_scale) and the float32 state the
                          kernel reads; ADAM_MV_REL = 1e-5 on m, v and ADAM_P_ABS = 2e-6 * max(1, max |p|) on p
                          (tests/test_row_kernels_gpu.py, from test_gemm_tt_table_form).
  3 Adam against the separate pass   p, m, v and the compute-dtype copy have the bits mtn_adam_step / mtn_adam_step_chunks
                          produce on clones over the same range with the same stored gradient; the copy is bf16(p) of the kernel's p.
  4 everything else       no bit changes in p, m, v, the copy (sentinel 7.0) and - outside the stored gradients - g.
No bound here was obtained by running a kernel; none is new except finalize_bound.
"""
import ctypes as C

import pytest
import torch

from tests import row_refs as rr
from tests import table_refs as tr
from tests.test_row_kernels_gpu import ADAM_MV_REL, ADAM_P_ABS, CHUNK_LENS, NOAM, _adam, _adam_chunks, _bits, _same_bits, _tick
from tests.util import absmax, lp_round, relmax

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
LP_SENTINEL = 7.0
GEMM_REL = 1e-4                        # test_gemm_tt_table_form: row sums and plain C against float64 on the bf16-rounded operands
NAN = float("nan")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def hip():
    from mtn_amd import lib as L
    return L, L.load()


def _state(dev, step):
    return torch.tensor(rr.noam_state64(step, *NOAM) + [0.0] * 4, dtype=torch.float32).to(dev)


def _gs(dev, grad_scale):
    return None if grad_scale is None else torch.tensor([grad_scale], device=dev)


class _Flat:
    """The flat fp32 buffers of a launch (row_refs.adam_inputs), their originals on the host, and a compute-dtype copy filled with
    the sentinel (allocated also when it is not passed to the launch: it must stay untouched then)."""

    def __init__(self, dev, n, seed):
        self.n = n
        self.p0, self.g0, self.m0, self.v0 = rr.adam_inputs(n, seed)
        self.p, self.g, self.m, self.v = (t.to(dev) for t in (self.p0, self.g0, self.m0, self.v0))
        self.lp = torch.full((n,), LP_SENTINEL, device=dev, dtype=BF16)

    def g_ptr(self, off):
        return self.g.data_ptr() + 4 * off


class _Problem:
    """One parameter-gradient problem C[M, N] = A^T B (A [K, M], B [K, N] bf16), its float64 reference on the bf16-rounded
    operands, and optionally the optimiser epilogue on a weight of its own (outside the flat buffers) with its free-running
    float64 Adam."""

    def __init__(self, L, dev, M, N, K, seed, rowsum=0, fuse=None, lpT=None, write_grad=0):
        """rowsum: device address or 0.  fuse: (state, gs) or None.  lpT: None | 'aligned' | 'ldT' | 'base'."""
        self.M, self.N, self.K, self.dev = M, N, K, dev
        self.A = torch.empty(K, M, device=dev, dtype=BF16)
        self.B = torch.empty(K, N, device=dev, dtype=BF16)
        self.out = torch.full((M, N), NAN, device=dev)
        p = L.GemmProblem()
        p.A, p.B, p.lda, p.ldb, p.M, p.N, p.K, p.a_trans, p.b_trans, p.gate_scale = self.A.data_ptr(), self.B.data_ptr(), M, N, M, N, K, 1, 1, 1.0
        p.out_f32, p.ldc, p.rowsum_out = self.out.data_ptr(), N, rowsum
        self.p, self.f = p, None
        self.operands(seed)
        if fuse is not None:
            state, gs = fuse
            gen = torch.Generator().manual_seed(seed + 7)
            self.w0, self.m0, self.v0 = torch.randn(M, N, generator=gen), 0.01 * torch.randn(M, N, generator=gen), 1e-4 * torch.rand(M, N, generator=gen)
            self.w, self.m, self.v = self.w0.to(dev), self.m0.to(dev), self.v0.to(dev)
            self.w64, self.m64, self.v64 = self.w0.double(), self.m0.double(), self.v0.double()
            self.lp = torch.full((M, N), LP_SENTINEL, device=dev, dtype=BF16)
            f = L.AdamFuse()
            f.p, f.m, f.v, f.p_lp = self.w.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self.lp.data_ptr()
            self.lpT, self.r0 = None, 0
            if lpT is not None:
                # the transposed copy as a row block [r0, r0 + M) of a taller weight: 'aligned' (16-byte base, ldT % 8 == 0: the LDS
                # epilogue), 'ldT' (ldT = M + 4) and 'base' (base 2 elements past a 16-byte boundary): the generic epilogue
                rows_total, self.r0 = {"aligned": (M + 64, 24), "ldT": (M + 4, 0), "base": (M + 8, 2)}[lpT]
                self.lpT = torch.full((N, rows_total), LP_SENTINEL, device=dev, dtype=BF16)
                f.p_lpT, f.ldT = self.lpT.data_ptr() + 2 * self.r0, rows_total
            f.write_grad, f.state, f.grad_scale, f.beta1, f.beta2, f.eps = write_grad, state.data_ptr(), L.ptr(gs), rr.BETA1, rr.BETA2, rr.ADAM_EPS
            self.f = f
            p.adam = C.pointer(f)

    def operands(self, seed):
        """new operand CONTENTS in the same device buffers"""
        gen = torch.Generator().manual_seed(seed)
        a, b = torch.randn(self.M, self.K, generator=gen), torch.randn(self.N, self.K, generator=gen)
        self.A.copy_(a.t().contiguous().to(BF16))
        self.B.copy_(b.t().contiguous().to(BF16))
        ar, br = lp_round(a, BF16).double(), lp_round(b, BF16).double()
        self.ref, self.rsum = ar @ br.t(), ar.sum(1)

    def check_plain(self):
        e = relmax(self.out, self.ref)
        assert e < GEMM_REL, e

    def check_weight(self, st, gscale, what):
        """One more step of the free-running float64 Adam on the float64 gradient; the compute-dtype copies exactly bf16(p)."""
        self.w64, self.m64, self.v64 = rr.adam_step64(self.w64, self.ref, self.m64, self.v64, st[1], st[2], st[3], gscale)
        errs = _adam_errs(self.w.cpu(), self.m.cpu(), self.v.cpu(), self.w64, self.m64, self.v64, what)
        assert torch.equal(_bits(self.lp), _bits(self.w.to(BF16)))
        if self.lpT is not None:
            r0, M = self.r0, self.M
            assert torch.equal(_bits(self.lpT[:, r0:r0 + M]), _bits(self.w.to(BF16).t()))
            rest = torch.cat([self.lpT[:, :r0], self.lpT[:, r0 + M:]], dim=1)
            assert bool((rest == LP_SENTINEL).all())                  # nothing outside the block was touched
        if self.f.write_grad:
            assert relmax(self.out, self.ref) < GEMM_REL
        else:
            assert bool(torch.isnan(self.out).all())                  # the gradient never went to memory
        return errs

    def weight_untouched(self):
        return (_same_bits(self.w.cpu(), self.w0) and _same_bits(self.m.cpu(), self.m0) and _same_bits(self.v.cpu(), self.v0)
                and bool((self.lp == LP_SENTINEL).all()) and (self.lpT is None or bool((self.lpT == LP_SENTINEL).all())))


def _adam_errs(p, m, v, p64, m64, v64, what):
    """The project's Adam bars (ADAM_MV_REL on m, v relative to the largest; ADAM_P_ABS * max(1, max |p|) on p): asserted, and
    returned as (m, v, p / bound) for _report to print."""
    e_m, e_v, e_p = relmax(m, m64), relmax(v, v64), absmax(p, p64)
    bound_p = ADAM_P_ABS * max(1.0, float(p64.abs().max()))
    assert e_m < ADAM_MV_REL and e_v < ADAM_MV_REL, (what, e_m, e_v)
    assert e_p < bound_p, (what, e_p, bound_p)
    return e_m, e_v, e_p / bound_p


def _report(what, errs):
    if not errs:
        print(f"{what}: no range is updated")
        return
    e_m, e_v, e_p = (max(e[k] for e in errs) for k in range(3))
    print(f"{what}: worst of {len(errs)} ranges: m rel {e_m:.3e}  v rel {e_v:.3e} (bar {ADAM_MV_REL:.0e})  p abs / bar {e_p:.3f} "
          f"(bar {ADAM_P_ABS:.0e} * max(1, max |p|))")


def _aux(L, flat, state, gs, ln=(), chunks=(), bias_adam=0, with_lp=True):
    """mtn_tt_aux over `flat`.  ln: [(device partial rows, nparts, table_refs.LnSlot)]; chunks: [table_refs.Chunk].  Returns the
    struct and what it points to on the host."""
    aux = L.TtAux()
    aux.p, aux.g, aux.m, aux.v, aux.lp = flat.p.data_ptr(), flat.g.data_ptr(), flat.m.data_ptr(), flat.v.data_ptr(), (flat.lp.data_ptr() if with_lp else 0)
    aux.n_flat = flat.n
    units = (L.TtLnUnit * max(1, len(ln)))()
    for u, (part, nparts, s) in zip(units, ln):
        u.partial, u.nparts, u.d, u.a_off, u.b_off = part.data_ptr(), nparts, s.d, s.a_off, s.b_off
    offs = (C.c_long * max(1, len(chunks)))(*[c.off for c in chunks])
    lens = (C.c_int * max(1, len(chunks)))(*[c.len for c in chunks])
    aux.n_ln, aux.n_chunks = len(ln), len(chunks)
    if ln:
        aux.ln = C.cast(units, C.POINTER(L.TtLnUnit))
    if chunks:
        aux.chunk_off, aux.chunk_len = C.cast(offs, C.POINTER(C.c_long)), C.cast(lens, C.POINTER(C.c_int))
    aux.bias_adam, aux.state, aux.grad_scale = bias_adam, state.data_ptr(), L.ptr(gs)
    aux.beta1, aux.beta2, aux.eps = rr.BETA1, rr.BETA2, rr.ADAM_EPS
    return aux, (units, offs, lens)


def _launch(L, lib, probs, aux):
    arr = (L.GemmProblem * len(probs))(*[q.p for q in probs])
    L.check(lib.mtn_gemm_tt_table_aux(L.MTN_BF16, len(probs), arr, None if aux is None else C.byref(aux), L.stream_ptr()))


def _dummy(L, dev):
    """Every launch needs a dW problem: the smallest one, output outside the flat buffers."""
    return _Problem(L, dev, 8, 8, 8, 3)


def _ln_partials(dev, cases, seed):
    """[(host rows [nparts, 2d], device rows with one more row of 1e30 behind them: a kernel that read it would show it)]"""
    out = []
    for i, (d, nparts) in enumerate(cases):
        x = tr.partials(nparts, 2 * d, seed + i)
        out.append((x, torch.cat([x, torch.full((1, 2 * d), 1e30)]).to(dev)))
    return out


def _check_ln_gradients(L, lib, dev, flat, slots, cases, parts):
    """Check 1 for LayerNorm slots.  Returns the worst |stored - float64 sum| / finalize_bound."""
    descs = (L.LnFinalizeDesc * len(cases))()
    outs = []
    for dsc, (d, nparts), (_, xd) in zip(descs, cases, parts):
        da, db = torch.full((d,), NAN, device=dev), torch.full((d,), NAN, device=dev)
        dsc.partial, dsc.nparts, dsc.d, dsc.da2, dsc.db2 = xd.data_ptr(), nparts, d, da.data_ptr(), db.data_ptr()
        outs.append((da, db))
    L.check(lib.mtn_layernorm_bwd_finalize(len(cases), descs, L.stream_ptr()))
    torch.cuda.synchronize()
    g = flat.g.cpu()
    worst = 0.0
    for s, (d, nparts), (x, xd), (da, db) in zip(slots, cases, parts, outs):
        got = torch.cat([g[s.a_off:s.a_off + d], g[s.b_off:s.b_off + d]])
        assert _same_bits(got, torch.cat([da, db]).cpu()), (d, nparts)             # the finalize kernel's bits: unscaled
        assert _same_bits(got, tr.finalize_f32(x)), (d, nparts)                    # ... which are the host emulation's
        frac = float(((got.double() - tr.finalize_f64(x)).abs() / tr.finalize_bound(x)).max())
        assert frac <= 1.0, (d, nparts, frac)
        worst = max(worst, frac)
        assert _same_bits(xd.cpu()[:nparts], x) and bool((xd[nparts] == 1e30).all())
    return worst


def _check_flat(L, lib, flat, state, gs, updated, chunks, stored, with_lp, what):
    """Checks 2, 3 and 4 on the flat buffers after ONE launch from their original contents.  updated: [(off, n)] of LayerNorm
    and bias ranges; chunks: [table_refs.Chunk] (updated too); stored: bool mask of where the launch stores a gradient."""
    dev = flat.p.device
    torch.cuda.synchronize()
    p, g, m, v, lp = (t.cpu() for t in (flat.p, flat.g, flat.m, flat.v, flat.lp))
    st = [float(x) for x in state.cpu().double()[:4]]                # the float32 state the kernel reads
    gscale = 1.0 if gs is None else float(gs)
    ranges = list(updated) + [(c.off, c.len) for c in chunks]
    listed = torch.zeros(flat.n, dtype=torch.bool)
    errs = []
    for off, n in ranges:
        sl = slice(off, off + n)
        assert not bool(listed[sl].any())
        listed[sl] = True
        p64, m64, v64 = rr.adam_step64(flat.p0[sl].double(), g[sl].double(), flat.m0[sl].double(), flat.v0[sl].double(), st[1], st[2], st[3], gscale)
        errs.append(_adam_errs(p[sl], m[sl], v[sl], p64, m64, v64, f"{what} [{off}, {off + n})"))
        assert not torch.equal(p[sl], flat.p0[sl])
        if with_lp:
            assert _same_bits(lp[sl], p[sl].to(BF16))
    _report(what, errs)
    # 3: the separate pass on clones, with the launch's own stored gradient
    P, M, V = flat.p0.to(dev), flat.m0.to(dev), flat.v0.to(dev)
    LP = torch.full((flat.n,), LP_SENTINEL, device=dev, dtype=BF16) if with_lp else None
    for off, n in updated:
        _adam(L, lib, n, P, flat.g, M, V, LP, state, gs, off=off)
    if chunks:
        _adam_chunks(L, lib, [c.off for c in chunks], [c.len for c in chunks], P, flat.g, M, V, LP, state, gs)
    torch.cuda.synchronize()
    assert _same_bits(P.cpu(), p) and _same_bits(M.cpu(), m) and _same_bits(V.cpu(), v)
    if with_lp:
        assert _same_bits(LP.cpu(), lp)
    # 4: nothing else changed
    for got, was in ((p, flat.p0), (m, flat.m0), (v, flat.v0)):
        assert torch.equal(_bits(got)[~listed], _bits(was)[~listed])
    assert torch.equal(_bits(g)[~stored], _bits(flat.g0)[~stored])
    assert bool((lp[~listed] == LP_SENTINEL).all()) if with_lp else bool((lp == LP_SENTINEL).all())
    return errs


# ------------------------------------------------------------------------------------------ LayerNorm units
# (d, nparts).  2d = 16: a unit with 240 idle threads; 192: one unit; 272: the gain | bias boundary inside unit 0 and a second unit
# of 16 columns, all bias; 1024: the boundary on a unit edge; 1280: five units, the boundary inside the third.  nparts: the first row
# count that enters each of the three summation loops (17 is the tail's second round, 49 the stride-64 loop, 113 the stride-128
# loop), and the values either side.  Every width meets one nparts >= 113 and one <= 17.
LN_CASES = [(8, 1), (8, 300), (96, 16), (96, 129), (136, 17), (136, 65), (136, 113), (512, 16), (512, 49), (512, 300), (640, 1), (640, 17),
            (640, 129)]


@pytest.mark.parametrize("grad_scale", [None, 0.25], ids=["noscale", "scale0.25"])
def test_layernorm_units(dev, hip, grad_scale):
    """13 LayerNorms, 37 units (front padded to 40) in one launch: the four checks; the stored gradient is the UNSCALED sum."""
    L, lib = hip
    assert {d for d, _ in LN_CASES} == {8, 96, 136, 512, 640} and {n for _, n in LN_CASES} == {1, 16, 17, 49, 65, 113, 129, 300}
    for d in (8, 96, 136, 512, 640):
        ns = [n for dd, n in LN_CASES if dd == d]
        assert min(ns) <= 17 and max(ns) >= 113
    assert tr.front_units([d for d, _ in LN_CASES], 0) == (37, 40)
    lay = tr.build_layout(7, ln_widths=[d for d, _ in LN_CASES])
    flat = _Flat(dev, lay.n_flat, 41)
    parts = _ln_partials(dev, LN_CASES, 500)
    state, gs = _state(dev, 2), _gs(dev, grad_scale)
    dummy = _dummy(L, dev)
    aux, keep = _aux(L, flat, state, gs, ln=[(xd, n, s) for (_, xd), (_, n), s in zip(parts, LN_CASES, lay.ln)])
    _launch(L, lib, [dummy], aux)
    torch.cuda.synchronize()
    worst = _check_ln_gradients(L, lib, dev, flat, lay.ln, LN_CASES, parts)
    print(f"finalize: worst |stored - float64| / finalize_bound = {worst:.3f}")
    _check_flat(L, lib, flat, state, gs, lay.ranges("ln"), [], lay.masks["ln"], True, "LayerNorm Adam")
    dummy.check_plain()


# ------------------------------------------------------------------------------------------ chunks
@pytest.mark.parametrize("with_lp", [True, False], ids=["copy", "nocopy"])
@pytest.mark.parametrize("front", ["20chunks", "2units+14chunks", "5units+2040chunks"])
def test_chunks(dev, hip, front, with_lp):
    """The chunk list of test_adam_forms_give_the_same_bits with holes.  20 chunks and no LayerNorm: the front is padded to 24, the
    four padding units do nothing (and the LayerNorm slot of the layout, not listed, is untouched).  One LayerNorm of two units and
    14 chunks: exactly 16 front tiles, no padding.  One LayerNorm of five units and 2040 chunks: 2045 front tiles padded to 2048,
    four times what the chip holds at once (two workgroups on each of 256 CUs), and the first padding unit has the grid index of the
    first chunk's unit modulo 8, i.e. its XCD and its L2.  A padding unit that repeated that chunk's update would start long after
    the update has retired, read its results and apply it a second time; among 24 front tiles, all resident at once, or from
    another XCD (whose L2 need not see the first update's stores before the kernel ends) it reads the same inputs and writes the
    same bits, which no check can tell from doing nothing.  The chunks' gradient is read only."""
    L, lib = hip
    many = front == "5units+2040chunks"
    lay = tr.build_layout(6, ln_widths=(640,), chunk_lens=tr.MANY_CHUNKS) if many else tr.build_layout(6, ln_widths=(136,), chunk_lens=CHUNK_LENS)
    flat = _Flat(dev, lay.n_flat, 43)
    state, gs = _state(dev, 2), _gs(dev, 0.25)
    dummy = _dummy(L, dev)
    if front == "20chunks":
        chunks, ln_cases, ln_slots = lay.chunks, [], []
        assert tr.front_units((), len(chunks)) == (0, 24)
    elif many:
        chunks, ln_cases, ln_slots = lay.chunks, [(640, 17)], lay.ln
        assert tr.front_units((640,), len(chunks)) == (5, 2048) and (5 + len(chunks)) % 8 == 5
    else:
        chunks, ln_cases, ln_slots = lay.chunks[:14], [(136, 17)], lay.ln
        assert tr.front_units((136,), len(chunks)) == (2, 16)
    parts = _ln_partials(dev, ln_cases, 520)
    aux, keep = _aux(L, flat, state, gs, ln=[(xd, n, s) for (_, xd), (_, n), s in zip(parts, ln_cases, ln_slots)], chunks=chunks, with_lp=with_lp)
    _launch(L, lib, [dummy], aux)
    torch.cuda.synchronize()
    stored = torch.zeros(flat.n, dtype=torch.bool)
    updated = []
    if ln_cases:
        worst = _check_ln_gradients(L, lib, dev, flat, ln_slots, ln_cases, parts)
        print(f"finalize: worst |stored - float64| / finalize_bound = {worst:.3f}")
        stored |= lay.masks["ln"]
        updated = lay.ranges("ln")
    _check_flat(L, lib, flat, state, gs, updated, chunks, stored, with_lp, f"chunks ({front})")
    dummy.check_plain()


# ------------------------------------------------------------------------------------------ bias Adam
# (8, 8, 8) the smallest problem; (200, 136, 40) 2 x 2 tiles, ragged rows and columns: the bias is summed by the column-0 tiles only
# and must be updated once; (384, 128, 64) three row tiles; (128, 264, 16) three column tiles
BIAS_SHAPES = [(8, 8, 8), (200, 136, 40), (384, 128, 64), (128, 264, 16)]


@pytest.mark.parametrize("bias_adam", [1, 0], ids=["bias_adam", "rowsums_only"])
@pytest.mark.parametrize("fused", [True, False], ids=["fused_weights", "plain"])
def test_bias_adam(dev, hip, fused, bias_adam):
    """No front units at all (n_ln = n_chunks = 0).  Five problems: three with rowsum_out inside [g, g + n_flat) (their biases get
    Adam when bias_adam is set, and only then), one with rowsum_out in a buffer of its own (row sums, no Adam), one without row
    sums; the weights with the optimiser epilogue or plain, outputs outside the flat buffers either way."""
    L, lib = hip
    inside = [0, 1, 2] if fused else [1, 2, 3]                      # which shapes have their bias in the flat buffers
    apart = 3 if fused else 0
    lay = tr.build_layout(7, bias_sizes=[BIAS_SHAPES[i][0] for i in inside])
    flat = _Flat(dev, lay.n_flat, 47)
    state, gs = _state(dev, 3), _gs(dev, 0.25)
    fuse = (state, gs) if fused else None
    own = torch.full((BIAS_SHAPES[apart][0] + 8,), NAN, device=dev)
    probs, slot_of = [], {}
    for i, (M, N, K) in enumerate(BIAS_SHAPES):
        if i in inside:
            slot_of[i] = lay.bias[inside.index(i)]
            assert slot_of[i].n == M
            rowsum = flat.g_ptr(slot_of[i].off)
        else:
            rowsum = own.data_ptr()
        probs.append(_Problem(L, dev, M, N, K, 80 + i, rowsum=rowsum, fuse=fuse, lpT="aligned" if i == 2 else None))
    probs.append(_Problem(L, dev, 8, 8, 8, 90, rowsum=0, fuse=fuse))
    aux, keep = _aux(L, flat, state, gs, bias_adam=bias_adam)
    _launch(L, lib, probs, aux)
    torch.cuda.synchronize()
    # 1: the row sums
    g = flat.g.cpu()
    worst = 0.0
    for i, s in slot_of.items():
        worst = max(worst, relmax(g[s.off:s.off + s.n], probs[i].rsum))
    worst = max(worst, relmax(own[:BIAS_SHAPES[apart][0]], probs[apart].rsum))
    print(f"row sums: worst relmax {worst:.3e} (bar {GEMM_REL:.0e})")
    assert worst < GEMM_REL
    assert bool(torch.isnan(own[BIAS_SHAPES[apart][0]:]).all())
    # 2 - 4
    _check_flat(L, lib, flat, state, gs, lay.ranges("bias") if bias_adam else [], [], lay.masks["bias"], True,
                f"bias Adam ({'fused' if fused else 'plain'} weights)" if bias_adam else "bias_adam = 0")
    st = [float(x) for x in state.cpu().double()[:4]]
    if fused:
        _report("fused weights", [q.check_weight(st, 0.25, f"weight {q.M}x{q.N}") for q in probs])
    else:
        for q in probs:
            q.check_plain()


# ------------------------------------------------------------------------------------------ everything in one launch, stepped
STEP_LN = [(136, 65), (8, 1), (512, 129)]
STEP_CHUNKS = CHUNK_LENS[:6]
STEP_PROBLEMS = [(200, 136, 40, True, "bias"), (8, 8, 8, False, "bias"), (128, 264, 16, True, None)]      # M, N, K, fused, rowsum


def _stepped(L, lib, dev, mode):
    """Three optimiser steps of one launch holding LayerNorm units, chunks, bias Adam and fused weights, mtn_noam_tick between
    them, new gradients / partial rows / operands written into the SAME device buffers before each.  mode 'eager': three calls;
    'graph': the call captured once, replayed three times.  Checks every step against the free-running float64 recurrence and
    returns the bits of everything after each step."""
    lay = tr.build_layout(9, ln_widths=[d for d, _ in STEP_LN], bias_sizes=[M for M, _, _, _, r in STEP_PROBLEMS if r], chunk_lens=STEP_CHUNKS)
    flat = _Flat(dev, lay.n_flat, 61)
    state, gs = torch.zeros(8, device=dev), _gs(dev, 0.25)
    probs, k = [], 0
    for i, (M, N, K, fused, r) in enumerate(STEP_PROBLEMS):
        rowsum = 0
        if r:
            rowsum, k = flat.g_ptr(lay.bias[k].off), k + 1
        probs.append(_Problem(L, dev, M, N, K, 100 + i, rowsum=rowsum, fuse=(state, gs) if fused else None, lpT="aligned" if i == 2 else None))
    part_d = [torch.full((n + 1, 2 * d), 1e30, device=dev) for d, n in STEP_LN]
    aux, keep = _aux(L, flat, state, gs, ln=[(xd, n, s) for xd, (_, n), s in zip(part_d, STEP_LN, lay.ln)], chunks=lay.chunks, bias_adam=1)
    graph = None
    if mode == "graph":
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):                                # the table is built and copied NOW: only pointers are frozen
            _launch(L, lib, probs, aux)
    updated = lay.ranges("ln") + lay.ranges("bias") + lay.ranges("chunk")
    stored = lay.masks["ln"] | lay.masks["bias"]
    listed = ~lay.untouched
    p64, m64, v64 = flat.p0.double(), flat.m0.double(), flat.v0.double()
    snaps = []
    for step in (1, 2, 3):
        _tick(L, lib, state, *NOAM)
        g_in = rr.adam_inputs(flat.n, 61 + step)[1]
        flat.g.copy_(g_in)
        xs = [tr.partials(n, 2 * d, 700 + 10 * step + i) for i, (d, n) in enumerate(STEP_LN)]
        for xd, x, (_, n) in zip(part_d, xs, STEP_LN):
            xd[:n].copy_(x)
        for i, q in enumerate(probs):
            q.operands(100 + 10 * step + i)
        if graph is None:
            _launch(L, lib, probs, aux)
        else:
            graph.replay()
        torch.cuda.synchronize()
        p, g, m, v, lp = (t.cpu() for t in (flat.p, flat.g, flat.m, flat.v, flat.lp))
        st = [float(x) for x in state.cpu().double()[:4]]
        assert st[0] == float(step)
        # 1: stored gradients
        for s, x in zip(lay.ln, xs):
            assert _same_bits(torch.cat([g[s.a_off:s.a_off + s.d], g[s.b_off:s.b_off + s.d]]), tr.finalize_f32(x))
        k = 0
        for q, (_, _, _, _, r) in zip(probs, STEP_PROBLEMS):
            if r:
                s, k = lay.bias[k], k + 1
                assert relmax(g[s.off:s.off + s.n], q.rsum) < GEMM_REL
        assert torch.equal(_bits(g)[~stored], _bits(g_in)[~stored])
        # 2: the free-running float64 recurrence, fed the stored gradient
        errs = []
        for off, n in updated:
            sl = slice(off, off + n)
            p64[sl], m64[sl], v64[sl] = rr.adam_step64(p64[sl], g[sl].double(), m64[sl], v64[sl], st[1], st[2], st[3], 0.25)
            errs.append(_adam_errs(p[sl], m[sl], v[sl], p64[sl], m64[sl], v64[sl], f"{mode} step {step} [{off}, {off + n})"))
            assert _same_bits(lp[sl], p[sl].to(BF16))
        _report(f"{mode} step {step}, flat ranges", errs)
        _report(f"{mode} step {step}, fused weights", [q.check_weight(st, 0.25, f"{mode} step {step} weight {q.M}x{q.N}") for q in probs if q.f])
        for q in probs:
            if not q.f:
                q.check_plain()
        # 4
        for got, was in ((p, flat.p0), (m, flat.m0), (v, flat.v0)):
            assert torch.equal(_bits(got)[~listed], _bits(was)[~listed])
        assert bool((lp[~listed] == LP_SENTINEL).all())
        snap = [p, g, m, v, lp]
        for q in probs:
            snap += [q.out.cpu()] + ([q.w.cpu(), q.m.cpu(), q.v.cpu(), q.lp.cpu()] if q.f else []) + ([q.lpT.cpu()] if q.f and q.lpT is not None else [])
        snaps.append(snap)
    return snaps


def test_everything_in_one_launch_stepped_and_captured(dev, hip):
    L, lib = hip
    eager = _stepped(L, lib, dev, "eager")
    replayed = _stepped(L, lib, dev, "graph")
    for step, (a, b) in enumerate(zip(eager, replayed), 1):
        assert len(a) == len(b)
        for k, (x, y) in enumerate(zip(a, b)):
            assert _same_bits(x, y), (step, k)
    assert not _same_bits(eager[0][0], eager[2][0])


# ------------------------------------------------------------------------------------------ generic epilogue fallback
FALLBACK_SHAPES = [(200, 136, 333), (8, 8, 8), (384, 128, 64), (128, 128, 96)]            # from test_gemm_tt_table_form's list


@pytest.mark.parametrize("misaligned", ["ldT", "base"])
def test_generic_epilogue_fallback(dev, hip, misaligned):
    """ONE transposed copy with ldT = M + 4 (not a multiple of 8), or with its base 2 elements past a 16-byte boundary, sends the
    whole launch through the generic epilogue (lds_epilogue = 0): test_gemm_tt_table_form's float64 checks and bars on every
    problem, two launches."""
    L, lib = hip
    state = _state(dev, 3)
    probs = []
    for i, (M, N, K) in enumerate(FALLBACK_SHAPES):
        kind = misaligned if i == 2 else ("aligned" if i % 2 == 0 else None)
        probs.append(_Problem(L, dev, M, N, K, 120 + i, rowsum=0, fuse=(state, None), lpT=kind, write_grad=int(i % 3 == 0)))
    q = probs[2]
    assert q.f.ldT % 8 != 0 or (q.f.p_lpT & 15) != 0
    st = [float(x) for x in state.cpu().double()[:4]]
    for launch in range(2):
        _launch(L, lib, probs, None)
        torch.cuda.synchronize()
        _report(f"generic epilogue ({misaligned}), launch {launch}", [q.check_weight(st, 1.0, f"weight {q.M}x{q.N}") for q in probs])


# ------------------------------------------------------------------------------------------ argument checks
def test_argument_checks(dev, hip):
    """Every bad mtn_tt_aux is refused on the host before anything is staged or launched: no buffer changes.  Then the unmodified
    arguments run."""
    L, lib = hip
    lay = tr.build_layout(8, ln_widths=(8,), chunk_lens=(8, 252))
    flat = _Flat(dev, lay.n_flat, 53)
    state, gs = _state(dev, 2), None
    prob = _Problem(L, dev, 8, 8, 8, 130, fuse=(state, gs))
    x, xd = _ln_partials(dev, [(8, 3)], 540)[0]

    def build():
        return _aux(L, flat, state, gs, ln=[(xd, 3, lay.ln[0])], chunks=lay.chunks)

    def untouched():
        torch.cuda.synchronize()
        return (all(_same_bits(a.cpu(), b) for a, b in ((flat.p, flat.p0), (flat.g, flat.g0), (flat.m, flat.m0), (flat.v, flat.v0)))
                and bool((flat.lp == LP_SENTINEL).all()) and prob.weight_untouched() and bool(torch.isnan(prob.out).all()))

    def chunk_len(i, n):
        def f(aux, keep):
            keep[2][i] = n
        return f

    def chunk_off(i, o):
        def f(aux, keep):
            keep[1][i] = o
        return f

    def unit(**kw):
        def f(aux, keep):
            for k, v in kw.items():
                setattr(keep[0][0], k, v)
        return f

    def field(**kw):
        def f(aux, keep):
            for k, v in kw.items():
                setattr(aux, k, v)
        return f

    last = lay.chunks[-1]
    bad = [chunk_len(0, 4100), chunk_len(0, 6), chunk_off(0, lay.chunks[0].off + 2),
           chunk_off(1, flat.n - last.len + 4),                                  # ends past n_flat
           unit(a_off=flat.n - 4),                                                 # a_off + d > n_flat
           unit(nparts=0), field(p=0), field(n_flat=0),
           field(ln=C.POINTER(L.TtLnUnit)()),                                      # n_ln > 0, ln = NULL
           field(state=0),                                                         # front units without the optimiser state
           field(beta2=0.99)]                                                      # != the problem's mtn_adam_fuse.beta2
    assert untouched()
    for mutate in bad:
        aux, keep = build()
        mutate(aux, keep)
        with pytest.raises(L.MtnHipError):
            _launch(L, lib, [prob], aux)
    assert untouched()
    aux, keep = build()
    _launch(L, lib, [prob], aux)
    torch.cuda.synchronize()
    assert not untouched()
    _check_ln_gradients(L, lib, dev, flat, lay.ln, [(8, 3)], [(x, xd)])
    _check_flat(L, lib, flat, state, gs, lay.ranges("ln"), lay.chunks, lay.masks["ln"], True, "unmodified arguments")
    prob.check_weight([float(v) for v in state.cpu().double()[:4]], 1.0, "weight 8x8")
