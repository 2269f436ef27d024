"""Direct tests, through the C ABI, of the LayerNorm row kernels of csrc/layernorm.hip (mtn_layernorm_fwd_group, _bwd_group,
_bwd_finalize and the single-stream wrappers) against the float64 references and DERIVED elementwise bounds of tests/ln_row_refs.py
(argued there, validated without a GPU by tests/test_ln_row_refs.py; none was obtained by running a kernel).  Every output lies in a
NaN-filled allocation with guard rows before and after it; inputs that must not be read (lut rows no token names, pe rows from
seq_len on) hold NaN.  Every element is compared; the worst |kernel - reference| / bound of each output is printed."""

import numpy as np
import pytest
import torch

from tests import ln_row_refs as lr

pytestmark = pytest.mark.gpu

NAN = float("nan")
G = 2                                   # guard rows on each side of an output
F32, BF16 = torch.float32, torch.bfloat16


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def hip():
    from mtn_amd import lib as L
    return L, L.load()


@pytest.fixture(scope="module")
def seed(dev):
    return torch.tensor([lr.SEED], dtype=torch.int64, device=dev)


class _Out:
    """A [rows, cols] output in the middle of a NaN-filled [G + rows + G, cols] allocation."""

    def __init__(self, dev, rows, cols, dtype=F32):
        self.full = torch.full((rows + 2 * G, cols), NAN, device=dev, dtype=dtype)
        self.rows = rows

    def ptr(self):
        return self.full[G:].data_ptr()

    def get(self):
        """-> the output on the host; the guard rows must still be NaN"""
        f = self.full.cpu()
        assert bool(torch.isnan(f[:G]).all()) and bool(torch.isnan(f[G + self.rows:]).all()), "guard rows written"
        return f[G:G + self.rows]

    def untouched(self):
        return bool(torch.isnan(self.full).all())


def _t(dev, a, dtype=F32):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).to(dtype).to(dev)


def _p(t):
    return 0 if t is None else t.data_ptr()


def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])


def _chunks(items, sizes=(1, 3, 8)):
    """consecutive groups of 1, 3, 8, 1, 3, 8 ... items"""
    out, i, k = [], 0, 0
    while i < len(items):
        out.append(items[i:i + sizes[k % len(sizes)]])
        i += sizes[k % len(sizes)]
        k += 1
    return out


WORST = {}


def _check(name, out, ref, bound, what):
    w = lr.assert_within(out, ref, bound, f"{name} {what}")
    WORST[name] = max(WORST.get(name, 0.0), w)
    return w


def _report():
    print("worst |kernel - float64| / bound so far:  " + " | ".join(f"{k} {v:.5f}" for k, v in sorted(WORST.items())))


# ------------------------------------------------------------------------------------------ forward
class _FwdStream:
    """Device buffers and descriptor of one forward stream.  c: a make_case / make_src problem (source fields optional)."""

    OUTS = ("y_f32", "y_lp", "mean", "rstd", "x_out")

    def __init__(self, L, dev, seed, c, lp_dtype, absent=()):
        self.c, self.lp_dtype = c, lp_dtype
        rows, d = c.rows, c.d
        tokens, pe = getattr(c, "tokens", None), getattr(c, "pe", None)
        self.keep_alive = k = dict(x=_t(dev, c.x), a2=_t(dev, c.a2), b2=_t(dev, c.b2), lut=_t(dev, getattr(c, "lut", None)), pe=_t(dev, pe),
                                   tokens=None if tokens is None else torch.as_tensor(tokens, dtype=torch.int64).to(dev))
        self.out = dict(y_f32=_Out(dev, rows, d), y_lp=_Out(dev, rows, d, lp_dtype), mean=_Out(dev, rows, 1), rstd=_Out(dev, rows, 1),
                        x_out=_Out(dev, rows, d))
        D = L.LnFwdDesc()
        D.rows, D.d, D.eps, D.x, D.a2, D.b2 = rows, d, c.eps, _p(k["x"]), _p(k["a2"]), _p(k["b2"])
        D.tokens, D.lut, D.emb_scale, D.pe = _p(k["tokens"]), _p(k["lut"]), float(getattr(c, "emb_scale", 1.0)), _p(k["pe"])
        D.seq_len, D.no_ln = int(getattr(c, "seq_len", 0)), int(getattr(c, "no_ln", False))
        if pe is not None and c.p > 0:
            D.drop = L.Dropout(float(c.p), c.salt, seed.data_ptr())
        for name in self.OUTS:
            setattr(D, name, 0 if name in absent else self.out[name].ptr())
        self.D, self.absent = D, set(absent)

    def check(self, what):
        c = self.c
        rows, d = c.rows, c.d
        if getattr(c, "pe", None) is not None:
            x64, bx = lr.src64(rows, d, **lr.src_args(c))
        else:
            x64, bx = np.asarray(c.x, dtype=np.float64), np.zeros((rows, d))
        got = {n: (None if n in self.absent else self.out[n].get()) for n in self.OUTS}
        for n in self.absent:
            assert self.out[n].untouched()
        if got["x_out"] is not None:
            _check("x_out", got["x_out"], x64, bx, what)
            if getattr(c, "keep", None) is not None:
                assert bool((_bits(got["x_out"])[torch.from_numpy(~c.keep)] == 0).all()), "dropped elements of x_out are +0.0"
        if getattr(c, "no_ln", False):
            assert self.out["mean"].untouched() and self.out["rstd"].untouched()
            if got["y_f32"] is not None:
                _check("y_f32", got["y_f32"], x64, bx, what)
            if got["y_lp"] is not None:
                _check("y_lp", got["y_lp"], x64, bx + (lr.BF * (np.abs(x64) + bx) if self.lp_dtype == BF16 else 0.0), what)
            return
        y, mean, rstd = lr.fwd64(x64, c.a2, c.b2, c.eps)
        B = lr.fwd_bounds(x64, bx, c.a2, c.b2, c.eps)
        if got["mean"] is not None:
            _check("mean", got["mean"][:, 0], mean, B["mean"], what)
        if got["rstd"] is not None:
            _check("rstd", got["rstd"][:, 0], rstd, B["rstd"], what)
        if got["y_f32"] is not None:
            _check("y_f32", got["y_f32"], y, B["y_f32"], what)
        if got["y_lp"] is not None:
            _check("y_lp", got["y_lp"], y, B["y_bf16" if self.lp_dtype == BF16 else "y_f32"], what)
        k = getattr(c, "const_row", None)
        if k is not None and not self.absent:              # class e: the constant row is exact and finite
            assert float(got["mean"][k, 0]) == 0.5 and got["rstd"][k, 0].numpy() == np.float32(1.0) / np.float32(c.eps)
            assert torch.equal(_bits(got["y_f32"][k]), _bits(torch.from_numpy(c.b2)))
            assert torch.equal(_bits(got["y_lp"][k]), _bits(torch.from_numpy(c.b2).to(self.lp_dtype)))


def _run_fwd(L, lib, dev, seed, cases, lp_dtype, absent=(), what=""):
    streams = [_FwdStream(L, dev, seed, c, lp_dtype, absent) for c in cases]
    arr = (L.LnFwdDesc * len(streams))(*[s.D for s in streams])
    L.check(lib.mtn_layernorm_fwd_group(L.dtype_code(lp_dtype), len(streams), arr, L.stream_ptr()))
    torch.cuda.synchronize()
    for i, s in enumerate(streams):
        s.check(f"{what} stream {i} {(s.c.rows, s.c.d, getattr(s.c, 'cls', getattr(s.c, 'mode', '')))}")
    return streams


def _by_class(cases):
    """class-major order: neighbours in a group differ in rows and d"""
    return sorted(cases, key=lambda t: (t[2], lr.PAIRS.index((t[0], t[1]))))


FWD_GROUPS = _chunks(_by_class([t for t in lr.fwd_cases() if t[1] <= 512])) + _chunks(_by_class([t for t in lr.fwd_cases() if t[1] > 512]))


@pytest.mark.parametrize("lp_dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("gi", range(len(FWD_GROUPS)), ids=[f"{len(g)}x{'small' if g[0][1] <= 512 else 'generic'}{i}" for i, g in enumerate(FWD_GROUPS)])
def test_forward_groups(dev, hip, seed, gi, lp_dtype):
    """Every (rows, d, class) of ln_row_refs.fwd_cases() in launches of 1, 3 and 8 streams (widths up to 512 together: the register
    kernel; wider ones together: the three-pass kernel), all five outputs present, both compute dtypes."""
    L, lib = hip
    _run_fwd(L, lib, dev, seed, [lr.make_case(*t) for t in FWD_GROUPS[gi]], lp_dtype, what=f"group {gi}")
    _report()


@pytest.mark.parametrize("absent", _FwdStream.OUTS)
def test_forward_each_output_absent_once(dev, hip, seed, absent):
    L, lib = hip
    for shapes in ([(5, 256, "a"), (3, 8, "b"), (17, 260, "c")], [(4, 516, "a"), (9, 2048, "d"), (1, 1028, "b")]):
        _run_fwd(L, lib, dev, seed, [lr.make_case(*t) for t in shapes], BF16, absent=(absent,), what=f"without {absent}")


def test_forward_single_stream_wrapper(dev, hip):
    L, lib = hip
    c = lr.make_case(9, 260, "a")
    x, a2, b2 = _t(dev, c.x), _t(dev, c.a2), _t(dev, c.b2)
    y, ylp, mean, rstd = _Out(dev, 9, 260), _Out(dev, 9, 260, BF16), _Out(dev, 9, 1), _Out(dev, 9, 1)
    L.check(lib.mtn_layernorm_fwd(L.MTN_BF16, 9, 260, c.eps, x.data_ptr(), a2.data_ptr(), b2.data_ptr(), y.ptr(), ylp.ptr(), mean.ptr(),
                                  rstd.ptr(), L.stream_ptr()))
    torch.cuda.synchronize()
    yr, mr, rr = lr.fwd64(c.x, c.a2, c.b2, c.eps)
    B = lr.fwd_bounds(c.x, np.zeros((9, 260)), c.a2, c.b2, c.eps)
    _check("y_f32", y.get(), yr, B["y_f32"], "wrapper")
    _check("y_lp", ylp.get(), yr, B["y_bf16"], "wrapper")
    _check("mean", mean.get()[:, 0], mr, B["mean"], "wrapper")
    _check("rstd", rstd.get()[:, 0], rr, B["rstd"], "wrapper")


MIXED = [(17, 260, "a"), (9, 256, "b"), (3, 512, "c"), (5, 4, "d")]


@pytest.mark.parametrize("lp_dtype", [F32, BF16], ids=["f32", "bf16"])
def test_forward_mixed_d_group(dev, hip, seed, lp_dtype):
    """A group takes its kernel from its LARGEST d: each stream of width <= 512 alone (register kernel) and beside a d = 516 stream
    (three-pass kernel) — the only way the same stream runs through both.  Each run inside the bounds."""
    L, lib = hip
    wide = lr.make_case(4, 516, "a")
    for t in MIXED:
        _run_fwd(L, lib, dev, seed, [lr.make_case(*t)], lp_dtype, what="alone")
        _run_fwd(L, lib, dev, seed, [lr.make_case(*t), wide], lp_dtype, what="beside d = 516")
    _run_fwd(L, lib, dev, seed, [wide] + [lr.make_case(*t) for t in MIXED], lp_dtype, what="all behind d = 516")
    _report()


@pytest.mark.parametrize("lp_dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("p", lr.SRC_P)
@pytest.mark.parametrize("d", lr.SRC_D)
def test_forward_source_modes(dev, hip, seed, d, p, lp_dtype):
    """The synthesised source row: tokens + pe + dropout, x + pe + dropout, and the same with no_ln = 1 (row -> x_out and y), three
    streams in one launch; d = 64 and 512 on the register kernel, 640 on the three-pass kernel.  Dropped elements of x_out are exactly
    0; mean and rstd are those of the dropped row; unnamed lut rows and pe rows from seq_len on hold NaN."""
    L, lib = hip
    _run_fwd(L, lib, dev, seed, [lr.make_src(m, d, p) for m in lr.SRC_MODES], lp_dtype, what=f"source d {d} p {p}")
    _report()


# ------------------------------------------------------------------------------------------ backward
class _BwdStream:
    def __init__(self, L, dev, seed, c, has_dres, lp_dtype, lp_p, salt, partial=True, alias=False, dx_lp=True):
        self.c, self.has_dres, self.lp_dtype, self.lp_p, self.salt = c, has_dres, lp_dtype, lp_p, salt
        rows, d = c.rows, c.d
        _, mean, rstd = lr.fwd64(c.x, c.a2, c.b2, c.eps)
        self.m32, self.r32 = mean.astype(np.float32), rstd.astype(np.float32)
        self.k = k = dict(x=_t(dev, c.x), a2=_t(dev, c.a2), g=_t(dev, c.g), mean=_t(dev, self.m32), rstd=_t(dev, self.r32),
                          dres=_t(dev, c.dres) if has_dres and not alias else None)
        self.nb = lr.nblocks(rows)
        self.dx, self.dx_lp = _Out(dev, rows, d), (_Out(dev, rows, d, lp_dtype) if dx_lp else None)
        self.partial = _Out(dev, self.nb, 2 * d) if partial else None
        if alias:                                            # dx aliases dres: the output buffer arrives holding dres
            self.dx.full[G:G + rows] = _t(dev, c.dres)
        D = L.LnBwdDesc()
        D.rows, D.d, D.eps, D.x, D.a2, D.mean, D.rstd, D.g = rows, d, c.eps, _p(k["x"]), _p(k["a2"]), _p(k["mean"]), _p(k["rstd"]), _p(k["g"])
        D.dres = self.dx.ptr() if alias else _p(k["dres"])
        D.dx, D.partial = self.dx.ptr(), (self.partial.ptr() if partial else 0)
        if dx_lp:
            D.dx_lp, D.dx_lp_dtype = self.dx_lp.ptr(), L.dtype_code(lp_dtype)
            if lp_p > 0:
                D.dx_lp_drop = L.Dropout(float(lp_p), salt, seed.data_ptr())
        self.D = D

    def refs(self):
        c = self.c
        ref = lr.bwd64(c.x, c.a2, c.g, c.eps, c.dres if self.has_dres else None)
        return ref, lr.bwd_bounds(c.x, c.a2, c.g, c.eps, self.m32, self.r32, self.has_dres, ref[0])

    def check(self, what):
        c = self.c
        (dx, da2, db2, part), B = self.refs()
        _check("dx", self.dx.get(), dx, B["dx"], what)
        if self.dx_lp is not None:
            keep = lr.keep2d(self.salt, self.lp_p, c.rows, c.d) if self.lp_p > 0 else None
            lp_ref, v = lr.handoff64(dx, keep, self.lp_p, self.lp_dtype)
            got = self.dx_lp.get()
            _check("dx_lp", got, lp_ref, lr.handoff_bound(v, B["dx"], keep, self.lp_p, self.lp_dtype), what)
            if keep is not None:
                assert bool((_bits(got)[torch.from_numpy(~keep)] == 0).all())
        if self.partial is not None:
            _check("partial", self.partial.get(), part, B["partial"], what)
        return (da2, db2), B


def _run_bwd(L, lib, dev, streams, what=""):
    arr = (L.LnBwdDesc * len(streams))(*[s.D for s in streams])
    L.check(lib.mtn_layernorm_bwd_group(len(streams), arr, L.stream_ptr()))
    fin = [s for s in streams if s.partial is not None]
    outs = [(_Out(dev, 1, s.c.d), _Out(dev, 1, s.c.d)) for s in fin]
    if fin:
        fa = (L.LnFinalizeDesc * len(fin))(*[L.LnFinalizeDesc(s.partial.ptr(), lib.mtn_layernorm_bwd_nparts(s.c.rows), s.c.d, a.ptr(), b.ptr())
                                             for s, (a, b) in zip(fin, outs)])
        L.check(lib.mtn_layernorm_bwd_finalize(len(fin), fa, L.stream_ptr()))
    torch.cuda.synchronize()
    for i, s in enumerate(streams):
        w = f"{what} stream {i} {(s.c.rows, s.c.d, s.c.cls)}"
        (da2, db2), B = s.check(w)
        if s.partial is not None:
            a, b = outs[fin.index(s)]
            _check("da2", a.get()[0], da2, B["da2"], w)
            _check("db2", b.get()[0], db2, B["db2"], w)
            # finalize holds only additions: the host emulation, fed the kernel's own partial rows, gives the same bits
            em = lr.emulate_finalize(s.partial.get().numpy())
            assert np.array_equal(em[:s.c.d].view(np.int32), a.get()[0].numpy().view(np.int32))
            assert np.array_equal(em[s.c.d:].view(np.int32), b.get()[0].numpy().view(np.int32))


_BWD = list(enumerate(lr.bwd_cases()))
_bkey = lambda it: (it[1][2], lr.PAIRS.index((it[1][0], it[1][1])))
BWD_GROUPS = _chunks(sorted([it for it in _BWD if it[1][1] <= 512], key=_bkey)) + _chunks(sorted([it for it in _BWD if it[1][1] > 512], key=_bkey))


@pytest.mark.parametrize("gi", range(len(BWD_GROUPS)), ids=[f"{len(g)}x{'small' if g[0][1][1] <= 512 else 'generic'}{i}" for i, g in enumerate(BWD_GROUPS)])
def test_backward_groups(dev, hip, seed, gi):
    """Every (rows, d, class) of ln_row_refs.bwd_cases() in launches of 1, 3 and 8 streams; per case with or without dres, the hand-off
    copy in float32 or bfloat16, without dropout or with p = 0.1 / 0.5 (ln_row_refs.bwd_variant); partial rows, then one grouped
    finalize per launch: da2, db2."""
    L, lib = hip
    streams = [_BwdStream(L, dev, seed, lr.make_case(*t), *lr.bwd_variant(i), salt=0x700 + i) for i, t in BWD_GROUPS[gi]]
    _run_bwd(L, lib, dev, streams, what=f"group {gi}")
    _report()


def test_backward_part_counts(hip):
    L, lib = hip
    for rows in (1, 7, 8, 9, 16, 17, 640, 4097):
        assert lib.mtn_layernorm_bwd_nparts(rows) == -(-rows // 8)
        for d in (4, 260, 2048):
            assert lib.mtn_layernorm_bwd_partial_floats(rows, d) == -(-rows // 8) * 2 * d


@pytest.mark.parametrize("shape", [(17, 260, "a"), (9, 1028, "c")], ids=["small", "generic"])
def test_backward_dx_aliases_dres(dev, hip, seed, shape):
    """dx may alias dres (include/mtn_hip.h): the output buffer arrives holding the residual gradient."""
    L, lib = hip
    _run_bwd(L, lib, dev, [_BwdStream(L, dev, seed, lr.make_case(*shape), True, BF16, 0.1, 0x7F0, alias=True)], what="dx aliases dres")


def test_backward_mixed_d_group(dev, hip, seed):
    """Each stream of width <= 512 alone (ln_bwd_small_kernel) and beside a d = 516 stream (ln_bwd_kernel); in the grouped run one
    member has partial = NULL (dx only) beside members with a partial buffer."""
    L, lib = hip
    mk = lambda t, i, **kw: _BwdStream(L, dev, seed, lr.make_case(*t), i % 2 == 0, (F32, BF16)[i % 2], (0.5, 0.0, 0.1)[i % 3], 0x7E0 + i, **kw)
    for i, t in enumerate(MIXED):
        _run_bwd(L, lib, dev, [mk(t, i)], what="alone")
        _run_bwd(L, lib, dev, [mk(t, i), mk((4, 516, "a"), i + 1, partial=(i % 2 == 0))], what="beside d = 516")
    _run_bwd(L, lib, dev, [mk((4, 516, "a"), 0)] + [mk(t, i, partial=(i != 1), dx_lp=(i != 2)) for i, t in enumerate(MIXED)], what="all behind d = 516")
    _run_bwd(L, lib, dev, [mk(t, i, partial=(i != 2)) for i, t in enumerate(MIXED)], what="small kernel, one partial NULL")
    _run_bwd(L, lib, dev, [mk(t, i, partial=False) for i, t in enumerate(MIXED[:2])], what="no partial at all")
    _report()


def test_backward_single_stream_wrapper(dev, hip):
    L, lib = hip
    c = lr.make_case(17, 260, "a")
    S = _BwdStream(L, dev, None, c, True, F32, 0.0, 0, dx_lp=False)
    da2, db2 = _Out(dev, 1, c.d), _Out(dev, 1, c.d)
    k = S.k
    L.check(lib.mtn_layernorm_bwd(c.rows, c.d, c.eps, _p(k["x"]), _p(k["a2"]), _p(k["mean"]), _p(k["rstd"]), _p(k["g"]), _p(k["dres"]), S.dx.ptr(),
                                  da2.ptr(), db2.ptr(), S.partial.ptr(), L.stream_ptr()))
    torch.cuda.synchronize()
    (ra, rb), B = S.check("wrapper")
    _check("da2", da2.get()[0], ra, B["da2"], "wrapper")
    _check("db2", db2.get()[0], rb, B["db2"], "wrapper")


# ------------------------------------------------------------------------------------------ finalize
def _finalize(L, lib, dev, specs):
    """specs: (nparts, d, with da2, with db2) -> per spec (partial, da2 row or None, db2 row or None), one call"""
    parts = [lr.make_partials(n, d, 31 * n + d + 5 * i) for i, (n, d, _, _) in enumerate(specs)]
    dparts = [_t(dev, p) for p in parts]
    outs = [(_Out(dev, 1, d) if wa else None, _Out(dev, 1, d) if wb else None) for (_, d, wa, wb) in specs]
    arr = (L.LnFinalizeDesc * len(specs))(*[L.LnFinalizeDesc(dp.data_ptr(), n, d, a.ptr() if a else 0, b.ptr() if b else 0)
                                            for dp, (n, d, _, _), (a, b) in zip(dparts, specs, outs)])
    L.check(lib.mtn_layernorm_bwd_finalize(len(specs), arr, L.stream_ptr()))
    torch.cuda.synchronize()
    return [(p, a.get()[0].numpy() if a else None, b.get()[0].numpy() if b else None) for p, (a, b) in zip(parts, outs)]


def _check_finalize(res, specs, again=None):
    for i, ((p, a, b), (n, d, _, _)) in enumerate(zip(res, specs)):
        ref, bound, em = lr.finalize64(p), lr.finalize_bound(p), lr.emulate_finalize(p)
        for half, got in ((slice(0, d), a), (slice(d, 2 * d), b)):
            if got is None:
                continue
            _check("finalize", got, ref[half], bound[half], f"nparts {n} d {d}")
            assert np.array_equal(got.view(np.int32), em[half].view(np.int32)), f"nparts {n} d {d}: not the bits of the emulation"
            if again is not None:
                other = again[i][1] if half.start == 0 else again[i][2]
                assert np.array_equal(got.view(np.int32), other.view(np.int32)), f"nparts {n} d {d}: bits differ between two runs"


def test_finalize_loop_boundaries(dev, hip):
    """Synthetic partial buffers straight into mtn_layernorm_bwd_finalize: every part count around the kernel's loop boundaries, three
    widths, all 39 members in ONE call (members of different d and nparts side by side), every third with a null da2 or db2.  Bound
    against float64, bit equality with the emulation, the same bits on a second run."""
    L, lib = hip
    specs = [(n, d, (i + j) % 3 != 1, (i + j) % 3 != 2) for i, n in enumerate(lr.FIN_NPARTS) for j, d in enumerate(lr.FIN_D)]
    first = _finalize(L, lib, dev, specs)
    _check_finalize(_finalize(L, lib, dev, specs), specs, again=first)
    _report()


def test_finalize_113_descriptors_split(dev, hip):
    """113 descriptors: MTN_LN_FINALIZE_MAX_GROUP = 112 in the first launch, one in the second."""
    L, lib = hip
    specs = [(lr.FIN_NPARTS[i % len(lr.FIN_NPARTS)], lr.FIN_D[i % 3], True, True) for i in range(113)]
    specs[112] = (129, 36, True, True)
    _check_finalize(_finalize(L, lib, dev, specs), specs)


# ------------------------------------------------------------------------------------------ argument checks
def test_argument_checks(dev, hip, seed):
    """Bad arguments raise MtnHipError and launch nothing: every output keeps its NaN."""
    L, lib = hip
    c = lr.make_case(5, 8, "a")

    def fwd(mutate, count=1):
        S = [_FwdStream(L, dev, seed, c, BF16) for _ in range(max(count, 1))]
        mutate(S[0].D)
        arr = (L.LnFwdDesc * len(S))(*[s.D for s in S])
        with pytest.raises(L.MtnHipError):
            L.check(lib.mtn_layernorm_fwd_group(L.MTN_BF16, count, arr, L.stream_ptr()))
        torch.cuda.synchronize()
        assert all(o.untouched() for s in S for o in s.out.values())

    def bwd(mutate, count=1):
        S = [_BwdStream(L, dev, seed, c, True, BF16, 0.1, 1) for _ in range(max(count, 1))]
        mutate(S[0].D)
        arr = (L.LnBwdDesc * len(S))(*[s.D for s in S])
        with pytest.raises(L.MtnHipError):
            L.check(lib.mtn_layernorm_bwd_group(count, arr, L.stream_ptr()))
        torch.cuda.synchronize()
        assert all(s.dx.untouched() and s.dx_lp.untouched() and s.partial.untouched() for s in S)

    def set_(**kw):
        def f(D):
            for k, v in kw.items():
                setattr(D, k, v)
        return f

    pe = torch.zeros(5, 8, device=dev)
    for m in (set_(d=6), set_(d=2), set_(rows=0), set_(x=0), set_(a2=0), set_(b2=0), set_(pe=pe.data_ptr(), seq_len=0)):
        fwd(m)
    fwd(set_(), count=9)
    fwd(set_(), count=0)
    # dropout on the source row without pe: ln_src would silently keep everything
    fwd(set_(drop=L.Dropout(0.1, 3, seed.data_ptr())))
    for m in (set_(d=6), set_(d=2052), set_(rows=0), set_(x=0), set_(a2=0), set_(mean=0), set_(rstd=0), set_(g=0), set_(dx=0)):
        bwd(m)
    bwd(set_(), count=9)
    bwd(set_(), count=0)

    # the single-stream wrapper: parameter gradients without the partial scratch buffer
    S = _BwdStream(L, dev, seed, c, False, F32, 0.0, 0, dx_lp=False)
    da2 = _Out(dev, 1, 8)
    k = S.k
    with pytest.raises(L.MtnHipError):
        L.check(lib.mtn_layernorm_bwd(5, 8, c.eps, _p(k["x"]), _p(k["a2"]), _p(k["mean"]), _p(k["rstd"]), _p(k["g"]), 0, S.dx.ptr(), da2.ptr(), 0,
                                      0, L.stream_ptr()))
    torch.cuda.synchronize()
    assert S.dx.untouched() and da2.untouched()
    # finalize: null partial, no parts
    part = torch.zeros(3, 16, device=dev)
    for F in (L.LnFinalizeDesc(0, 3, 8, da2.ptr(), 0), L.LnFinalizeDesc(part.data_ptr(), 0, 8, da2.ptr(), 0)):
        with pytest.raises(L.MtnHipError):
            L.check(lib.mtn_layernorm_bwd_finalize(1, (L.LnFinalizeDesc * 1)(F), L.stream_ptr()))
    torch.cuda.synchronize()
    assert da2.untouched()


def test_source_dropout_with_pe_still_accepted(dev, hip, seed):
    """The new check refuses only dropout WITHOUT pe: p = 0 without pe and p > 0 with pe both launch."""
    L, lib = hip
    _run_fwd(L, lib, dev, seed, [lr.make_case(3, 8, "a"), lr.make_src("x_pe", 64, 0.5)], F32, what="accepted")
