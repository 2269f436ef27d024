"""LayerNorm backward "by linearity" (include/mtn_hip.h mtn_ln_epilogue), each part run DIRECTLY against float64 references
(tests/ln_epi_refs.py, validated on the CPU by tests/test_ln_epi_refs.py): the consume epilogue on every kernel instance that
carries it, the emit epilogue on every instance, the chain mtn_ln_fold -> emit -> consume on a consistent feed-forward slice,
mtn_ln_fold away from d = 512, groups that mix problems with and without an epilogue, and the emit argument contract.

Consume rows (M, N, K, np, dres, dx_lp, colpart) — CONSUME_ROWS for the 64- and 32-row tiles, CONSUME_ROWS_128X for the 128-row kernel.
Every row ends in a ragged 8-row colpart block (M % 8 != 0).  Stages: 256 elements of K on full stages, 128 on half stages, 64 on the
128 x 128 kernel's ring of four.
  c0  (1, 16, 40, 1, dres, no dx_lp, colpart)        one row; N narrower than every tile (most waves hold no column); one stage; np = 1
  c1  (70, 144, 264, 3, no dres, masked, colpart)    partial 64- / 32-row tile; three 64-column tiles with a ragged last one (16 of 64; 16 of
                                                     32); 2 stages (3 on half stages); np < 8: one gather pass with idle threads
  c2  (135, 512, 520, 10, dres, unmasked, no colpart) three 64-row tiles, the last with 7 rows; the step's width; 3 stages (5 on half
                                                     stages: the two-buffer refill path); np = 10: a second gather pass
  c3  (70, 48, 520, 10, dres, masked, colpart)       N narrower than a 64 tile, 1.5 tiles of 32; long K on a narrow problem
  x0  (1, 16, 264, 1, dres, no dx_lp, colpart)       128 x 128: one row, one 16-column strip; 5 stages = one past the ring of four
  x1  (70, 144, 776, 3, no dres, masked, colpart)    two column tiles, the second 16 wide; 13 stages: the ring wraps three times
  x2  (135, 512, 264, 10, dres, unmasked, no colpart) two row tiles, the second with 7 rows; the step's width
  x3  (135, 48, 776, 10, dres, masked, colpart)      narrow and long
Instances (environment -> census name): CONSUME_VARIANTS.  "nw8" (MTN_GEMM_NW16=0) must give the bits of the default 16-wave run.
Rows that leave dx_lp or colpart out are run a second time with both present: every common output must keep its bits.

Emit shapes (M, N = d_ff, K = d): (70, 64, 40) one block, one stage; (33, 192, 264) three blocks, 2 stages (3 half); (135, 640, 520) three
row tiles x ten blocks, 3 stages (5 half) — each with gate scale 1 and 1 / 0.9, on the default (16 waves), MTN_GEMM_NW16=0 and half-stage
instances; MTN_GEMM_EPI_PRE=0 (the gate from the epilogue's own load) must give the bits of the default.

Bars, and the worst figure measured on an MI355X beside each (every case prints its own):
  consume dx vs consume64                   1e-4                  3.1e-7  (128x x1; the 64- and 32-row instances agree to the digit: 2.1e-7 on c1)
  consume dx_lp vs dx_ref * mask * scale    1e-2                  3.0e-3  (c2), zero pattern exact
  consume da2 / db2 (finalize of colpart)   1e-4                  2.2e-7 / 2.3e-7  (128x x3 / x1)
  group: plain out_f32 / out_lp             1e-5 sqrt(K) / 1e-2   1.5e-7 / 2.9e-3;  its two consumes: dx 1.5e-7, dx_lp 3.0e-3
  emit out_lp vs float64 dh                 1e-2                  3.0e-3  ((33, 192, 264), p = 0.1)
  emit partials vs emit64 on the stored dh  error <= emit_bound   error / bound 0.137 at worst ((135, 640, 520)); 2.5e-6 absolute
  chain dx vs ref_def                       1e-4                  8.2e-8
  chain dx vs ref_true                      1e-4 + 2 gap          1.30e-4, 1.69e-4, 7.05e-5 on the three shapes, with gap = relmax(ref_def,
                                                                  ref_true) = 1.30e-4, 1.69e-4, 7.05e-5: all of it is the method's own cost
  fold u / c vs fold64                      1e-4 max(1, |ref|max) 3.5e-7 / 8.8e-8 absolute (d = 2048, K = 65)
"""
import ctypes as C
import functools
import os

import pytest
import torch

from tests import ln_epi_refs as R
from tests.test_dropout_parity_gpu import _gemm_problem, _keep, _seed
from tests.test_model_gpu import dev  # noqa: F401  (fixture)
from tests.util import lp_round, relmax

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
EPS = 1e-6
P_LP, SALT_LP = 0.5, 4 * 21 + 1
GUARD = 7.0
NAN = float("nan")

D64, D64H = "gemm_dma_kernel<64,64>", "gemm_dma_kernel<64,64> half stages"
D32, D32H = "gemm_dma_kernel<32,32>", "gemm_dma_kernel<32,32> half stages"
CONSUME_VARIANTS = {
    "64": ({"MTN_GEMM_TILE": "64"}, D64),                                     # sixteen waves (the default)
    "64-nw8": ({"MTN_GEMM_TILE": "64", "MTN_GEMM_NW16": "0"}, D64),
    "64-half": ({"MTN_GEMM_TILE": "64", "MTN_GEMM_FORCE_HALF": "1"}, D64H),
    "32": ({"MTN_GEMM_TILE": "32"}, D32),
    "32-half": ({"MTN_GEMM_TILE": "32", "MTN_GEMM_FORCE_HALF": "1"}, D32H),
    "128x": ({"MTN_GEMM_128X_MIN_TILES": "1"}, "gemm_dma128x_kernel"),
}
#                     M    N    K   np  dres   dx_lp       colpart
CONSUME_ROWS = [(1, 16, 40, 1, True, "none", True),
                (70, 144, 264, 3, False, "masked", True),
                (135, 512, 520, 10, True, "unmasked", False),
                (70, 48, 520, 10, True, "masked", True)]
CONSUME_ROWS_128X = [(1, 16, 264, 1, True, "none", True),
                     (70, 144, 776, 3, False, "masked", True),
                     (135, 512, 264, 10, True, "unmasked", False),
                     (135, 48, 776, 10, True, "masked", True)]
CONSUME_CASES = [(v, i) for v in CONSUME_VARIANTS for i in range(4)]


def _rows_of(variant):
    return CONSUME_ROWS_128X if variant == "128x" else CONSUME_ROWS


def test_rows_reach_every_value_per_family():
    """The census of the shape rows themselves: every value the rows are there for appears in each family of instances."""
    for rows, ks in ((CONSUME_ROWS, {40, 264, 520}), (CONSUME_ROWS_128X, {264, 776})):
        col = lambda k: {r[k] for r in rows}
        assert col(0) == {1, 70, 135} and col(1) == {16, 48, 144, 512} and col(2) == ks and col(3) == {1, 3, 10}
        assert col(4) == {True, False} and col(5) == {"none", "unmasked", "masked"} and col(6) == {True, False}
        assert all(r[0] % 8 != 0 for r in rows)


def _launch(env, problems, expect=1):
    """One grouped mtn_gemm under `env`; -> the census name of the kernel that ran."""
    from mtn_amd import lib as L, ops
    lib = L.load()
    try:
        os.environ.update(env)
        L.reload_env()
        lib.mtn_census_begin()
        try:
            ops.gemm(L.MTN_BF16, problems)
            torch.cuda.synchronize()
        finally:
            n = lib.mtn_census_end()
        assert n == expect, n
        info = L.CensusLaunch()
        L.check(lib.mtn_census_info(0, C.byref(info)))
        return lib.mtn_census_variant_name(info.variant).decode()
    finally:
        for k in env:
            os.environ.pop(k, None)
        L.reload_env()


# ------------------------------------------------------------------------------------------ consume
@functools.lru_cache(maxsize=None)
def _consume_data(M, N, K, np_pairs):
    """Operands and float64 references of one consume shape, built once."""
    g = torch.Generator().manual_seed(1000 * M + N + K + np_pairs)
    d = dict(dy=lp_round(torch.randn(M, K, generator=g), BF16), w=lp_round(torch.randn(K, N, generator=g) * K ** -0.5, BF16),     # w: [K][N], b_trans = 1
             x=torch.randn(M, N, generator=g) * 2 + 0.3, a2=1 + 0.3 * torch.randn(N, generator=g), dres=torch.randn(M, N, generator=g))
    gref = d["dy"].double() @ d["w"].double()
    mean, rstd = R.row_stats64(d["x"], EPS)
    s1, p2 = R.row_sums64(gref, d["x"], d["a2"], mean, rstd)
    part = R.deal_partials(s1, p2, np_pairs, g)
    assert float((part.sum(1)[:, 0] - s1).abs().max()) <= 1e-12 * float(part.abs().sum(1).max())
    dx, da2, db2 = R.consume64(gref, d["x"], d["a2"], mean, rstd, EPS, d["dres"])
    d.update(mean=mean.float(), rstd=rstd.float(), part=part.float().contiguous(), dx_dres=dx, dx_plain=dx - d["dres"].double(), da2=da2, db2=db2)
    return d


def _consume_problem(dev, d, M, N, K, np_pairs, has_dres, lp_mode, has_cp, seed):
    """-> (problem, outputs dict, keep-alive list).  Outputs carry their sentinels; part and colpart their guards."""
    from mtn_amd import lib as L, ops
    D = lambda t: t.to(dev).contiguous()
    A, B = d["dy"].to(dev, BF16), d["w"].to(dev, BF16)
    xd, ad, md, rd, dd = D(d["x"]), D(d["a2"]), D(d["mean"]), D(d["rstd"]), D(d["dres"])
    part = torch.cat([d["part"].reshape(-1), torch.full((8,), GUARD)]).to(dev)
    dx = torch.full((M, N), NAN, device=dev)
    dx_lp = torch.full((M, N), GUARD, device=dev, dtype=BF16)
    nparts = L.load().mtn_layernorm_bwd_nparts(M)
    assert nparts == (M + 7) // 8
    colpart = torch.full((nparts + 1, 2 * N), NAN, device=dev)
    colpart[nparts] = GUARD
    e = L.LnEpilogue()
    e.mode, e.part, e.np, e.x, e.a2, e.mean, e.rstd, e.eps, e.dx = 2, part.data_ptr(), np_pairs, xd.data_ptr(), ad.data_ptr(), md.data_ptr(), rd.data_ptr(), EPS, dx.data_ptr()
    if has_dres:
        e.dres = dd.data_ptr()
    if lp_mode != "none":
        e.dx_lp = dx_lp.data_ptr()
        e.dx_lp_drop = ops._drop(P_LP, SALT_LP, seed) if lp_mode == "masked" else ops._drop(0.0, 0, None)
    if has_cp:
        e.colpart = colpart.data_ptr()
    pr = _gemm_problem(L, A, B, M, N, K, 0, 1, K, N)
    pr.ln = C.pointer(e)
    out = dict(dx=dx, dx_lp=dx_lp if lp_mode != "none" else None, colpart=colpart if has_cp else None, part=part, nparts=nparts)
    return pr, out, [e, A, B, xd, ad, md, rd, dd, seed]


def _collect(dev, out, N):
    """Device outputs -> CPU; da2 | db2 through mtn_layernorm_bwd_finalize over the colpart rows."""
    from mtn_amd import lib as L
    got = dict(dx=out["dx"].cpu(), part=out["part"].cpu(), dx_lp=None, colpart=None)
    if out["dx_lp"] is not None:
        got["dx_lp"] = out["dx_lp"].float().cpu()
    if out["colpart"] is not None:
        da, db = torch.full((N,), NAN, device=dev), torch.full((N,), NAN, device=dev)
        desc = (L.LnFinalizeDesc * 1)(L.LnFinalizeDesc(out["colpart"].data_ptr(), out["nparts"], N, da.data_ptr(), db.data_ptr()))
        L.check(L.load().mtn_layernorm_bwd_finalize(1, desc, L.stream_ptr()))
        torch.cuda.synchronize()
        got.update(colpart=out["colpart"].cpu(), da2=da.cpu(), db2=db.cpu())
    return got


_RUNS = {}


def _consume_run(dev, variant, ri, full=False):
    """The outputs of row `ri` on instance `variant` (run once, kept on the CPU).  full: dx_lp and colpart both present."""
    key = (variant, ri, full)
    if key not in _RUNS:
        M, N, K, np_pairs, has_dres, lp_mode, has_cp = _rows_of(variant)[ri]
        if full:
            lp_mode, has_cp = ("masked" if lp_mode == "none" else lp_mode), True
        env, _ = CONSUME_VARIANTS[variant]
        pr, out, hold = _consume_problem(dev, _consume_data(M, N, K, np_pairs), M, N, K, np_pairs, has_dres, lp_mode, has_cp, _seed(dev))
        name = _launch(env, [pr])
        got = _collect(dev, out, N)
        got["name"] = name
        del hold
        _RUNS[key] = got
    return _RUNS[key]


def _check_consume(got, d, M, N, np_pairs, has_dres, lp_mode, has_cp, tag):
    """The assertions every consume output is held to; -> the measured figures."""
    assert torch.equal(got["part"][:-8], d["part"].reshape(-1)) and bool((got["part"][-8:] == GUARD).all()), tag      # read only; guard whole
    dx_ref = d["dx_dres"] if has_dres else d["dx_plain"]
    assert bool(torch.isfinite(got["dx"]).all()), (tag, int((~torch.isfinite(got["dx"])).sum()))
    fig = dict(dx=relmax(got["dx"], dx_ref))
    if lp_mode != "none":
        lp = got["dx_lp"]
        if lp_mode == "masked":
            keep, sm = _keep(SALT_LP, P_LP, (M, N))
            assert torch.equal(lp != 0, keep), (tag, int(((lp != 0) != keep).sum()))
            fig["dx_lp"] = relmax(lp, dx_ref * sm)
        else:
            assert bool((lp != 0).all()), tag
            fig["dx_lp"] = relmax(lp, dx_ref)
    if has_cp:
        cp = got["colpart"]
        assert bool((cp[-1] == GUARD).all()), tag                                   # the row behind the last partial row
        assert bool(torch.isfinite(cp[:-1]).all()), (tag, "a partial row or column tile was never written")
        assert bool(torch.isfinite(got["da2"]).all()) and bool(torch.isfinite(got["db2"]).all()), tag
        fig.update(da2=relmax(got["da2"], d["da2"]), db2=relmax(got["db2"], d["db2"]))
    print(f"ln-consume {tag}: " + " ".join(f"{k}={v:.2e}" for k, v in fig.items()))
    assert fig["dx"] < 1e-4, (tag, fig)
    assert fig.get("dx_lp", 0.0) < 1e-2, (tag, fig)
    assert fig.get("da2", 0.0) < 1e-4 and fig.get("db2", 0.0) < 1e-4, (tag, fig)
    return fig


def _same_bits(a, b, tag):
    for k in ("dx", "dx_lp", "colpart", "da2", "db2"):                      # all float32 on the CPU by now; compared as bit patterns
        if a.get(k) is not None and b.get(k) is not None:
            assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), (tag, k)


@pytest.mark.parametrize("variant,ri", CONSUME_CASES, ids=[f"{v}-{'x' if v == '128x' else 'c'}{i}" for v, i in CONSUME_CASES])
def test_consume_epilogue(dev, variant, ri):
    """mtn_gemm with ln.mode = MTN_LN_CONSUME on one kernel instance and one shape row: dx, the masked / unmasked bf16 copy and da2 | db2
    (colpart through mtn_layernorm_bwd_finalize) against float64 autograd of the oracle's layer_norm on g = dy W in float64; the two row
    sums arrive as np float32 pairs dealt on the host from that g.  Sentinels: dx NaN, dx_lp 7, colpart NaN + a guard row, part + a guard."""
    row = _rows_of(variant)[ri]
    M, N, K, np_pairs, has_dres, lp_mode, has_cp = row
    d = _consume_data(M, N, K, np_pairs)
    got = _consume_run(dev, variant, ri)
    want = CONSUME_VARIANTS[variant][1]
    assert got["name"].startswith(want) and ("half" in got["name"]) == ("half" in want), (got["name"], want)
    tag = f"{variant} {row}"
    _check_consume(got, d, M, N, np_pairs, has_dres, lp_mode, has_cp, tag)
    if lp_mode == "none" or not has_cp:                       # leaving an optional output out changes nothing else
        full = _consume_run(dev, variant, ri, full=True)
        _check_consume(full, d, M, N, np_pairs, has_dres, "masked" if lp_mode == "none" else lp_mode, True, tag + " (all outputs)")
        _same_bits(got, full, tag)
    if variant == "64-nw8":                                   # the eight-wave form: the bits of the sixteen-wave one
        _same_bits(got, _consume_run(dev, "64", ri), tag + " vs 16 waves")


def test_group_mixes_plain_and_epilogue_problems(dev):
    """One launch: consume (70, 144, 264, np = 3), a plain dX problem (B as it lies, residual + both outputs, the bf16 copy masked after
    the residual), consume (33, 48, 40, np = 1) — slot_of must hand each problem its own epilogue slot, and the plain one none.  Then
    nine epilogue problems in one launch: refused (eight slots)."""
    from mtn_amd import lib as L, ops
    seed = _seed(dev)
    shapes = [(70, 144, 264, 3), (33, 48, 40, 1)]
    cons = []
    for M, N, K, np_pairs in shapes:
        d = _consume_data(M, N, K, np_pairs)
        cons.append((d, M, N, np_pairs) + _consume_problem(dev, d, M, N, K, np_pairs, True, "masked", True, seed))
    M, N, K, salt, p = 104, 72, 136, 4 * 11 + 2, 0.5
    g = torch.Generator().manual_seed(9)
    a, b, res = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g), torch.randn(M, N, generator=g)
    A, B, Res = a.to(dev, BF16), b.t().contiguous().to(dev, BF16), res.to(dev)
    of = torch.full((M, N), NAN, device=dev)
    ol = torch.full((M, N), GUARD, device=dev, dtype=BF16)
    plain = _gemm_problem(L, A, B, M, N, K, 0, 1, K, N)
    plain.residual, plain.ldr, plain.out_f32, plain.out_lp, plain.ldc, plain.lp_drop_after_residual = Res.data_ptr(), N, of.data_ptr(), ol.data_ptr(), N, 1
    plain.drop = ops._drop(p, salt, seed)
    name = _launch({}, [cons[0][4], plain, cons[1][4]])
    assert name.startswith("gemm_dma_kernel<"), name
    v = lp_round(a, BF16).double() @ lp_round(b, BF16).double().t() + res.double()
    keep, sm = _keep(salt, p, (M, N))
    gf, gl = of.cpu(), ol.float().cpu()
    assert torch.equal(gl != 0, keep)
    e_f, e_l = relmax(gf, v), relmax(gl, v * sm)
    print(f"ln-group plain problem: out_f32 {e_f:.2e} out_lp {e_l:.2e} ({name})")
    assert e_f < 1e-5 * K ** 0.5 and e_l < 1e-2, (e_f, e_l)
    for d, Mc, Nc, np_pairs, _pr, out, _hold in cons:
        _check_consume(_collect(dev, out, Nc), d, Mc, Nc, np_pairs, True, "masked", True, f"group {(Mc, Nc, np_pairs)}")
    # nine problems with an epilogue: one more than the launch has slots for (the same small problem nine times: a host check)
    d = _consume_data(33, 48, 40, 1)
    pr, out, _hold = _consume_problem(dev, d, 33, 48, 40, 1, True, "none", False, seed)
    with pytest.raises(L.MtnHipError, match="too many"):
        ops.gemm(L.MTN_BF16, [pr] * 9)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out["dx"]).all())                 # refused before any launch


# ------------------------------------------------------------------------------------------ emit
EMIT_VARIANTS = {"default": ({}, D64), "nw8": ({"MTN_GEMM_NW16": "0"}, D64), "half": ({"MTN_GEMM_FORCE_HALF": "1"}, D64H),
                 "nopre": ({"MTN_GEMM_EPI_PRE": "0"}, D64)}
EMIT_SHAPES = [(70, 64, 40), (33, 192, 264), (135, 640, 520)]
EMIT_P = [0.0, 0.1]


def _f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


@functools.lru_cache(maxsize=None)
def _emit_data(M, N, K):
    g = torch.Generator().manual_seed(M + N + K)
    rn = lambda *s: torch.randn(*s, generator=g)
    dy, w2 = lp_round(rn(M, K), BF16), lp_round(rn(K, N) * K ** -0.5, BF16)                 # w2 [K = d][N = d_ff] as it lies
    hid = lp_round(rn(M, N), BF16)                                                          # about half <= 0 ...
    hid[:, ::7] = 0.0                                                                       # ... some of them exact zeros
    w1, b1, a2, b2 = lp_round(rn(N, 64) * 0.125, BF16), 0.1 * rn(N), 1 + 0.3 * rn(64), 0.2 * rn(64)
    u, c = R.fold64(w1, b1, a2, b2)
    return dict(dy=dy, w2=w2, hid=hid, fold=torch.cat([u, c]).float().contiguous(), v=dy.double() @ w2.double())


def _emit_problem(dev, dy, w2, hid, fold, M, N, K, gate_scale, ldc=None, gate=True):
    from mtn_amd import lib as L
    ldc = N if ldc is None else ldc
    A, B, F = dy.to(dev, BF16), w2.to(dev, BF16), fold.to(dev)
    G = torch.zeros(M, ldc, device=dev, dtype=BF16)
    G[:, :N] = hid.to(dev, BF16)
    dh = torch.full((M, ldc), GUARD, device=dev, dtype=BF16)
    nblk = N // 64
    part = torch.full((M * nblk * 2 + 8,), NAN, device=dev)
    part[-8:] = GUARD
    e = L.LnEpilogue()
    e.mode, e.fold, e.gate_inv_scale, e.part = 1, F.data_ptr(), _f32(1.0 / _f32(gate_scale)), part.data_ptr()
    pr = _gemm_problem(L, A, B, M, N, K, 0, 1, K, N)
    pr.gate, pr.gate_scale, pr.out_lp, pr.ldc = (G.data_ptr() if gate else None), _f32(gate_scale), dh.data_ptr(), ldc
    pr.ln = C.pointer(e)
    return pr, dh, part, [e, A, B, F, G]


_EMITS = {}


def _emit_run(dev, variant, si, p):
    key = (variant, si, p)
    if key not in _EMITS:
        M, N, K = EMIT_SHAPES[si]
        d = _emit_data(M, N, K)
        pr, dh, part, hold = _emit_problem(dev, d["dy"], d["w2"], d["hid"], d["fold"], M, N, K, 1.0 / (1.0 - p))
        name = _launch(EMIT_VARIANTS[variant][0], [pr])
        _EMITS[key] = dict(name=name, dh=dh.float().cpu(), part=part.cpu())
        del hold
    return _EMITS[key]


def _check_emit(dh, part, hid, fold, v64, gate_scale, M, N, tag):
    """out_lp against the float64 dh; the partials against their definition over the STORED out_lp, inside the derived bound."""
    gs, nblk = _f32(gate_scale), N // 64
    inv = _f32(1.0 / gs)
    want = torch.where(hid > 0, v64 * gs, torch.zeros_like(v64))
    assert bool((dh[hid <= 0] == 0).all()), tag
    e_dh = relmax(dh, want)
    assert bool((part[-8:] == GUARD).all()), tag
    got = part[:-8].reshape(M, nblk, 2)
    assert bool(torch.isfinite(got).all()), (tag, int((~torch.isfinite(got)).sum()))
    u, c = fold[:N], fold[N:]
    err = (got.double() - R.emit64(dh, hid, inv, u, c)).abs()
    bound = R.emit_bound(dh, hid, inv, u, c)
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f"ln-emit {tag}: out_lp {e_dh:.2e} partial error / bound {ratio:.3f} (worst abs {float(err.max()):.2e})")
    assert e_dh < 1e-2, (tag, e_dh)
    assert bool((err <= bound).all()), (tag, ratio, int((err > bound).sum()))
    return e_dh, ratio


@pytest.mark.parametrize("si", range(len(EMIT_SHAPES)), ids=["x".join(map(str, s)) for s in EMIT_SHAPES])
@pytest.mark.parametrize("variant", list(EMIT_VARIANTS))
def test_emit_epilogue(dev, variant, si):
    """mtn_gemm with ln.mode = MTN_LN_EMIT: dh = (dy W2) gated by the saved hidden, and per row and 64-column block the pair
    {sum dh u, sum dh (hid / scale - c)} over the value the consumer will read (the bf16 dh)."""
    M, N, K = EMIT_SHAPES[si]
    d = _emit_data(M, N, K)
    for p in EMIT_P:
        got = _emit_run(dev, variant, si, p)
        assert got["name"] == EMIT_VARIANTS[variant][1], got["name"]
        _check_emit(got["dh"], got["part"], d["hid"], d["fold"], d["v"], 1.0 / (1.0 - p), M, N, f"{variant} {(M, N, K)} p={p}")
        if variant == "nopre":                                # the gate from the epilogue's own load: the same bits
            ref = _emit_run(dev, "default", si, p)
            assert torch.equal(got["dh"], ref["dh"]) and torch.equal(got["part"].view(torch.int32), ref["part"].view(torch.int32))


@pytest.mark.parametrize("what", ["no_gate", "ldc"])
def test_emit_contract_is_refused(dev, what):
    """The second partial needs the gate VALUE, which the GEMM epilogue reports on its 16-byte path only: an emit problem without a
    gate, or with ldc % 4 != 0, is refused by mtn_gemm's argument check (before this check it ran and wrote -sum v c).  Nothing launches."""
    from mtn_amd import lib as L, ops
    M, N, K = EMIT_SHAPES[0]
    d = _emit_data(M, N, K)
    pr, dh, part, _hold = _emit_problem(dev, d["dy"], d["w2"], d["hid"], d["fold"], M, N, K, 1.0, ldc=N + 2 if what == "ldc" else None, gate=what != "no_gate")
    lib = L.load()
    lib.mtn_census_begin()
    try:
        with pytest.raises(L.MtnHipError, match="emit"):
            ops.gemm(L.MTN_BF16, [pr])
        torch.cuda.synchronize()
    finally:
        n = lib.mtn_census_end()
    assert n == 0
    assert bool((dh.float() == GUARD).all()) and bool(torch.isnan(part[:-8]).all())


# ------------------------------------------------------------------------------------------ fold, directly
def _fold_launch(dev, d, items):
    """items: [(w bf16-valued [K, d], bias or None, a2, b2)] -> [out tensor [2K + 8] on the device], one mtn_ln_fold launch."""
    from mtn_amd import lib as L
    descs = (L.LnFoldDesc * len(items))()
    hold, outs, block_desc, blocks = [], [], [], 0
    for i, (w, bias, a2, b2) in enumerate(items):
        K = w.size(0)
        W, A2, B2 = w.to(dev, BF16).contiguous(), a2.to(dev).contiguous(), b2.to(dev).contiguous()
        Bi = None if bias is None else bias.to(dev).contiguous()
        out = torch.full((2 * K + 8,), NAN, device=dev)
        out[2 * K:] = GUARD
        descs[i].w, descs[i].bias, descs[i].a2, descs[i].b2 = W.data_ptr(), (None if Bi is None else Bi.data_ptr()), A2.data_ptr(), B2.data_ptr()
        descs[i].out, descs[i].K, descs[i].block_start = out.data_ptr(), K, blocks
        nb = (K + 63) // 64
        block_desc += [i] * nb
        blocks += nb
        hold += [W, A2, B2, Bi]
        outs.append(out)
    table = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).to(dev)
    bd = torch.tensor(block_desc, dtype=torch.int32).to(dev)
    L.check(L.load().mtn_ln_fold(L.MTN_BF16, table.data_ptr(), bd.data_ptr(), blocks, d, L.stream_ptr()))
    torch.cuda.synchronize()
    del hold
    return outs


@pytest.mark.parametrize("d", [8, 96, 512, 520, 2048])
def test_ln_fold_direct(dev, d):
    """mtn_ln_fold on a hand-built descriptor table: K = 1 (one row, seven idle waves), 65 (a second block of one row) and 200 (a ragged
    last block; no bias) in one launch; d = 8 and 96 (one and twelve live lanes), 512 (all), 520 and 2048 (the four-chunk kernel with one
    live lane / every lane in its last chunk).  Each out [2K] starts as NaN with a guard behind it."""
    g = torch.Generator().manual_seed(d)
    rn = lambda *s: torch.randn(*s, generator=g)
    items = [(lp_round(rn(K, d) * d ** -0.5, BF16), (None if K == 200 else 0.5 * rn(K)), 1 + 0.3 * rn(d), 0.2 * rn(d)) for K in (1, 65, 200)]
    outs = _fold_launch(dev, d, items)
    for (w, bias, a2, b2), out in zip(items, outs):
        K = w.size(0)
        got = out.cpu()
        assert bool((got[2 * K:] == GUARD).all()), (d, K)
        assert bool(torch.isfinite(got[:2 * K]).all()), (d, K)
        u, c = R.fold64(w, bias, a2, b2)
        eu, ec = float((got[:K].double() - u).abs().max()), float((got[K:2 * K].double() - c).abs().max())
        print(f"ln-fold d={d} K={K} bias={'no' if bias is None else 'yes'}: u {eu:.2e} (|u|max {float(u.abs().max()):.2f}) c {ec:.2e} (|c|max {float(c.abs().max()):.2f})")
        assert eu < 1e-4 * max(1.0, float(u.abs().max())) and ec < 1e-4 * max(1.0, float(c.abs().max())), (d, K, eu, ec)


# ------------------------------------------------------------------------------------------ the chain fold -> emit -> consume
@pytest.mark.parametrize("rows,d,d_ff", [(70, 64, 640), (33, 48, 192), (135, 512, 192)])
def test_fold_emit_consume_chain(dev, rows, d, d_ff):
    """The three kernels as the feed-forward backward chains them, on a consistent slice (q = W1 LN(x) + b1, hid = bf16(relu(q) mask /
    (1 - p)), p = 0.1): mtn_ln_fold of W1, the emit GEMM dh = (dy W2) gated with its partials, the consume GEMM g = dh W1 reading them
    (np = d_ff / 64).  Both references start from the DEVICE's dh: ref_def = the header's formula on the float64 partials of their
    definition; ref_true = float64 autograd on g = dh W1.  Their distance is the method's own cost of reading q back from the bf16 hid."""
    from mtn_amd import lib as L
    s = R.ffn_slice(rows, d, d_ff, 0.1, seed=rows + d_ff)
    hid = lp_round(s.hid.float(), BF16)
    assert torch.equal(hid > 0, s.hid > 0)
    out_fold, = _fold_launch(dev, d, [(s.w1, s.b1, s.a2, s.b2)])
    u64, c64 = R.fold64(s.w1, s.b1, s.a2, s.b2)
    fold = out_fold[:2 * d_ff]
    e_fold = max(float((fold[:d_ff].double().cpu() - u64).abs().max()) / max(1.0, float(u64.abs().max())),
                 float((fold[d_ff:].double().cpu() - c64).abs().max()) / max(1.0, float(c64.abs().max())))
    assert e_fold < 1e-4, e_fold
    pe, dh, part, hold_e = _emit_problem(dev, s.dy, s.w2, hid, fold.cpu(), rows, d_ff, d, s.scale)
    pe.ln.contents.fold = fold.data_ptr()                                  # the device's own fold vectors, not a copy
    assert _launch({}, [pe]) == D64
    dh_dev = dh.float().cpu()
    assert bool((dh_dev[hid <= 0] == 0).all()) and relmax(dh_dev, s.dh) < 1e-2
    # consume on the device's dh and partials
    np_pairs = d_ff // 64
    cd = dict(dy=dh_dev, w=s.w1, x=s.x, a2=s.a2, dres=s.dres, mean=s.mean.float(), rstd=s.rstd.float(), part=part[:-8].cpu().reshape(rows, np_pairs, 2))
    pc, out, hold_c = _consume_problem(dev, cd, rows, d, d_ff, np_pairs, True, "none", True, None)
    pc.ln.contents.part = part.data_ptr()
    name = _launch({}, [pc])
    assert name.startswith("gemm_dma_kernel<"), name
    got = _collect(dev, out, d)
    assert bool((part[-8:].cpu() == GUARD).all())
    # references from the device's dh
    gs, inv = _f32(s.scale), _f32(1.0 / _f32(s.scale))
    p64 = R.emit64(dh_dev, hid, inv, u64, c64).sum(1)
    g64 = dh_dev.double() @ s.w1.double()
    ref_def = R.consume64_from_sums(p64[:, 0], p64[:, 1], g64, s.x, s.a2, s.mean, s.rstd, s.eps, s.dres)
    ref_true, da2, db2 = R.consume64(g64, s.x, s.a2, s.mean, s.rstd, s.eps, s.dres)
    assert bool(torch.isfinite(got["dx"]).all())
    gap, e_def, e_true = relmax(ref_def, ref_true), relmax(got["dx"], ref_def), relmax(got["dx"], ref_true)
    e_a, e_b = relmax(got["da2"], da2), relmax(got["db2"], db2)
    print(f"ln-chain {(rows, d, d_ff)}: fold {e_fold:.2e} dx vs ref_def {e_def:.2e} vs ref_true {e_true:.2e} (ref_def vs ref_true {gap:.2e}) da2 {e_a:.2e} db2 {e_b:.2e} ({name}, scale {gs})")
    assert e_def < 1e-4, (e_def, gap)
    assert e_true < 1e-4 + 2 * gap, (e_true, gap)
    assert bool((got["colpart"][-1] == GUARD).all()) and e_a < 1e-4 and e_b < 1e-4, (e_a, e_b)
    del hold_e, hold_c
