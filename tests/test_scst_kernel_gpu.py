"""The kernels of self-critical sequence training (csrc/scst.hip) through the C ABI and through mtn_amd.ops against the numpy definitions
of tests/scst_refs.py (validated without a GPU by tests/test_scst_refs.py); outputs and guard regions are pre-filled with NaN / sentinels.

Weighted loss head: the kernel is the loss head's float32 closed form with one more factor per row, so its bars are the ones
tests/test_distill_kernel_gpu.py holds rowloss and dlogits to (4x what float32 delivers on the closed form on a CPU,
distill_refs.CPU_F32_DISTILL_*): lse absolute, rowloss relative to the case's largest |rowloss|, dlogits relative to max |ref|, bfloat16
dlogits + 1 bfloat16 ulp of the reference element (one rounding of the float32 value).  None was obtained by running the kernel.
Rewards: integers exact, doubles within 1e-9 (tests/test_eval_kernel_gpu.py's bar and reasoning).  Assemble and advantage: exact."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import distill_refs as dr
from tests import row_refs as rr
from tests import scst_refs as sr

pytestmark = pytest.mark.gpu

LSE_ABS = 4 * dr.CPU_F32_DISTILL_LSE
ROWLOSS_REL = 4 * dr.CPU_F32_DISTILL_ROWLOSS
DLOGITS_REL = 4 * dr.CPU_F32_DISTILL_DLOGITS
TOL = 1e-9
NAN = float("nan")
PAD_SENTINEL = 1e30
SMOOTHINGS = {"sm0": (0.1, (0.0, 0.0, 0.0)), "sm0.1-inherited": (0.1, (-1.0, -1.0, -1.0)), "mixed": (0.1, (0.0, 0.1, -1.0))}


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


class _Head:
    """Device buffers of one loss-head case: lse / rowloss carry 4 extra elements and dlogits one extra row, all NaN; the padding columns
    of the logits hold 1e30; the weights of segment s lie 4-byte (not 16-byte) aligned.  ``A``: the weighted block, ``H``: the plain
    loss head's on the SAME buffers."""

    def __init__(self, L, dev, V, z, targets, weights, smoothing, smoothing_seg, ldz_pad=12, ldd_pad=4):
        self.rows, self.V = z.shape[0], V
        self.ldz, self.ldd = V + ldz_pad, V + ldd_pad
        zb = torch.full((self.rows, self.ldz), PAD_SENTINEL)
        zb[:, :V] = torch.from_numpy(z)
        self.z0, self.z = zb, zb.to(dev)
        self.targets = [torch.from_numpy(t).to(dev) for t in targets]
        self.w = [None if w is None else torch.cat([torch.full((1,), NAN), torch.from_numpy(w)]).to(dev)[1:] for w in weights]
        self.norm = torch.tensor(sr.NORM, device=dev)
        self.gloss = torch.tensor([sr.GLOSS], device=dev)
        self.lse = torch.full((self.rows + 4,), NAN, device=dev)
        self.rowloss = torch.full((self.rows + 4,), NAN, device=dev)
        self.A, self.H = L.WLossHeadArgs(), L.LossHeadArgs()
        for A in (self.A, self.H):
            A.n_seg = len(targets)
            for s, t in enumerate(targets):
                A.rows[s], A.target[s], A.norm[s], A.coef[s] = t.size, self.targets[s].data_ptr(), self.norm.data_ptr() + 4 * s, sr.COEF[s]
            A.V, A.ldz, A.pad, A.smoothing = V, self.ldz, sr.PAD, smoothing
            A.logits, A.lse, A.rowloss, A.gloss = self.z.data_ptr(), self.lse.data_ptr(), self.rowloss.data_ptr(), self.gloss.data_ptr()
        for s, w in enumerate(self.w):
            self.A.roww[s] = 0 if w is None else w.data_ptr()
            self.A.smoothing_seg[s] = smoothing_seg[s]
        self.new_dz(dev, torch.float32)

    def new_dz(self, dev, dtype):
        self.dz = torch.full((self.rows + 1, self.ldd), NAN, device=dev, dtype=dtype)
        self.A.dlogits = self.H.dlogits = self.dz.data_ptr()
        self.A.ldd = self.H.ldd = self.ldd


@pytest.mark.parametrize("V", [64, 104])
@pytest.mark.parametrize("sm", list(SMOOTHINGS))
def test_weighted_loss_head(dev, hip, V, sm):
    """lse, rowloss and their sum, dlogits in float32 and bfloat16 against the float64 definition: negative, zero and unit weights, zeroed
    <pad> rows, the quirk row, smoothing 0 / 0.1 per segment.  Zero-weight and zeroed rows hold +0.0, the padding columns +0.0, guards and
    inputs are untouched, two launches give equal bytes."""
    L, lib = hip
    smoothing, seg = SMOOTHINGS[sm]
    z, targets, weights = sr.head_inputs(V, 40 + V)
    eff = [smoothing if s < 0 else s for s in seg]
    ref = sr.weighted_loss_head(z, targets, weights, eff, V, sr.PAD, sr.COEF, sr.NORM, sr.GLOSS)
    R = _Head(L, dev, V, z, targets, weights, smoothing, seg)
    L.check(lib.mtn_wlosshead_fwd(C.byref(R.A), L.stream_ptr()))
    torch.cuda.synchronize()
    n = R.rows
    lse, rowloss = R.lse.cpu(), R.rowloss.cpu()
    assert _all_nan(lse[n:]) and _all_nan(rowloss[n:]) and not torch.isnan(lse[:n]).any() and not torch.isnan(rowloss[:n]).any()
    big = float(np.abs(ref["rowloss"]).max())
    e_lse = float(np.abs(lse[:n].double().numpy() - ref["lse"]).max())
    e_row = float(np.abs(rowloss[:n].double().numpy() - ref["rowloss"]).max()) / big
    e_sum = abs(float(rowloss[:n].double().sum()) - ref["total"])
    print(f"lse abs {e_lse:.3e} (bound {LSE_ABS:.3e})  rowloss rel {e_row:.3e} (bound {ROWLOSS_REL:.3e})  sum abs {e_sum:.3e}")
    assert e_lse <= LSE_ABS and e_row <= ROWLOSS_REL and e_sum <= ROWLOSS_REL * big * n
    zero = torch.from_numpy(ref["zero"])
    assert bool((_bits(rowloss[:n][zero]) == 0).all())                                   # +0.0, not -0.0
    signs = np.sign(ref["rowloss"][~ref["zero"]])
    assert (np.sign(rowloss[:n].numpy()[~ref["zero"]]) == signs).all() and (signs < 0).any() and (signs > 0).any()
    assert _same_bits(R.z.cpu(), R.z0)

    want64 = torch.from_numpy(ref["dlogits"])
    dmax = float(want64.abs().max())
    for dtype in (torch.float32, torch.bfloat16):
        R.new_dz(dev, dtype)
        L.check(lib.mtn_wlosshead_bwd(L.dtype_code(dtype), C.byref(R.A), L.stream_ptr()))
        torch.cuda.synchronize()
        dz = R.dz.cpu()
        assert _all_nan(dz[n])
        assert bool((_bits(dz[:n, V:]) == 0).all())                                      # columns V..ldd-1: +0.0 in every row
        assert bool((_bits(dz[:n][zero]) == 0).all())                                    # zero weights and zeroed rows: +0.0
        got = dz[:n, :V].double()
        assert not torch.isnan(got).any()
        if dtype == torch.float32:
            want, tol = want64, torch.full_like(got, DLOGITS_REL * dmax)
        else:
            want, tol = want64.to(torch.bfloat16).double(), rr.bf16_ulp(want64) + DLOGITS_REL * dmax
        err = (got - want).abs()
        print(f"{dtype}: dlogits worst err / bound {float((err / tol).max()):.3f}, rel to max {float(err.max()) / dmax:.3e}")
        assert bool((err <= tol).all())
        first = R.dz
        R.new_dz(dev, dtype)
        L.check(lib.mtn_wlosshead_bwd(L.dtype_code(dtype), C.byref(R.A), L.stream_ptr()))
        torch.cuda.synchronize()
        assert _same_bits(R.dz, first) and _same_bits(R.lse.cpu()[:n], lse[:n]) and _same_bits(R.z.cpu(), R.z0)
    L.check(lib.mtn_wlosshead_fwd(C.byref(R.A), L.stream_ptr()))
    torch.cuda.synchronize()
    assert _same_bits(R.lse.cpu(), lse) and _same_bits(R.rowloss.cpu(), rowloss)


@pytest.mark.parametrize("V", [64, 104])
@pytest.mark.parametrize("smoothing", [0.1, 0.0])
@pytest.mark.parametrize("how", ["inherit", "restated"])
def test_without_weights_the_bits_are_the_loss_heads(dev, hip, V, smoothing, how):
    """roww == NULL on every segment at the loss head's smoothing (taken from `smoothing`, or restated per segment): lse, rowloss and
    dlogits (float32 and bfloat16) equal mtn_losshead_fwd / _bwd on the same buffers bit for bit."""
    L, lib = hip
    z, targets, _ = sr.head_inputs(V, 50 + V)
    seg = (-1.0,) * 3 if how == "inherit" else (smoothing,) * 3
    R = _Head(L, dev, V, z, targets, [None] * 3, smoothing, seg)
    n = R.rows
    L.check(lib.mtn_losshead_fwd(C.byref(R.H), L.stream_ptr()))
    torch.cuda.synchronize()
    lse_h, row_h = R.lse.clone(), R.rowloss.clone()
    assert not torch.isnan(row_h[:n]).any()
    R.lse.fill_(NAN); R.rowloss.fill_(NAN)
    L.check(lib.mtn_wlosshead_fwd(C.byref(R.A), L.stream_ptr()))
    torch.cuda.synchronize()
    assert _same_bits(R.lse, lse_h) and _same_bits(R.rowloss, row_h)
    for dtype in (torch.float32, torch.bfloat16):
        R.new_dz(dev, dtype)
        L.check(lib.mtn_losshead_bwd(L.dtype_code(dtype), C.byref(R.H), L.stream_ptr()))
        torch.cuda.synchronize()
        dz_h = R.dz
        R.new_dz(dev, dtype)
        L.check(lib.mtn_wlosshead_bwd(L.dtype_code(dtype), C.byref(R.A), L.stream_ptr()))
        torch.cuda.synchronize()
        assert _same_bits(R.dz, dz_h) and not torch.isnan(R.dz[:n]).any()


def test_weighted_head_argument_checks_leave_the_guards(dev, hip):
    L, lib = hip
    z, targets, weights = sr.head_inputs(64, 3)
    for kw in (dict(roww=(0, 2)), dict(smoothing_seg=(1, NAN)), dict(V=62), dict(n_seg=5), dict(pad=64), dict(ldz=60)):
        R = _Head(L, dev, 64, z, targets, weights, 0.1, (0.0, 0.1, -1.0))
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(R.A, k)[v[0]] = (getattr(R.A, k)[v[0]] or 0) + v[1] if k == "roww" else v[1]
            else:
                setattr(R.A, k, v)
        with pytest.raises(L.MtnHipError):
            L.check(lib.mtn_wlosshead_fwd(C.byref(R.A), L.stream_ptr()))
        for code in (L.MTN_F32, L.MTN_BF16):
            with pytest.raises(L.MtnHipError):
                L.check(lib.mtn_wlosshead_bwd(code, C.byref(R.A), L.stream_ptr()))
        torch.cuda.synchronize()
        assert _all_nan(R.dz) and _all_nan(R.lse) and _all_nan(R.rowloss)


# ------------------------------------------------------------------------------------------ rewards against a fixed corpus
@pytest.fixture(scope="module")
def corpus(dev):
    from mtn_amd import ops
    ref_sets, hyps, items = sr.reward_corpus()
    Rm, Lm, ldl = 3, 12, 16
    ref_np, ref_len, n_ref = sr.pack_corpus(ref_sets, Rm, ldl, fill=3)                   # garbage that occurs in the corpus
    ref = torch.from_numpy(ref_np).to(dev)[:, :, :Lm]
    d = dict(ref_sets=ref_sets, hyps=hyps, items=items, R=Rm, L=Lm, ldl=ldl, ref=ref, ref_len=torch.from_numpy(ref_len).to(dev),
             n_ref=torch.from_numpy(n_ref).to(dev))
    d["table"] = ops.eval_table_build(d["ref"], d["ref_len"], d["n_ref"])
    d["want"] = sr.rewards(hyps, items, ref_sets)
    return d


def _rows_on_device(dev, hyps, ldl, Lm):
    hyp_np, hyp_len = sr.pack_rows(hyps, ldl, fill=3)
    return torch.from_numpy(hyp_np).to(dev)[:, :Lm], torch.from_numpy(hyp_len).to(dev)


def test_rewards_of_rows_against_the_corpus_table(dev, corpus):
    """N = 10 hypotheses of lengths 0, 1, 3 and L among them, naming repeated and permuted items of a corpus of 7: integers exact,
    doubles within 1e-9; outputs carry a NaN / sentinel guard row; two calls give equal bytes; the table is not written."""
    from mtn_amd import ops
    c = corpus
    hyp, hyp_len = _rows_on_device(dev, c["hyps"], c["ldl"], c["L"])
    item = torch.tensor(c["items"], dtype=torch.int32, device=dev)
    N = len(c["hyps"])
    table0 = c["table"].clone()

    def run():
        stats = torch.full((N + 1, 10), -77, dtype=torch.int32, device=dev)
        rouge = torch.full((N + 1,), NAN, dtype=torch.float64, device=dev)
        cider = torch.full((N + 1,), NAN, dtype=torch.float64, device=dev)
        ops.eval_score_rows(hyp, hyp_len, item, c["ref"], c["ref_len"], c["n_ref"], c["table"], out=(stats[:N], rouge[:N], cider[:N]))
        torch.cuda.synchronize()
        return stats.cpu(), rouge.cpu(), cider.cpu()

    stats, rouge, cider = run()
    want = c["want"]
    assert (stats[:N].numpy() == want["stats"]).all() and bool((stats[N] == -77).all())
    assert _all_nan(rouge[N:]) and _all_nan(cider[N:])
    e_r, e_c = np.abs(rouge[:N].numpy() - want["rouge"]).max(), np.abs(cider[:N].numpy() - want["cider"]).max()
    print(f"rouge abs {e_r:.3e}  cider abs {e_c:.3e}  (bound {TOL:.0e});  cider {np.round(want['cider'], 3).tolist()}")
    assert e_r <= TOL and e_c <= TOL
    assert float(want["cider"].max()) > 0.1 and float(want["rouge"].max()) > 0.1        # the case scores something
    again = run()
    assert all(_same_bits(a, b) for a, b in zip((stats, rouge, cider), again))
    assert torch.equal(c["table"], table0)


def test_one_hypothesis_per_item_in_order_is_eval_metrics(dev, corpus):
    """N = Qc, item[n] = n: cider, rouge and stats are mtn_eval_metrics's bytes on the same corpus."""
    from mtn_amd import ops
    c = corpus
    Qc = len(c["ref_sets"])
    hyps = [list(refs[-1][1:]) + [q % 6] for q, refs in enumerate(c["ref_sets"])]
    hyps = [h[:c["L"]] for h in hyps]
    hyp, hyp_len = _rows_on_device(dev, hyps, c["ldl"], c["L"])
    item = torch.arange(Qc, dtype=torch.int32, device=dev)
    stats, rouge, cider = ops.eval_score_rows(hyp, hyp_len, item, c["ref"], c["ref_len"], c["n_ref"], c["table"])
    m_stats, m_rouge, m_cider, _, _ = ops.eval_metrics(hyp, hyp_len, c["ref"], c["ref_len"], c["n_ref"])
    torch.cuda.synchronize()
    assert _same_bits(stats, m_stats) and _same_bits(rouge, m_rouge) and _same_bits(cider, m_cider)
    want = sr.rewards(hyps, list(range(Qc)), c["ref_sets"])
    assert (stats.cpu().numpy() == want["stats"]).all() and np.abs(cider.cpu().numpy() - want["cider"]).max() <= TOL
    assert float(cider.max()) > 0.1


def test_an_item_outside_the_corpus_is_clamped(dev, corpus):
    from mtn_amd import ops
    c = corpus
    hyp, hyp_len = _rows_on_device(dev, [c["hyps"][3]] * 4, c["ldl"], c["L"])
    item = torch.tensor([-5, 0, 6, 1000], dtype=torch.int32, device=dev)
    _, rouge, cider = ops.eval_score_rows(hyp, hyp_len, item, c["ref"], c["ref_len"], c["n_ref"], c["table"])
    torch.cuda.synchronize()
    assert _same_bits(cider[0], cider[1]) and _same_bits(cider[2], cider[3]) and _same_bits(rouge[0], rouge[1]) and _same_bits(rouge[2], rouge[3])


# ------------------------------------------------------------------------------------------ assemble and advantage
@pytest.mark.parametrize("T", [5, 7])
def test_assemble_cuts_every_case(dev, T):
    """6 rows, L = 5: <eos> at 0, at L - 1, nowhere, in the middle, twice, at 1.  Exact; hyp columns past L and the guard rows keep
    their sentinel."""
    from mtn_amd import ops
    sos, eos, pad, Lm, ldh = 0, 2, 1, 5, 8
    log = sr.assemble_log(eos, Lm)
    rows = log.shape[1]
    trg = torch.full((rows + 1, T), -9, dtype=torch.long, device=dev)
    trg_y = torch.full((rows + 1, T), -9, dtype=torch.long, device=dev)
    hyp = torch.full((rows + 1, ldh), -9, dtype=torch.int32, device=dev)
    hyp_len = torch.full((rows + 1,), -9, dtype=torch.int32, device=dev)
    ops.scst_assemble(torch.from_numpy(log).to(dev), sos, eos, pad, T=T, out=(trg[:rows], trg_y[:rows], hyp[:rows, :Lm], hyp_len[:rows]),
                      hyp_stride=ldh)
    torch.cuda.synchronize()
    w_trg, w_trg_y, w_hyp, w_len = sr.assemble(log, sos, eos, pad, T)
    assert (trg[:rows].cpu().numpy() == w_trg).all() and (trg_y[:rows].cpu().numpy() == w_trg_y).all()
    assert (hyp[:rows, :Lm].cpu().numpy() == w_hyp).all() and (hyp_len[:rows].cpu().numpy() == w_len).all()
    assert bool((hyp[:rows, Lm:] == -9).all()) and bool((hyp[rows] == -9).all()) and bool((trg[rows] == -9).all())
    assert bool((trg_y[rows] == -9).all()) and int(hyp_len[rows]) == -9
    assert w_len.tolist() == [0, 4, 4, 2, 1, 1]
    # allocated by the wrapper: the same rows
    a, b, h, n = ops.scst_assemble(torch.from_numpy(log).to(dev), sos, eos, pad, T=T)
    assert (a.cpu().numpy() == w_trg).all() and (b.cpu().numpy() == w_trg_y).all() and (h.cpu().numpy() == w_hyp).all()
    assert (n.cpu().numpy() == w_len).all()


@pytest.mark.parametrize("S", [2, 4])
@pytest.mark.parametrize("mode", ["mean", "given"])
def test_advantage_is_numpy_double(dev, S, mode):
    """D = 3: r - b bit-equal to numpy float64, the row weights its float32 rounding on every target row, the two means bit-equal."""
    from mtn_amd import ops
    D, T = 3, 5
    rng = np.random.RandomState(7 + S)
    reward = rng.rand(D, S) * 3.0
    reward[1] = reward[1, 0]                                                             # a dialogue of equal rewards
    baseline = rng.rand(D) if mode == "given" else None
    want = sr.advantage(reward, T, baseline)
    roww = torch.full((D * S + 1, T), NAN, device=dev)
    r_dev = torch.from_numpy(reward).to(dev)
    b_dev = None if baseline is None else torch.from_numpy(baseline).to(dev)
    _, means, adv = ops.scst_advantage(r_dev, T, baseline=b_dev, roww=roww, adv=True)
    torch.cuda.synchronize()
    assert _same_bits(adv.cpu(), torch.from_numpy(want["adv"]))
    assert _same_bits(roww[:D * S].cpu(), torch.from_numpy(want["roww"])) and _all_nan(roww[D * S])
    assert _same_bits(means.cpu(), torch.tensor([want["mean_reward"], want["mean_baseline"]], dtype=torch.float64))
    if mode == "mean" and S == 2:
        assert bool((roww[S:2 * S] == 0).all())                                          # equal rewards, exact sums: no advantage
    again = torch.full_like(roww, NAN)
    ops.scst_advantage(r_dev, T, baseline=b_dev, roww=again)
    torch.cuda.synchronize()
    assert _same_bits(again.cpu(), roww.cpu())
