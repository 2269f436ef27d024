"""The float64 reference of the distillation loss head (tests/distill_refs.py) checked without a GPU: the kernel's closed form against
the composed reference, alpha = 0 against row_refs.composed_loss, the header's backward formula against autograd, the case list against
the lists it is meant to cover, and the recorded float32 yardsticks the GPU bounds are 4x of."""
import pytest
import torch

from tests import distill_refs as dr
from tests import row_refs as rr

CASES = dr.dist_cases()
IDS = [dr.dist_case_id(c) for c in CASES]


def test_case_list_covers_what_it_should():
    cs = CASES
    assert {c.V for c in cs} == set(dr.VS)
    assert {(c.segs, c.teach) for c in cs} == set(dr.LAYOUTS)
    for V in dr.VS:
        assert {c.pads for c in cs if c.V == V} == set(rr.PAD_KINDS)
    for name in ("ldz_pad", "ldq_pad", "ldd_pad"):
        assert {getattr(c, name) for c in cs} == {0, 12, 60}
    assert {c.T for c in cs} == {0.5, 1.0, 2.0} and {c.alpha for c in cs} == {0.0, 0.3, 1.0} and {c.smoothing for c in cs} == {0.0, 0.1}
    assert {c.form for c in cs} == set(dr.FORMS)
    for T in dr.TEMPS:                                           # every temperature meets multi-sweep and single-sweep rows, every alpha > 0
        assert {c.V > 256 for c in cs if c.T == T} == {False, True}
        assert {c.alpha for c in cs if c.T == T} >= {0.3, 1.0}
    for form in dr.FORMS:
        assert {c.V > 256 for c in cs if c.form == form and c.alpha > 0} == {False, True}
    for i, c in enumerate(cs):                                   # -inf never fills a teacher row
        for q in dr.dist_inputs(c, dr.DIST_SEED + i)[2]:
            assert q is None or bool(torch.isfinite(q).any(1).all())


@pytest.mark.parametrize("idx", range(len(CASES)), ids=IDS)
def test_closed_form_matches_composed_reference(idx):
    """The max-shifted closed form in float64 == F.kl_div on log_softmax(z / T), softmax(q / T) to 1e-11 of the largest kd, rows of <pad>
    targets and segments without a teacher hold kd = 0, -inf teacher columns make no NaN, and rowloss sums to the total."""
    c = CASES[idx]
    z, targets, teachers = dr.dist_inputs(c, dr.DIST_SEED + idx)
    ref = dr.composed_distill(z, targets, teachers, c)
    mask = dr.kd_rows_mask(c, targets)
    assert bool(torch.isfinite(ref["rowloss"]).all()) and bool(torch.isfinite(ref["dlogits"]).all()) and bool(torch.isfinite(ref["rowkd"]).all())
    assert bool((ref["rowkd"][~mask] == 0).all()) and bool((ref["rowkd"] >= -1e-12).all())
    assert abs(float(ref["rowloss"].sum()) - ref["total"]) <= 1e-12 * max(1.0, abs(ref["total"]))
    if not mask.any():
        return
    T = c.T
    z64 = z.double()
    q64 = torch.cat([q.double() if q is not None else torch.zeros(n, c.V, dtype=torch.float64) for q, n in zip(teachers, c.segs)])
    da = z64 / T - (z64 / T).max(1, keepdim=True).values
    db = q64 / T - (q64 / T).max(1, keepdim=True).values
    e = db.exp()
    term = torch.where(torch.isinf(db), torch.zeros((), dtype=torch.float64), e * (db - da))
    kd = term.sum(1) / e.sum(1) - e.sum(1).log() + da.exp().sum(1).log()
    assert float((kd - ref["rowkd"])[mask].abs().max()) <= 1e-11 * max(1.0, float(ref["rowkd"].max()))


@pytest.mark.parametrize("idx", [i for i, c in enumerate(CASES) if c.alpha == 0], ids=[IDS[i] for i, c in enumerate(CASES) if c.alpha == 0])
def test_alpha_zero_is_the_plain_loss_head_reference(idx):
    c = CASES[idx]
    z, targets, teachers = dr.dist_inputs(c, dr.DIST_SEED + idx)
    ref, plain = dr.composed_distill(z, targets, teachers, c), rr.composed_loss(z, targets, dr.loss_case(c))
    for k in ("lse", "rowloss", "dlogits"):
        assert torch.equal(ref[k], plain[k])
    assert ref["total"] == plain["total"] and bool((ref["rowkd"] == 0).all())
    f32, plain32 = dr.closed_form_f32(z, targets, teachers, c), rr.closed_form_f32(z, targets, dr.loss_case(c))
    assert torch.equal(f32[0], plain32[0]) and torch.equal(f32[1], plain32[1]) and torch.equal(f32[3], plain32[2])


@pytest.mark.parametrize("idx", range(len(CASES)), ids=IDS)
def test_backward_formula_matches_autograd(idx):
    """dz_j = g scale [(1 - alpha)(softmax_j(z) sum(td) - td_j) + alpha T (pS_j - pT_j)] written out in float64 == the autograd gradient of
    the composed total, to 1e-12 of its largest element."""
    c = CASES[idx]
    z, targets, teachers = dr.dist_inputs(c, dr.DIST_SEED + idx)
    ref = dr.composed_distill(z, targets, teachers, c)
    hard = ref["hard"]
    z64 = z.double()
    td = torch.cat([rr.smoothed_targets(t, c.V, c.pad, c.smoothing) for t in targets])
    scale = dr.seg_scale(c)
    dist, mask = dr.seg_distilled(c), dr.kd_rows_mask(c, targets)
    w = torch.where(dist, torch.tensor(1.0 - c.alpha, dtype=torch.float64), torch.ones((), dtype=torch.float64))
    d = w.unsqueeze(1) * (hard["softmax"] * hard["sum_td"].unsqueeze(1) - td)
    if mask.any():
        q64 = torch.cat([q.double() if q is not None else torch.zeros(n, c.V, dtype=torch.float64) for q, n in zip(teachers, c.segs)])
        soft = c.alpha * c.T * (torch.softmax(z64 / c.T, 1) - torch.softmax(q64 / c.T, 1))
        d = d + torch.where(mask.unsqueeze(1), soft, torch.zeros((), dtype=torch.float64))
    d = rr.GLOSS * scale.unsqueeze(1) * d
    assert float((d - ref["dlogits"]).abs().max()) <= 1e-12 * float(ref["dlogits"].abs().max())
    assert bool((ref["dlogits"][ref["zero"]] == 0).all())


def measure():
    worst = [0.0, 0.0, 0.0, 0.0]
    for i, c in enumerate(CASES):
        z, targets, teachers = dr.dist_inputs(c, dr.DIST_SEED + i)
        e = dr.dist_errors(*dr.closed_form_f32(z, targets, teachers, c), dr.composed_distill(z, targets, teachers, c))
        worst = [max(a, b) for a, b in zip(worst, e)]
    return worst


def test_float32_yardsticks_are_what_the_cpu_measures():
    """The constants the GPU bounds are 4x of: the float32 CPU evaluation of the closed form against float64, re-measured."""
    worst = measure()
    print("lse %.3e  rowloss %.3e  rowkd %.3e  dlogits %.3e" % tuple(worst))
    rec = (dr.CPU_F32_DISTILL_LSE, dr.CPU_F32_DISTILL_ROWLOSS, dr.CPU_F32_DISTILL_ROWKD, dr.CPU_F32_DISTILL_DLOGITS)
    for got, r in zip(worst, rec):
        assert r / 2 <= got <= r * 2, (worst, rec)


def test_composed_fallback_of_simple_loss_compute_matches_the_reference():
    """SimpleLossCompute.loss(..., teacher_logp=...) on CPU tensors (the composed PyTorch form) == the composed float64 reference on the
    generator's logits, value and gradient; alpha = 0 is the plain loss."""
    from mtn_amd.data_utils import LabelSmoothing, SimpleLossCompute
    from mtn_amd.mtn import Generator
    torch.manual_seed(3)
    V, d, n = 104, 16, 9
    gen = Generator(d, V).double()
    x = torch.randn(n, d, dtype=torch.float64, requires_grad=True)
    y = torch.randint(2, V, (n,))
    y[4] = y[8] = 1
    q = torch.randn(n, V) * 2 + 5
    norm = torch.tensor(7.0)
    lc = SimpleLossCompute(gen, None, LabelSmoothing(V, 1, 0.1), opt=None, sync=False)
    c = dr.DistCase(V, (n,), (0,), 0, 0, 0, "tail", 0.1, 2.0, 0.3, "off+", 1, 1.0, 0.0)
    loss = lc.loss(x, y, norm, teacher_logp=q, alpha=c.alpha, temperature=c.T)
    (gx,) = torch.autograd.grad(loss, x)
    z = gen.proj(x).detach()
    ref = dr.composed_distill(z.float(), [y], [q], c)                       # (its inputs are float32 rows: compare at that precision)
    scale = rr.COEF[0] / rr.NORM[0]
    want = ref["total"] / scale / float(norm)
    assert abs(float(loss.detach()) - want) <= 1e-6 * abs(want)
    assert abs(float(lc.last_kd_sum) - float(ref["rowkd"].sum())) <= 1e-6 * float(ref["rowkd"].sum())
    gz = ref["dlogits"] / rr.GLOSS / scale / float(norm)                    # d loss / d logits -> d loss / d x through the projection
    assert float((gz @ gen.proj.weight.detach() - gx).abs().max()) <= 1e-6 * float(gx.abs().max())
    plain = lc.loss(x, y, norm)
    assert float(lc.loss(x, y, norm, teacher_logp=q, alpha=0.0, temperature=2.0)) == float(plain) and lc.last_kd_sum is None
    with pytest.raises(ValueError):
        lc.loss(x, y, norm, teacher_logp=q, alpha=1.5)
    with pytest.raises(ValueError):
        lc.loss(x, y, norm, teacher_logp=q, alpha=0.5, temperature=0.0)
