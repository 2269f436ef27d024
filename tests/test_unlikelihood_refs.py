"""tests/unlikelihood_refs.py checked without a GPU: the closed-form gradient of the header against float64 autograd of the clamped
definition, the conditions on the inputs that give the float32 bounds their meaning, and the float32 constants the GPU bounds are 4x of."""
import pytest
import torch

from tests import row_refs as rr
from tests import unlikelihood_refs as ur

CASES = ur.ul_cases()
IDS = [ur.ul_case_id(c) for c in CASES]


@pytest.fixture(scope="module")
def refs():
    out = []
    for i, c in enumerate(CASES):
        z, targets = ur.ul_inputs(c, ur.UL_SEED + i)
        out.append((z, targets, ur.composed_ul(z, targets, c)))
    return out


@pytest.mark.parametrize("idx", range(len(CASES)), ids=IDS)
def test_closed_form_gradient_is_autograd_of_the_definition(refs, idx):
    """float64 on both sides: loss and gradient agree to rounding, clamped candidates included."""
    c = CASES[idx]
    z, targets, ref = refs[idx]
    lse, rowloss, rowul, dz = ur.closed_form(z, targets, c, dtype=torch.float64)
    assert float((rowul - ref["rowul"]).abs().max()) <= 1e-12 * max(1.0, float(ref["rowul"].abs().max()))
    assert float((rowloss - ref["rowloss"]).abs().max()) <= 1e-12 * max(1.0, float(ref["rowloss"].abs().max()))
    assert float((dz - ref["dlogits"]).abs().max()) <= 1e-12 * float(ref["dlogits"].abs().max())
    if c.clamp:                                              # the clamped candidate carries no gradient of its own: only -p_j R is left
        row, col = ur.clamped_candidate(c, targets)
        extra = ref["dlogits"][row] - ref["hard"]["dlogits"][row]
        M = ur.candidate_mask(c, targets)[row]
        p = ref["softmax"][row]
        others = M.clone()
        others[col] = False
        R = float((p[others] / (1 - p[others])).sum())
        g = rr.GLOSS * float(ur.seg_scale(c)[row]) * c.ul_alpha
        assert abs(float(extra[col]) + g * float(p[col]) * R) <= 1e-15


def test_the_cases_cover_what_they_are_meant_to(refs):
    Vs, Ts, ns, alphas, sms, ldz, ldd = set(), set(), set(), set(), set(), set(), set()
    seen = dict(repeat=False, own=False, inside=False, tail=False, allpad=False, quirk=False, col0=False, colV1=False, col256=False,
                clamp=False, late_seg=False, empty_after_exclusion=False)
    for c, (z, targets, ref) in zip(CASES, refs):
        Vs.add(c.V); alphas.add(c.ul_alpha); sms.add(c.smoothing); ldz.add(c.ldz_pad); ldd.add(c.ldd_pad)
        M = ur.candidate_mask(c, targets)
        seen["col0"] |= bool(M[:, 0].any())
        seen["colV1"] |= bool(M[:, c.V - 1].any())
        seen["col256"] |= c.V == 260 and bool(M[:, 256:].any())
        seen["clamp"] |= c.clamp
        seen["quirk"] |= c.pads == "quirk" and any(T > 0 and int(t[0]) == c.pad and int((t == c.pad).sum()) == 1
                                                    for (n, T), t in zip(c.layout, targets))
        for s, ((n, T), t) in enumerate(zip(c.layout, targets)):
            if T == 0:
                continue
            Ts.add(T); ns.add(n)
            seen["late_seg"] |= s > 0 and c.layout[s - 1][1] == 0
            for b in range(n):
                y = t[b * T:(b + 1) * T].tolist()
                seen["allpad"] |= T > 1 and all(v == c.pad for v in y)
                seen["tail"] |= y[-1] == c.pad and y[0] != c.pad
                seen["inside"] |= any(y[i] == c.pad and y[i + 1] != c.pad and y[i - 1] != c.pad for i in range(1, T - 1))
                for i in range(1, T):
                    pre = [v for v in y[:i] if v != c.pad]
                    seen["repeat"] |= y[i] != c.pad and len(set(pre) - {y[i]}) < len([v for v in pre if v != y[i]])
                    seen["own"] |= y[i] != c.pad and y[i] in pre
                    seen["empty_after_exclusion"] |= y[i] != c.pad and y[i] in pre and not (set(pre) - {y[i]})
    assert Vs == {8, 260, 3000} and Ts == {1, 5, 70} and ns == {1, 3}
    assert alphas == {0.5, 2.0} and sms == {0.0, 0.1} and ldz == {0, 12} and ldd == {0, 12}
    missing = [k for k, v in seen.items() if not v and k != "empty_after_exclusion"]
    assert not missing, missing


@pytest.mark.parametrize("idx", range(len(CASES)), ids=IDS)
def test_input_conditions(refs, idx):
    """Every unclamped candidate has p_c <= 0.9 (1 - p_c is conditioned by at most 10); the candidate meant to be clamped has
    1 - p_c <= 1e-9 in float64.  The band between is not tested (include/mtn_hip.h says so)."""
    c = CASES[idx]
    z, targets, ref = refs[idx]
    M = ur.candidate_mask(c, targets)
    p = ref["softmax"]
    u = -torch.expm1(torch.log_softmax(z.double(), dim=1))      # 1 - p without the cancellation
    if c.clamp:
        row, col = ur.clamped_candidate(c, targets)
        assert bool(M[row, col]) and float(u[row, col]) <= 1e-9
        M = M.clone()
        M[row, col] = False
    if bool(M.any()):
        assert float(p[M].max()) <= 0.9


def test_float32_constants_are_no_smaller_than_measured(refs):
    worst = [0.0] * 4
    for c, (z, targets, ref) in zip(CASES, refs):
        e = ur.ul_errors(*ur.closed_form_f32(z, targets, c), ref)
        worst = [max(a, b) for a, b in zip(worst, e)]
    print("measured: lse %.3e  rowloss %.3e  rowul %.3e  dlogits %.3e" % tuple(worst))
    have = (ur.CPU_F32_UL_LSE, ur.CPU_F32_UL_ROWLOSS, ur.CPU_F32_UL_ROWUL, ur.CPU_F32_UL_DLOGITS)
    for got, const in zip(worst, have):
        assert got <= const
        assert const <= 4 * max(got, 1e-8)                  # nor so much larger that the bound means nothing


def test_alpha_zero_and_seq_len_zero_are_the_plain_loss(refs):
    c = CASES[7]
    z, targets, _ = refs[7]
    ref = ur.composed_ul(z, targets, c, ul_alpha=0.0)
    assert torch.equal(ref["rowloss"], ref["hard"]["rowloss"]) and torch.equal(ref["dlogits"], ref["hard"]["dlogits"])
    assert not bool(ref["rowul"].any())
    full = ur.composed_ul(z, targets, c)
    n0 = ur.seg_rows(c)[0]                                  # segment 0 of this case has seq_len 0
    assert torch.equal(full["rowloss"][:n0], full["hard"]["rowloss"][:n0]) and not bool(full["rowul"][:n0].any())
    assert bool(full["rowul"][n0:].any())
