"""The float64 references of tests/test_row_kernels_gpu.py (tests/row_refs.py) checked without a GPU: the composed loss-head
reference against mtn_amd.data_utils.LabelSmoothing (the project's second, independent statement of the loss) on the GPU test's
own case list, the float64 Adam against torch.optim.Adam, the Noam state, and the recorded float32 yardsticks the GPU bounds are
multiples of."""
import math

import pytest
import torch

from tests import row_refs as rr

LOSS_CASES = rr.loss_cases()


def test_case_list_covers_what_the_issue_names():
    cs = LOSS_CASES
    assert {c.V for c in cs} >= {8, 104, 256, 260, 1024, 3000, 3004, 8192}
    assert {c.segs for c in cs} >= {(1,), (5,), (18, 15), (640, 100, 7), (3, 1, 1, 2)}
    assert {c.ldz_pad for c in cs} == {0, 12} and {c.ldd_pad for c in cs} == {0, 4, 60}
    assert {(c.scale, c.offset) for c in cs} >= {(1.0, 0.0), (8.0, 0.0), (1.0, 50.0), (1.0, -50.0)}
    assert 0.0 in {c.smoothing for c in cs}
    for V in (3000, 3004):
        assert {c.pads for c in cs if c.V == V} == set(rr.PAD_KINDS)
    ls = rr.lsm_cases()
    assert {(c.rows, c.V) for c in ls} == {(r, V) for r in (1, 5, 64) for V in (1, 7, 255, 256, 257, 3000, 5003)}
    for V in (7, 255, 256, 257, 3000, 5003):
        assert len({(c.ldx_pad, c.ldo_pad, c.inplace, c.offset) for c in ls if c.V == V}) == 3
    assert {c.offset for c in ls} == {0.0, 1e4, -1e4} and {c.inplace for c in ls} == {False, True}


@pytest.mark.parametrize("idx", range(len(LOSS_CASES)), ids=[rr.loss_case_id(c) for c in LOSS_CASES])
def test_composed_loss_matches_label_smoothing_module(idx):
    """composed_loss (oracle label_smoothing_kl per segment) == sum coef / norm * LabelSmoothing.forward in float64, value and
    gradient, to 1e-12 relative; the pad placement does what its name says (which rows are zeroed, which keep the quirk)."""
    from mtn_amd.data_utils import LabelSmoothing
    c = LOSS_CASES[idx]
    z, targets = rr.loss_inputs(c, rr.LOSS_SEED + idx)
    ref = rr.composed_loss(z, targets, c)
    z64 = z.double().clone().requires_grad_()
    logp = torch.log_softmax(z64, dim=1)
    crit = LabelSmoothing(c.V, c.pad, c.smoothing)
    total, base = 0.0, 0
    for s, t in enumerate(targets):
        total = total + rr.COEF[s] * crit(logp[base:base + t.numel()], t) / rr.NORM[s]
        base += t.numel()
    (grad,) = torch.autograd.grad(total, z64)
    assert abs(float(total.detach()) - ref["total"]) <= 1e-12 * abs(ref["total"])
    assert abs(float(ref["rowloss"].sum()) - ref["total"]) <= 1e-12 * abs(ref["total"])
    assert float((rr.GLOSS * grad - ref["dlogits"]).abs().max()) <= 1e-12 * float(ref["dlogits"].abs().max())
    # the placement: lone <pad> rows at local row 0 survive, every other <pad> row is zeroed
    base = 0
    for s, t in enumerate(targets):
        kind = c.pads
        if kind == "lone0_late":
            kind = "tail" if s == 0 else ("lone0" if s == min(2, len(c.segs) - 1) else "none")
        zero = ref["zero"][base:base + t.numel()]
        is_pad = t == c.pad
        if kind == "none":
            assert not is_pad.any()
        elif kind == "tail":
            assert not bool(is_pad[0]) and torch.equal(zero, is_pad) and (t.numel() == 1 or is_pad.any())
        elif kind == "lone0" or (kind == "zero_plus" and t.numel() == 1):
            assert bool(is_pad[0]) and int(is_pad.sum()) == 1 and not zero.any()
            if c.smoothing > 0:
                assert float(ref["rowloss"][base].abs()) > 0
        else:
            assert bool(is_pad[0]) and int(is_pad.sum()) == 2 and torch.equal(zero, is_pad)
        assert bool((ref["rowloss"][base:base + t.numel()][zero] == 0).all())
        base += t.numel()


def test_float32_yardsticks_are_what_the_cpu_measures():
    """The constants the GPU bounds are 4x of: the float32 CPU evaluation of the same formulas against float64, re-measured."""
    worst = [0.0, 0.0, 0.0]
    for i, c in enumerate(LOSS_CASES):
        z, targets = rr.loss_inputs(c, rr.LOSS_SEED + i)
        e = rr.loss_errors(*rr.closed_form_f32(z, targets, c), rr.composed_loss(z, targets, c))
        worst = [max(a, b) for a, b in zip(worst, e)]
    lsm = 0.0
    for i, c in enumerate(rr.lsm_cases()):
        if c.offset == 0:
            x = rr.lsm_inputs(c, rr.LSM_SEED + i)
            lsm = max(lsm, float((torch.log_softmax(x, 1).double() - torch.log_softmax(x.double(), 1)).abs().max()))
    for got, rec in zip(worst + [lsm], (rr.CPU_F32_LSE_ABS, rr.CPU_F32_ROWLOSS_REL, rr.CPU_F32_DLOGITS_REL, rr.CPU_F32_LSM_ABS)):
        assert rec / 2 <= got <= rec * 2, (worst, lsm)


@pytest.mark.parametrize("grad_scale", [1.0, 0.125])
def test_adam_step64_matches_torch_adam(grad_scale):
    p0, g0, m0, v0 = (t.double() for t in rr.adam_inputs(4100, 5))
    w = p0.clone().requires_grad_()
    opt = torch.optim.Adam([w], lr=1.0, betas=(rr.BETA1, rr.BETA2), eps=rr.ADAM_EPS)
    p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    for step in range(1, 4):
        g = rr.adam_inputs(4100, 5 + step)[1].double()
        st = rr.noam_state64(step, 128, 10, 2.0)
        opt.param_groups[0]["lr"] = st[1]
        w.grad = g * grad_scale
        opt.step()
        p, m, v = rr.adam_step64(p, g, m, v, st[1], st[2], st[3], grad_scale)
        assert float((w.detach() - p).abs().max()) <= 1e-12 * float(p.abs().max())
        state = opt.state[w]
        assert float((state["exp_avg"] - m).abs().max()) <= 1e-12 * float(m.abs().max())
        assert float((state["exp_avg_sq"] - v).abs().max()) <= 1e-12 * float(v.abs().max())
    # a nonzero starting state goes through the same recurrence: one more step from (m0, v0), against the formula written out
    st = rr.noam_state64(7, 128, 10, 2.0)
    p1, m1, v1 = rr.adam_step64(p0, g0, m0, v0, st[1], st[2], st[3])
    m_ = 0.9 * m0 + 0.1 * g0
    v_ = 0.98 * v0 + 0.02 * g0 * g0
    assert float((m1 - m_).abs().max()) <= 1e-15 and float((v1 - v_).abs().max()) <= 1e-15      # 1 - 0.9 is not 0.1 to the last bit
    assert float((p1 - (p0 - st[1] / st[2] * m_ / (v_.sqrt() / math.sqrt(st[3]) + 1e-9))).abs().max()) <= 1e-15
    assert float(p1[0]) == float(p0[0])                      # g = m = v = 0: 0 / eps


def test_noam_state64():
    from oracle.mtn_oracle import noam_rate
    assert rr.noam_state64(1, 512, 4000, 1.0) == [1.0, 512 ** -0.5 * 4000 ** -1.5, 1.0 - 0.9, 1.0 - 0.98]
    s = rr.noam_state64(4000, 512, 4000, 1.0)
    assert abs(s[1] - 512 ** -0.5 * 4000 ** -0.5) <= 1e-18 and s[1] == noam_rate(4000, 512, 4000, 1.0)
    assert rr.noam_state64(10 ** 5, 128, 10, 2.0)[2:] == [1.0, 1.0]
    assert rr.noam_state64(11, 128, 10, 2.0)[1] == 2.0 * 128 ** -0.5 * 11 ** -0.5


def test_bf16_ulp():
    x = torch.tensor([1.0, 1.99, 2.0, -3.0, 0.0476, 1e-45], dtype=torch.float64)
    want = [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -6, 2.0 ** -12, 2.0 ** -133]
    assert rr.bf16_ulp(x).tolist() == want
    b = torch.tensor([1.0, 2.0, 0.0476], dtype=torch.bfloat16)
    nxt = (b.view(torch.int16) + 1).view(torch.bfloat16)
    assert torch.equal((nxt.double() - b.double()), rr.bf16_ulp(b.double()))
