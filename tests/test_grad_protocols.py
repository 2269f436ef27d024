"""The two gradient protocols of the training path (mtn_amd.ops), on CPU tensors and without the HIP library:
HandOff (a consumer writes the producer's masked compute-dtype dy; valid only for the untouched dx) and GradMeet (the gradients
of a tensor with several consumers meet in one buffer and return to autograd once)."""
import torch

from mtn_amd import ops


def _offered():
    h = ops.HandOff(0.1, 7 * 4 + 1, None, torch.bfloat16)
    dx = torch.randn(3, 5, 8)
    dyl = h.offer(dx, torch.bfloat16)
    assert dyl.dtype == torch.bfloat16 and dyl.shape == dx.shape and (h.p, h.salt, h.seed, h.lp) == (0.1, 29, None, torch.bfloat16)
    return h, dx, dyl


def test_handoff_claim_returns_the_offer_for_the_untouched_dx():
    h, dx, dyl = _offered()
    assert h.claim(dx) is dyl


def test_handoff_claim_refuses_a_dx_that_was_added_to():
    h, dx, _ = _offered()
    dx.add_(1)
    assert h.claim(dx) is None


def test_handoff_claim_refuses_a_clone():
    h, dx, _ = _offered()
    assert h.claim(dx.clone()) is None


def test_handoff_claim_refuses_a_view_of_another_shape():
    h, dx, _ = _offered()
    v = dx.view(15, 8)
    assert v.data_ptr() == dx.data_ptr() and v._version == dx._version      # only the shape tells them apart
    assert h.claim(v) is None


def test_handoff_claim_clears_whatever_it_answers():
    h, dx, dyl = _offered()
    assert h.claim(dx) is dyl
    assert h.claim(dx) is None
    h, dx, _ = _offered()
    assert h.claim(dx.clone()) is None
    assert h.claim(dx) is None                   # a refused claim ends the offer too


def test_handoff_withdraw():
    h, dx, dyl = _offered()
    h.withdraw(dx.data_ptr() + 4)                # another tensor: the offer stands
    assert h.dyl is dyl
    h.withdraw(dx.data_ptr())
    assert h.claim(dx) is None


def test_handoff_claim_without_an_offer():
    assert ops.HandOff(0.0, 1, None, torch.float32).claim(torch.zeros(2)) is None


def test_handoff_of_a_sublayer_config_is_its_output_dropout_site():
    seed = torch.zeros(1, dtype=torch.int64)
    for cfg in (ops.MhaConfig(heads=4, p_attn=0.3, p_out=0.2, salt=5, seed=seed, lp_dtype=torch.float32),
                ops.FfnConfig(p_hidden=0.3, p_out=0.2, salt=5, seed=seed, lp_dtype=torch.float32)):
        h = ops.HandOff.of(cfg)
        assert (h.p, h.salt, h.seed, h.lp) == (0.2, 21, seed, torch.float32)
        d = h.drop()
        assert (d.p, d.salt, d.seed) == (torch.tensor(0.2).item(), 21, seed.data_ptr())


def _settle(g, dx):
    later = []
    ret = g.settle(dx, later)
    for buf, d in later:
        buf.add_(d)
    return ret


def test_grad_meet_three_inputs_settle_in_order():
    t = torch.zeros(4, 6, requires_grad=True)
    assert ops.GradMeet.join(t) is None                          # nobody opened a meeting point: plain autograd
    g = ops.GradMeet.join(t, create=True)
    assert ops.GradMeet.join(t) is g and ops.GradMeet.join(t) is g and t._mtn_gacc is g and g.remaining == 3
    # values at which fp32 addition is not associative (the spacing at 1e8 is 8): the order of additions shows in the bits
    dxs = [torch.full((4, 6), v) for v in (1e8, 5.0, 5.0)]
    want = (dxs[0].clone() + dxs[1]) + dxs[2]                    # 100000008 + 5 -> 100000016
    assert not torch.equal(want, dxs[0] + (dxs[1] + dxs[2]))     # 100000000 + 10 -> 100000008
    first = dxs[0].data_ptr()
    assert _settle(g, dxs[0]) is None
    assert _settle(g, dxs[1]) is None
    out = _settle(g, dxs[2])
    assert out is not None and out.data_ptr() == first and torch.equal(out, want)
    assert g.buf is None and g.remaining == 0                    # ready for the next backward pass


def test_grad_meet_lone_joiner_gets_its_own_dx_back():
    t = torch.zeros(2, 3)
    g = ops.GradMeet.join(t, create=True)
    dx, later = torch.randn(2, 3), []
    assert g.settle(dx, later) is dx and later == [] and g.buf is None


def test_grad_meet_memory_role_writes_then_accumulates():
    t = torch.zeros(2, 5, 3)
    g = ops.GradMeet.join(t, create=True)
    ops.GradMeet.join(t)
    buf, accumulate, last = g.buffer((2, 5, 3), torch.device("cpu"))
    assert accumulate == 0 and not last and buf.shape == (2, 5, 3) and buf.dtype == torch.float32
    buf2, accumulate, last = g.buffer((2, 5, 3), torch.device("cpu"))
    assert buf2 is buf and accumulate == 1 and last and g.buf is None


def test_grad_meet_memory_role_accumulates_into_the_first_writers_dx():
    t = torch.zeros(2, 3)
    g = ops.GradMeet.join(t, create=True)
    ops.GradMeet.join(t)
    dx, later = torch.ones(2, 3), []
    assert g.settle(dx, later) is None and later == []
    buf, accumulate, last = g.buffer((2, 3), torch.device("cpu"))
    assert buf is dx and accumulate == 1 and last


def test_grad_meet_seed_takes_a_leaf_gradient_only_when_it_can_stand_for_the_first_writer():
    t = torch.zeros(4, 6)
    g = ops.GradMeet.join(t, create=True)
    grad = torch.randn(4, 6)
    assert not g.seed(grad.double(), t.shape) and not g.seed(torch.randn(6, 4).t(), t.shape) and not g.seed(grad[:2], t.shape) and g.buf is None
    assert g.seed(grad, t.shape) and g.buf is grad
    assert not g.seed(torch.randn(4, 6), t.shape) and g.buf is grad          # taken already
    buf, accumulate, last = g.buffer((4, 6), torch.device("cpu"))
    assert buf is grad and accumulate == 1 and last
    assert not g.seed(grad, t.shape)                                           # nobody is waiting any more
