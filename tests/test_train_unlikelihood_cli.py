"""train.py's --unlikelihood-alpha at the command line (defaults, validation, the conflict messages) and the composed PyTorch path of
SimpleLossCompute.loss(unlikelihood=...) — the one CPU tensors and un-flattened models take — against the float64 definition of
tests/unlikelihood_refs.py: loss and input gradient.  No GPU needed."""
import pytest
import torch

from mtn_amd import train
from mtn_amd.data_utils import LabelSmoothing, SimpleLossCompute
from tests import unlikelihood_refs as ur

CORPUS = ["--corpus-videos", "4"]


def test_the_flag_parses_with_its_default():
    assert train.parse([]).unlikelihood_alpha == 0.0
    assert train.parse(["--unlikelihood-alpha", "1"]).unlikelihood_alpha == 1.0          # the fixed synthetic batch takes it too
    a = train.parse(CORPUS + ["--unlikelihood-alpha", "0.25", "--ema-decay", "0.99", "--eager"])
    assert a.unlikelihood_alpha == 0.25 and a.ema_decay == 0.99 and a.eager
    assert train.unlikelihood_flag_error(a) is None


@pytest.mark.parametrize("value", ["-0.5", "nan", "inf", "-inf"])
def test_a_bad_alpha_is_refused_with_a_message(value, capsys):
    with pytest.raises(SystemExit) as e:
        train.parse(CORPUS + ["--unlikelihood-alpha=" + value])
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "--unlikelihood-alpha must be finite and >= 0" in err


def test_conflicts_are_named(capsys, monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit):
        train.parse(CORPUS + ["--unlikelihood-alpha", "1", "--distill-model", "t/a_1", "--distill-conf", "t/a.conf"])
    err = capsys.readouterr().err
    assert "--unlikelihood-alpha" in err and "--distill-model" in err
    with pytest.raises(SystemExit):
        train.parse(CORPUS + ["--unlikelihood-alpha", "1", "--scst-samples", "2"])
    err = capsys.readouterr().err
    assert "--unlikelihood-alpha" in err and "--scst-samples" in err
    # at 0 the flag is off: nothing to refuse
    assert train.parse(CORPUS + ["--unlikelihood-alpha", "0", "--scst-samples", "2"]).scst_samples == 2


# ------------------------------------------------------------------------------------------ the composed path
V, PAD, B, T, D = 24, 1, 3, 7, 16


class _Gen(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.proj = torch.nn.Linear(D, V).double()

    def forward(self, x):
        return torch.log_softmax(self.proj(x), dim=-1)


def _setup():
    g = torch.Generator().manual_seed(11)
    gen = _Gen()
    with torch.no_grad():
        gen.proj.weight.copy_(torch.randn(V, D, generator=g, dtype=torch.float64))
        gen.proj.bias.copy_(torch.randn(V, generator=g, dtype=torch.float64))
    x = torch.randn(B, T, D, generator=g, dtype=torch.float64)
    y = torch.randint(2, 8, (B, T), generator=g)              # six tokens over seven positions: repeats in every sequence
    y[0, 5:] = PAD                                            # a tail of <pad>
    y[1, 3] = PAD                                             # a <pad> inside
    y[2, 4] = y[2, 1]                                         # the row's own target in its prefix
    return gen, x, y, (y != PAD).sum()


def _reference(gen, x, y, norm, alpha):
    x = x.clone().requires_grad_()
    logp = gen(x)
    plain = LabelSmoothing(V, PAD, 0.1)(logp.reshape(-1, V), y.reshape(-1)) / norm.double()
    ul = ur.ul_rows_of_logp(logp, y, PAD)
    total = plain + alpha * ul.sum() / norm.double()
    (gx,) = torch.autograd.grad(total, x)
    return float(total.detach()), gx, float(ul.sum().detach()), float(plain.detach())


@pytest.mark.parametrize("alpha", [0.5, 2.0])
def test_composed_loss_and_gradient_are_the_definitions(alpha):
    gen, x, y, norm = _setup()
    want, want_gx, want_ul, plain = _reference(gen, x, y, norm, alpha)
    lc = SimpleLossCompute(gen, None, LabelSmoothing(V, PAD, 0.1), opt=None, sync=False)
    xg = x.clone().requires_grad_()
    loss = lc.loss(xg, y, norm, unlikelihood=alpha)
    (gx,) = torch.autograd.grad(loss, xg)
    assert want_ul > 0.1 and want > plain
    assert abs(float(loss.detach()) - want) <= 1e-12 * abs(want)
    assert abs(float(lc.last_ul_sum) - want_ul) <= 1e-12 * want_ul
    assert float((gx - want_gx).abs().max()) <= 1e-12 * float(want_gx.abs().max())


def test_a_clamped_candidate_has_no_gradient_of_its_own():
    """One candidate with probability 1 - 1e-15: torch.clamp's gradient is 0 there, and the loss holds -log(1e-5f) for it."""
    gen, x, y, norm = _setup()
    with torch.no_grad():
        gen.proj.weight.zero_()
        gen.proj.bias.zero_()
        gen.proj.bias[int(y[2, 0])] = 40.0
    want, want_gx, want_ul, _ = _reference(gen, x, y, norm, 1.0)
    lc = SimpleLossCompute(gen, None, LabelSmoothing(V, PAD, 0.1), opt=None, sync=False)
    loss = lc.loss(x, y, norm, unlikelihood=1.0)
    assert abs(float(loss.detach()) - want) <= 1e-12 * abs(want)
    assert want_ul >= 11.5                                              # -log(1e-5) = 11.51 at least once


def test_alpha_zero_is_the_plain_loss_exactly():
    gen, x, y, norm = _setup()
    lc = SimpleLossCompute(gen, None, LabelSmoothing(V, PAD, 0.1), opt=None, sync=False)
    plain = lc.loss(x, y, norm)
    zero = lc.loss(x, y, norm, unlikelihood=0.0)
    assert torch.equal(plain, zero) and lc.last_ul_sum is None
    assert float(lc.loss(x, y, norm, unlikelihood=1.0)) > float(plain) and lc.last_ul_sum is not None


def test_argument_checks_name_the_conflict():
    gen, x, y, norm = _setup()
    lc = SimpleLossCompute(gen, None, LabelSmoothing(V, PAD, 0.1), opt=None, sync=False)
    q = torch.zeros(B * T, V, dtype=torch.float64)
    with pytest.raises(ValueError, match="teacher"):
        lc.loss(x, y, norm, teacher_logp=q, alpha=0.5, unlikelihood=1.0)
    with pytest.raises(ValueError, match="row weights"):
        lc.loss(x, y, norm, row_weights=torch.ones(B * T), unlikelihood=1.0)
    with pytest.raises(ValueError, match=r"\(B, T\)"):
        lc.loss(x.reshape(B * T, D), y.reshape(-1), norm, unlikelihood=1.0)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="finite"):
            lc.loss(x, y, norm, unlikelihood=bad)
