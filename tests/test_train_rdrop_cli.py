"""train.py's --rdrop-alpha at the command line (defaults, validation, each conflict message, the flag absent equal to --rdrop-alpha 0) and
the composed PyTorch path of SimpleLossCompute.loss(rdrop=...) — the one CPU tensors and un-flattened models take — against the float64
definition of tests/rdrop_refs.py: loss and input gradient.  No GPU needed."""
import pytest
import torch

from mtn_amd import train
from mtn_amd.data_utils import LabelSmoothing, SimpleLossCompute
from tests import rdrop_refs as rd

CORPUS = ["--corpus-videos", "4"]


def test_the_flag_parses_with_its_default():
    assert train.parse([]).rdrop_alpha == 0.0
    assert train.parse(["--rdrop-alpha", "1"]).rdrop_alpha == 1.0                        # the fixed synthetic batch takes it too
    a = train.parse(CORPUS + ["--rdrop-alpha", "0.25", "--ema-decay", "0.99", "--eager", "--clip-grad-norm", "1", "--accum-steps", "2"])
    assert a.rdrop_alpha == 0.25 and a.ema_decay == 0.99 and a.eager and a.clip_grad_norm == 1.0 and a.accum_steps == 2
    assert train.rdrop_flag_error(a) is None


def test_the_flag_absent_equals_alpha_zero():
    for argv in ([], CORPUS, CORPUS + ["--eager", "--unlikelihood-alpha", "1"]):
        assert vars(train.parse(argv)) == vars(train.parse(argv + ["--rdrop-alpha", "0"]))
        assert train.rdrop_flag_error(train.parse(argv)) is None


def test_the_help_text_says_what_the_batch_size_means(capsys):
    with pytest.raises(SystemExit):
        train.parse(["--help"])
    text = " ".join(capsys.readouterr().out.split())
    assert "--rdrop-alpha" in text and "2 B rows" in text and "activation memory" in text


@pytest.mark.parametrize("value", ["-0.5", "nan", "inf", "-inf"])
def test_a_bad_alpha_is_refused_with_a_message(value, capsys):
    with pytest.raises(SystemExit) as e:
        train.parse(CORPUS + ["--rdrop-alpha=" + value])
    assert e.value.code == 2
    assert "--rdrop-alpha must be finite and >= 0" in capsys.readouterr().err


@pytest.mark.parametrize("other,flags", [("--distill-model", ["--distill-model", "t/a_1", "--distill-conf", "t/a.conf"]),
                                         ("--scst-samples", ["--scst-samples", "2"]),
                                         ("--unlikelihood-alpha", ["--unlikelihood-alpha", "1"]),
                                         ("--sched-sample-prob", ["--sched-sample-prob", "0.25"])])
def test_conflicts_are_named(other, flags, capsys, monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit) as e:
        train.parse(CORPUS + ["--rdrop-alpha", "1"] + flags)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "--rdrop-alpha does not combine with " + other in err
    # at 0 the flag is off: nothing to refuse
    assert train.parse(CORPUS + ["--rdrop-alpha", "0"] + flags).rdrop_alpha == 0.0
    args = train.parse(CORPUS + flags)                         # the function itself, in the style of its siblings
    assert train.rdrop_flag_error(args) is None
    args.rdrop_alpha = 1.0
    assert other in train.rdrop_flag_error(args)


# ------------------------------------------------------------------------------------------ the composed path
V, PAD, B, T, D = 24, 1, 3, 7, 16


class _Gen(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.proj = torch.nn.Linear(D, V).double()

    def forward(self, x):
        return torch.log_softmax(self.proj(x), dim=-1)


def _setup():
    g = torch.Generator().manual_seed(13)
    gen = _Gen()
    with torch.no_grad():
        gen.proj.weight.copy_(torch.randn(V, D, generator=g, dtype=torch.float64))
        gen.proj.bias.copy_(torch.randn(V, generator=g, dtype=torch.float64))
    x = torch.randn(B, T, D, generator=g, dtype=torch.float64)
    x = torch.cat([x, x + 0.3 * torch.randn(B, T, D, generator=g, dtype=torch.float64)])      # the second pass: the first, perturbed
    y = torch.randint(2, V, (B, T), generator=g)
    y[0, 5:] = PAD                                            # a tail of <pad>
    y[1, 3] = PAD                                             # a <pad> inside
    y = torch.cat([y, y])
    return gen, x, y, (y != PAD).sum()


def _reference(gen, x, y, norm, alpha):
    x = x.clone().requires_grad_()
    logp = gen(x)
    plain = LabelSmoothing(V, PAD, 0.1)(logp.reshape(-1, V), y.reshape(-1)) / norm.double()
    rows = rd.rd_rows_of_logp(logp.reshape(-1, V), y, PAD)
    total = plain + alpha * rows.sum() / norm.double()
    (gx,) = torch.autograd.grad(total, x)
    return float(total.detach()), gx, float(rows.sum().detach()), float(plain.detach())


@pytest.mark.parametrize("alpha", [0.3, 5.0])
def test_composed_loss_and_gradient_are_the_definitions(alpha):
    gen, x, y, norm = _setup()
    want, want_gx, want_rd, plain = _reference(gen, x, y, norm, alpha)
    lc = SimpleLossCompute(gen, None, LabelSmoothing(V, PAD, 0.1), opt=None, sync=False)
    xg = x.clone().requires_grad_()
    loss = lc.loss(xg, y, norm, rdrop=alpha)
    (gx,) = torch.autograd.grad(loss, xg)
    assert want_rd > 0.1 and want > plain
    assert abs(float(loss.detach()) - want) <= 1e-12 * abs(want)
    assert abs(float(lc.last_rd_sum) - want_rd) <= 1e-12 * want_rd
    assert float((gx - want_gx).abs().max()) <= 1e-12 * float(want_gx.abs().max())


def test_alpha_zero_is_the_plain_loss_exactly():
    gen, x, y, norm = _setup()
    lc = SimpleLossCompute(gen, None, LabelSmoothing(V, PAD, 0.1), opt=None, sync=False)
    plain = lc.loss(x, y, norm)
    zero = lc.loss(x, y, norm, rdrop=0.0)
    assert torch.equal(plain, zero) and lc.last_rd_sum is None
    assert float(lc.loss(x, y, norm, rdrop=1.0).detach()) > float(plain.detach()) and lc.last_rd_sum is not None


def test_argument_checks_name_the_conflict():
    gen, x, y, norm = _setup()
    lc = SimpleLossCompute(gen, None, LabelSmoothing(V, PAD, 0.1), opt=None, sync=False)
    q = torch.zeros(2 * B * T, V, dtype=torch.float64)
    with pytest.raises(ValueError, match="teacher"):
        lc.loss(x, y, norm, teacher_logp=q, alpha=0.5, rdrop=1.0)
    with pytest.raises(ValueError, match="row weights"):
        lc.loss(x, y, norm, row_weights=torch.ones(2 * B * T), rdrop=1.0)
    with pytest.raises(ValueError, match="unlikelihood"):
        lc.loss(x, y, norm, unlikelihood=1.0, rdrop=1.0)
    with pytest.raises(ValueError, match=r"\(2 B, T\)"):
        lc.loss(x.reshape(2 * B * T, D), y.reshape(-1), norm, rdrop=1.0)
    with pytest.raises(ValueError, match=r"\(2 B, T\)"):
        lc.loss(x[:5], y[:5], norm, rdrop=1.0)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="finite"):
            lc.loss(x, y, norm, rdrop=bad)
