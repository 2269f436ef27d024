"""train.py's --clip-grad-norm at the command line, in the form of tests/test_train_unlikelihood_cli.py: the default, what parses, every
line clip_flag_error can return, and the epoch line's wording.  No GPU needed."""
import math

import pytest

from mtn_amd import train

CORPUS = ["--corpus-videos", "4"]


@pytest.fixture(autouse=True)
def _one_rank(monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("MTN_DP_SHARDED", raising=False)


def test_the_flag_parses_with_its_default():
    assert train.parse([]).clip_grad_norm == 0.0
    assert train.parse(["--clip-grad-norm", "1"]).clip_grad_norm == 1.0                  # the fixed synthetic batch takes it too
    assert train.parse(["--clip-grad-norm", "inf"]).clip_grad_norm == math.inf           # measure, never clip
    a = train.parse(CORPUS + ["--clip-grad-norm", "0.25", "--ema-decay", "0.99", "--eager", "--unlikelihood-alpha", "0.5", "--resume", "x/m_1"])
    assert a.clip_grad_norm == 0.25 and a.ema_decay == 0.99 and a.eager and a.unlikelihood_alpha == 0.5
    assert train.clip_flag_error(a) is None
    assert train.parse(CORPUS + ["--clip-grad-norm", "2", "--scst-samples", "2"]).scst_samples == 2
    assert train.parse(CORPUS + ["--clip-grad-norm", "2", "--distill-model", "t/a_1", "--distill-conf", "t/a.conf"]).distill_model == ["t/a_1"]


@pytest.mark.parametrize("value", ["-0.5", "nan", "-inf"])
def test_a_bad_norm_is_refused_with_a_message(value, capsys):
    with pytest.raises(SystemExit) as e:
        train.parse(CORPUS + ["--clip-grad-norm=" + value])
    assert e.value.code == 2
    assert "--clip-grad-norm must be 0 (off) or > 0" in capsys.readouterr().err


def test_the_sharded_optimiser_is_named(monkeypatch, capsys):
    a = train.parse(["--clip-grad-norm", "1"])
    assert train.clip_flag_error(a, world=2) is None                                     # several ranks: the all-reduce scheme
    monkeypatch.setenv("MTN_DP_SHARDED", "0")
    assert train.clip_flag_error(a, world=2) is None
    monkeypatch.setenv("MTN_DP_SHARDED", "1")
    assert train.clip_flag_error(a, world=1) is None                                     # one rank: nothing is sharded
    err = train.clip_flag_error(a, world=2)
    assert "--clip-grad-norm" in err and "sharded" in err and "MTN_DP_SHARDED" in err
    monkeypatch.setenv("WORLD_SIZE", "2")                                                # ... and what the launcher says counts at parse time
    with pytest.raises(SystemExit):
        train.parse(["--clip-grad-norm", "1"])
    assert "sharded" in capsys.readouterr().err
    a.clip_grad_norm = 0.0                                                               # at 0 the flag is off: nothing to refuse
    assert train.clip_flag_error(a, world=2) is None


class _Adam:
    def __init__(self, st):
        self.st, self.resets = st, 0

    def clip_stats(self, reset=False):
        self.resets += bool(reset)
        return self.st


def test_the_epoch_line_and_the_non_finite_exit(capsys):
    adam = _Adam(dict(mean=1.5, max=4.25, steps=10, clipped=3, nonfinite=0))
    train.clip_epoch_report(adam, 1, rank=0)
    assert capsys.readouterr().out.strip() == "epoch 2 gradient norm: mean 1.500000 max 4.250000 clipped 3 of 10 steps"
    train.clip_epoch_report(adam, 1, rank=1)
    assert capsys.readouterr().out == "" and adam.resets == 2                            # every rank reads and resets, rank 0 prints
    bad = _Adam(dict(mean=1.5, max=4.25, steps=10, clipped=3, nonfinite=2))
    with pytest.raises(SystemExit) as e:
        train.clip_epoch_report(bad, 4, rank=1)
    assert "epoch 5" in str(e.value.code) and "2 of 10 steps" in str(e.value.code) and "not finite" in str(e.value.code)
