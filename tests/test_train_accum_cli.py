"""train.py's --accum-steps at the command line, in the form of tests/test_train_clip_cli.py: the default, what parses, every line
accum_flag_error can return.  No GPU needed."""
import pytest

from mtn_amd import train

CORPUS = ["--corpus-videos", "4"]


@pytest.fixture(autouse=True)
def _one_rank(monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("MTN_DP_SHARDED", raising=False)


def test_the_flag_parses_and_the_default_is_off():
    assert train.parse([]).accum_steps == 1
    assert train.accum_flag_error(train.parse([])) is None
    assert train.parse(["--accum-steps", "4"]).accum_steps == 4                          # the fixed synthetic batch takes it too
    a = train.parse(CORPUS + ["--accum-steps", "2", "--ema-decay", "0.99", "--eager", "--unlikelihood-alpha", "0.5", "--resume", "x/m_1",
                              "--clip-grad-norm", "1", "--cut-a", "1"])
    assert a.accum_steps == 2 and a.ema_decay == 0.99 and a.eager and a.clip_grad_norm == 1.0
    assert train.accum_flag_error(a) is None and train.accum_flag_error(a, world=2) is None
    assert train.parse(CORPUS + ["--accum-steps", "2", "--distill-model", "t/a_1", "--distill-conf", "t/a.conf"]).distill_model == ["t/a_1"]
    assert train.parse(CORPUS + ["--accum-steps", "1", "--scst-samples", "2"]).scst_samples == 2      # 1 is off: nothing to refuse


@pytest.mark.parametrize("value", ["0", "-1", "-8"])
def test_a_window_below_one_is_refused_with_a_message(value, capsys):
    with pytest.raises(SystemExit) as e:
        train.parse(CORPUS + ["--accum-steps=" + value])
    assert e.value.code == 2
    assert "--accum-steps must be an integer >= 1" in capsys.readouterr().err


@pytest.mark.parametrize("value", ["1.5", "2.0", "two", "nan", ""])
def test_a_window_that_is_no_integer_is_refused(value, capsys):
    with pytest.raises(SystemExit) as e:
        train.parse(CORPUS + ["--accum-steps=" + value])
    assert e.value.code == 2
    assert "--accum-steps" in capsys.readouterr().err


def test_the_scst_conflict_names_itself(capsys):
    with pytest.raises(SystemExit) as e:
        train.parse(CORPUS + ["--accum-steps", "2", "--scst-samples", "2"])
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "--accum-steps does not combine with --scst-samples" in err


def test_the_sharded_optimiser_is_named(monkeypatch, capsys):
    a = train.parse(["--accum-steps", "2"])
    assert train.accum_flag_error(a, world=2) is None                                    # several ranks: the all-reduce scheme
    monkeypatch.setenv("MTN_DP_SHARDED", "0")
    assert train.accum_flag_error(a, world=2) is None
    monkeypatch.setenv("MTN_DP_SHARDED", "1")
    assert train.accum_flag_error(a, world=1) is None                                    # one rank: nothing is sharded
    err = train.accum_flag_error(a, world=2)
    assert "--accum-steps" in err and "sharded" in err and "MTN_DP_SHARDED" in err
    monkeypatch.setenv("WORLD_SIZE", "2")                                                # ... and what the launcher says counts at parse time
    with pytest.raises(SystemExit):
        train.parse(["--accum-steps", "2"])
    assert "sharded" in capsys.readouterr().err
    a.accum_steps = 1                                                                    # at 1 the flag is off: nothing to refuse
    assert train.accum_flag_error(a, world=2) is None
