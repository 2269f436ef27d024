"""train.py's --ema-decay and average.py's --weights at the command line (no GPU needed)."""
import pytest

from mtn_amd import average, train


def test_ema_decay_defaults_to_off_and_parses():
    assert train.parse([]).ema_decay == 0.0
    assert train.parse(["--ema-decay", "0"]).ema_decay == 0.0                  # 0 is accepted as off
    assert train.parse(["--ema-decay", "0.999", "--batch-size", "4"]).ema_decay == 0.999
    assert train.ema_flag_error(train.parse(["--ema-decay", "0.5"])) is None


@pytest.mark.parametrize("value", ["1", "-0.1", "nan", "1.5", "inf"])
def test_a_bad_ema_decay_is_a_usage_error(value, capsys):
    with pytest.raises(SystemExit) as e:
        train.parse(["--ema-decay", value])
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "--ema-decay" in err and len(err.strip().splitlines()[-1]) < 200


def test_average_weights_default_to_uniform():
    a = average.parse(["--inputs", "a", "b", "c", "--output", "o"])
    assert a.weights == [1.0, 1.0, 1.0] and a.inputs == ["a", "b", "c"] and a.output == "o"
    assert average.parse(["--inputs", "a", "b", "c", "--output", "o", "--weights", "1", "1", "2"]).weights == [1.0, 1.0, 2.0]
    assert average.parse(["--inputs", "a", "b", "--output", "o", "--weights", "0", "2"]).weights == [0.0, 2.0]


@pytest.mark.parametrize("weights,word", [(["1", "-1"], "negative"), (["1", "nan"], "not finite"), (["inf", "1"], "not finite"),
                                          (["0", "0"], "all zero"), (["1"], "one weight per"), (["1", "1", "1"], "one weight per")])
def test_bad_average_weights_are_refused_naming_the_cause(weights, word, capsys):
    with pytest.raises(SystemExit) as e:
        average.parse(["--inputs", "a", "b", "--output", "o", "--weights"] + weights)
    assert e.value.code == 2
    assert word in capsys.readouterr().err
