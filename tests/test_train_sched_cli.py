"""train.py's --sched-sample-* flags at the command line, in the form of tests/test_train_accum_cli.py: the defaults, what parses, every
line sched_flag_error can return, and the flags as a SchedConfig.  No GPU needed."""
import pytest

from mtn_amd import train

CORPUS = ["--corpus-videos", "4"]


@pytest.fixture(autouse=True)
def _one_rank(monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("MTN_DP_SHARDED", raising=False)


def test_the_flags_parse_and_the_default_is_off():
    a = train.parse([])
    assert (a.sched_sample_prob, a.sched_sample_start, a.sched_sample_ramp, a.sched_sample_pick, a.sched_sample_temperature,
            a.sched_sample_seed) == (0.0, 0, 0, "argmax", 1.0, 0)
    assert train.sched_flag_error(a) is None and train.sched_config(a) is None
    assert train.parse(["--sched-sample-prob", "0.25"]).sched_sample_prob == 0.25            # the fixed synthetic batch takes it too
    a = train.parse(CORPUS + ["--sched-sample-prob", "1", "--sched-sample-start", "100", "--sched-sample-ramp", "4000", "--sched-sample-pick",
                              "sample", "--sched-sample-temperature", "0.7", "--sched-sample-seed", "11", "--ema-decay", "0.99", "--eager",
                              "--unlikelihood-alpha", "0.5", "--resume", "x/m_1", "--clip-grad-norm", "1", "--cut-a", "1", "--accum-steps", "2"])
    assert train.sched_flag_error(a) is None and train.sched_flag_error(a, world=2) is None
    c = train.sched_config(a)
    assert (c.prob, c.start, c.ramp, c.pick, c.temperature, c.seed, c.banned) == (1.0, 100, 4000, "sample", 0.7, 11, (2,))
    # with the probability at 0 the other flags are idle: no conflict to name
    assert train.parse(CORPUS + ["--sched-sample-pick", "sample", "--scst-samples", "2"]).scst_samples == 2
    assert train.parse(CORPUS + ["--sched-sample-start", "5", "--distill-model", "t/a_1", "--distill-conf", "t/a.conf"]).distill_model == ["t/a_1"]


@pytest.mark.parametrize("flag,value,message", [
    ("--sched-sample-prob", "-0.1", "--sched-sample-prob must be 0 (off) or lie in (0, 1]"),
    ("--sched-sample-prob", "1.5", "--sched-sample-prob must be 0 (off) or lie in (0, 1]"),
    ("--sched-sample-prob", "nan", "--sched-sample-prob must be 0 (off) or lie in (0, 1]"),
    ("--sched-sample-start", "-1", "--sched-sample-start must be >= 0"),
    ("--sched-sample-ramp", "-5", "--sched-sample-ramp must be >= 0"),
    ("--sched-sample-temperature", "0", "--sched-sample-temperature must be finite and > 0"),
    ("--sched-sample-temperature", "-1", "--sched-sample-temperature must be finite and > 0"),
    ("--sched-sample-temperature", "inf", "--sched-sample-temperature must be finite and > 0"),
    ("--sched-sample-temperature", "nan", "--sched-sample-temperature must be finite and > 0"),
    ("--sched-sample-seed", "-1", "--sched-sample-seed must lie in [0, 2^62)"),
    ("--sched-sample-seed", str(1 << 62), "--sched-sample-seed must lie in [0, 2^62)"),
])
def test_a_bad_value_is_refused_with_a_message(flag, value, message, capsys):
    with pytest.raises(SystemExit) as e:
        train.parse(CORPUS + ["--sched-sample-prob", "0.5", flag + "=" + value])
    assert e.value.code == 2
    assert message in capsys.readouterr().err


@pytest.mark.parametrize("argv", [["--sched-sample-pick", "greedy"], ["--sched-sample-start", "1.5"], ["--sched-sample-ramp", "ten"],
                                  ["--sched-sample-prob", "half"], ["--sched-sample-seed", "0.5"]])
def test_what_the_parser_itself_refuses(argv, capsys):
    with pytest.raises(SystemExit) as e:
        train.parse(CORPUS + argv)
    assert e.value.code == 2
    assert argv[0] in capsys.readouterr().err


def test_the_distillation_conflict_names_itself(capsys):
    with pytest.raises(SystemExit) as e:
        train.parse(CORPUS + ["--sched-sample-prob", "0.25", "--distill-model", "t/a_1", "--distill-conf", "t/a.conf"])
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "--sched-sample-prob does not combine with --distill-model" in err and "mixed inputs" in err


def test_the_scst_conflict_names_itself(capsys):
    with pytest.raises(SystemExit) as e:
        train.parse(CORPUS + ["--sched-sample-prob", "0.25", "--scst-samples", "2"])
    assert e.value.code == 2
    assert "--sched-sample-prob does not combine with --scst-samples" in capsys.readouterr().err


def test_the_step_classes_refuse_the_same_combinations():
    """TrainStep / BucketedTrainer name the conflict before they touch a model or a device."""
    from mtn_amd.train_step import BucketedTrainer, SchedConfig, ScstConfig, TrainStep
    cfg = SchedConfig(0.25)
    for cls, kw in ((TrainStep, dict(model=None, batch=None, vocab=10)), (BucketedTrainer, dict(model=None, corpus=None, vocab_size=10))):
        with pytest.raises(ValueError, match="sched .*does not combine with a teacher"):
            cls(sched=cfg, teacher=object(), **kw)
        with pytest.raises(ValueError, match="sched .*does not combine with scst"):
            cls(sched=cfg, scst=ScstConfig(), **kw)
