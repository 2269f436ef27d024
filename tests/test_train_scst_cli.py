"""train.py's self-critical-training flags at the command line: defaults, validation and the conflict messages (no GPU needed)."""
import pytest

from mtn_amd import train

CORPUS = ["--corpus-videos", "4"]


def test_flags_parse_with_their_defaults():
    a = train.parse([])
    assert a.scst_samples == 0 and a.scst_reward == "cider" and a.scst_baseline == "mean"
    assert a.scst_temperature == 1.0 and a.scst_top_k == 0 and a.scst_top_p == 1.0 and a.scst_xe_weight == 0.0
    a = train.parse(CORPUS + ["--scst-samples", "4", "--scst-reward", "rouge", "--scst-baseline", "greedy", "--scst-temperature", "0.7",
                              "--scst-top-k", "20", "--scst-top-p", "0.9", "--scst-xe-weight", "0.5", "--ema-decay", "0.99", "--resume", "x/mtn_1"])
    assert (a.scst_samples, a.scst_reward, a.scst_baseline, a.scst_temperature, a.scst_top_k, a.scst_top_p, a.scst_xe_weight) == (
        4, "rouge", "greedy", 0.7, 20, 0.9, 0.5)
    assert a.ema_decay == 0.99 and a.resume == "x/mtn_1"                  # both combine with the flag
    for s in (2, 16):
        assert train.parse(CORPUS + ["--scst-samples", str(s)]).scst_samples == s
    assert train.parse(["--train-set", "t.json", "--scst-samples", "2"]).scst_samples == 2
    # the companions mean nothing without --scst-samples and are not validated then
    assert train.parse(["--scst-top-p", "0.5", "--scst-xe-weight", "1"]).scst_samples == 0


@pytest.mark.parametrize("argv,word", [
    (["--scst-samples", "1"], "2..16"),
    (["--scst-samples", "17"], "2..16"),
    (["--scst-samples", "-2"], "2..16"),
    (["--scst-samples", "2", "--scst-reward", "bleu"], "--scst-reward"),
    (["--scst-samples", "2", "--scst-baseline", "median"], "--scst-baseline"),
    (["--scst-samples", "2", "--scst-temperature", "-1"], "--scst-temperature"),
    (["--scst-samples", "2", "--scst-temperature", "nan"], "--scst-temperature"),
    (["--scst-samples", "2", "--scst-temperature", "inf"], "--scst-temperature"),
    (["--scst-samples", "2", "--scst-top-k", "-1"], "--scst-top-k"),
    (["--scst-samples", "2", "--scst-top-p", "0"], "--scst-top-p"),
    (["--scst-samples", "2", "--scst-top-p", "1.5"], "--scst-top-p"),
    (["--scst-samples", "2", "--scst-xe-weight", "-0.5"], "--scst-xe-weight"),
    (["--scst-samples", "2", "--scst-xe-weight", "inf"], "--scst-xe-weight"),
    (["--scst-samples", "2", "--max-length", "1"], "--max-length"),
])
def test_bad_flags_are_refused_with_a_message(argv, word, capsys):
    with pytest.raises(SystemExit) as e:
        train.parse(CORPUS + argv)
    assert e.value.code == 2
    assert word in capsys.readouterr().err


def test_conflicts_are_named(capsys, monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit):
        train.parse(CORPUS + ["--scst-samples", "2", "--distill-model", "t/a_1", "--distill-conf", "t/a.conf"])
    err = capsys.readouterr().err
    assert "--scst-samples" in err and "--distill-model" in err and "out of scope" in err
    with pytest.raises(SystemExit):
        train.parse(["--scst-samples", "2"])                              # neither --train-set nor --corpus-videos
    err = capsys.readouterr().err
    assert "--scst-samples" in err and "fixed synthetic batch" in err
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit):
        train.parse(CORPUS + ["--scst-samples", "2"])
    err = capsys.readouterr().err
    assert "--scst-samples" in err and "more than one rank (2)" in err
    assert train.parse(CORPUS).scst_samples == 0                          # two ranks without the flag: nothing to refuse


def test_the_conflict_check_takes_the_rank_count_it_is_given(monkeypatch):
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    a = train.parse(CORPUS + ["--scst-samples", "2"])
    assert train.scst_flag_error(a) is None and train.scst_flag_error(a, world=1) is None
    assert "more than one rank (4)" in train.scst_flag_error(a, world=4)
    assert train.scst_flag_error(train.parse([]), world=4) is None
