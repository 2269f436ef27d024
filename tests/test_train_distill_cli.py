"""train.py's knowledge-distillation flags at the command line and the conf checks behind them (no GPU needed)."""
import argparse

import pytest

from mtn_amd import train


def test_flags_parse_with_their_defaults():
    a = train.parse([])
    assert a.distill_model == [] and a.distill_conf == [] and a.distill_weights is None
    assert a.distill_mode == "prob" and a.distill_alpha == 0.5 and a.distill_temperature == 1.0
    a = train.parse(["--distill-model", "t/a_1", "t/a_2", "--distill-conf", "t/a.conf", "--distill-weights", "2", "1", "--distill-mode", "logprob",
                     "--distill-alpha", "0.3", "--distill-temperature", "2"])
    assert a.distill_model == ["t/a_1", "t/a_2"] and a.distill_conf == ["t/a.conf"] and a.distill_weights == [2.0, 1.0]
    assert a.distill_mode == "logprob" and a.distill_alpha == 0.3 and a.distill_temperature == 2.0
    a = train.parse(["--distill-model", "a", "b", "--distill-conf", "a.conf", "b.conf", "--distill-alpha", "0", "--batch-size", "4"])
    assert a.distill_conf == ["a.conf", "b.conf"] and a.distill_alpha == 0.0 and a.batch_size == 4


@pytest.mark.parametrize("argv,word", [
    (["--distill-model", "a", "--distill-conf", "a.conf", "--distill-alpha", "1.5"], "--distill-alpha"),
    (["--distill-model", "a", "--distill-conf", "a.conf", "--distill-alpha", "-0.1"], "--distill-alpha"),
    (["--distill-model", "a", "--distill-conf", "a.conf", "--distill-alpha", "nan"], "--distill-alpha"),
    (["--distill-model", "a", "--distill-conf", "a.conf", "--distill-temperature", "0"], "--distill-temperature"),
    (["--distill-model", "a", "--distill-conf", "a.conf", "--distill-temperature", "-2"], "--distill-temperature"),
    (["--distill-model", "a", "--distill-conf", "a.conf", "--distill-temperature", "inf"], "--distill-temperature"),
    (["--distill-model"] + ["m%d" % i for i in range(9)] + ["--distill-conf", "a.conf"], "at most 8"),
    (["--distill-model", "a", "b", "c", "--distill-conf", "a.conf", "b.conf"], "one conf per"),
    (["--distill-conf", "a.conf"], "needs --distill-model"),
    (["--distill-model", "a"], "needs --distill-conf"),
    (["--distill-model", "a", "b", "--distill-conf", "a.conf", "--distill-weights", "1"], "one weight per"),
    (["--distill-model", "a", "b", "--distill-conf", "a.conf", "--distill-weights", "0", "0"], "not all 0"),
    (["--distill-model", "a", "b", "--distill-conf", "a.conf", "--distill-weights", "1", "-1"], ">= 0"),
    (["--distill-model", "a", "--distill-conf", "a.conf", "--distill-mode", "mean"], "--distill-mode"),
])
def test_bad_flags_are_refused_with_a_message(argv, word, capsys):
    with pytest.raises(SystemExit) as e:
        train.parse(argv)
    assert e.value.code == 2
    assert word in capsys.readouterr().err


def _conf(vocab, **kw):
    a = dict(fea_type=["i3d", "vgg"], include_caption="caption,summary", separate_caption=1, max_history_length=3, merge_source=0)
    a.update(kw)
    return dict(vocab), argparse.Namespace(**a)


def test_a_vocabulary_mismatch_names_the_first_differing_word():
    vocab = {"<unk>": 0, "<blank>": 1, "<sos>": 2, "<eos>": 3, "a": 4, "dog": 5, "runs": 6}
    args = train.parse(["--fea-type", "i3d", "vgg", "--include-caption", "caption,summary", "--max-history-length", "3"])
    train.check_distill_confs([_conf(vocab)], ["t.conf (teacher 0)"], vocab, args)                   # equal maps: accepted
    swapped = dict(vocab, dog=6, runs=5)
    with pytest.raises(SystemExit) as e:
        train.check_distill_confs([_conf(vocab), _conf(swapped)], ["t0.conf (teacher 0)", "t1.conf (teacher 1)"], vocab, args)
    assert "t1.conf (teacher 1)" in str(e.value) and "'dog'" in str(e.value) and "'runs'" not in str(e.value)
    missing = {k: v for k, v in vocab.items() if k != "a"}
    with pytest.raises(SystemExit) as e:
        train.check_distill_confs([_conf(missing)], ["t.conf (teacher 0)"], vocab, args)
    assert "'a'" in str(e.value) and "missing" in str(e.value)
    more = dict(vocab, cat=7)                                                                          # same size check is not enough either way
    with pytest.raises(SystemExit) as e:
        train.check_distill_confs([_conf(more)], ["t.conf (teacher 0)"], vocab, args)
    assert "'cat'" in str(e.value)
    assert train.vocab_difference(vocab, dict(vocab)) is None


def test_a_data_shaping_field_that_differs_is_named():
    vocab = {"<unk>": 0, "<blank>": 1, "a": 2}
    args = train.parse(["--fea-type", "i3d", "vgg", "--include-caption", "caption,summary", "--max-history-length", "3"])
    with pytest.raises(SystemExit) as e:
        train.check_distill_confs([_conf(vocab, max_history_length=2)], ["t.conf (teacher 0)"], vocab, args)
    assert "max_history_length" in str(e.value) and "t.conf (teacher 0)" in str(e.value)
    with pytest.raises(SystemExit) as e:
        train.check_distill_confs([_conf(vocab, fea_type=["i3d"])], ["t.conf (teacher 0)"], vocab, args)
    assert "fea_type" in str(e.value)


def test_synthetic_data_compares_the_vocabulary_size():
    args = train.parse(["--vocab-size", "64"])
    train.check_distill_confs([_conf({"w%d" % i: i for i in range(64)})], ["t.conf"], None, args)
    with pytest.raises(SystemExit) as e:
        train.check_distill_confs([_conf({"w%d" % i: i for i in range(60)})], ["t.conf"], None, args)
    assert "60" in str(e.value) and "64" in str(e.value)


def test_no_teacher_without_the_flag():
    assert train.load_teacher(train.parse([]), None, None) is None
