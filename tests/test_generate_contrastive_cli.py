"""--decode-style contrastive at generate.py's command line and in the functions behind it, without a GPU: the flags parse with their
defaults and ranges, every flag the search does not combine with ends the run naming it, the --decode-style error lists the new style,
the keyword checks of decode.py / generate_response raise ValueError, and build_result writes "contrastive" only when it is given."""
import pytest

from mtn_amd import generate as G

BASE = ["--decode-style", "contrastive"]


def _error(capsys, argv):
    with pytest.raises(SystemExit) as e:
        G.parse(argv)
    assert e.value.code == 2
    return capsys.readouterr().err


def test_flags_parse_with_defaults():
    a = G.parse(BASE)
    assert (a.decode_style, a.contrastive_k, a.contrastive_alpha, a.min_length) == ("contrastive", 5, 0.6, 1)
    a = G.parse(BASE + ["--contrastive-k", "12", "--contrastive-alpha", "1", "--min-length", "4", "--penalty", "0.5", "--maxlen", "20",
                        "--dialogues-per-search", "3", "--evaluate", "--no-buckets"])
    assert (a.contrastive_k, a.contrastive_alpha, a.min_length, a.penalty, a.maxlen, a.dialogues_per_search, a.evaluate) == (12, 1.0, 4, 0.5, 20, 3, True)
    assert G.parse(BASE + ["--contrastive-k", "1", "--contrastive-alpha", "0"]).contrastive_alpha == 0.0
    a = G.parse([])                                              # other styles: the defaults are there and change nothing
    assert (a.decode_style, a.contrastive_k, a.contrastive_alpha) == ("greedy", 5, 0.6)
    assert G.CONTRASTIVE_MAX_K == 12


@pytest.mark.parametrize("argv, needle", [
    (["--contrastive-k", "0"], "--contrastive-k must be in [1, 12]"), (["--contrastive-k", "13"], "--contrastive-k must be in [1, 12]"),
    (["--contrastive-k", "-2"], "--contrastive-k"), (["--contrastive-alpha", "-0.1"], "--contrastive-alpha must be in [0, 1]"),
    (["--contrastive-alpha", "1.01"], "--contrastive-alpha must be in [0, 1]"), (["--contrastive-alpha", "nan"], "--contrastive-alpha"),
    (["--contrastive-alpha", "inf"], "--contrastive-alpha"),
])
def test_ranges(capsys, argv, needle):
    assert needle in _error(capsys, BASE + argv)
    assert needle.split(" ")[0] in _error(capsys, argv)          # the ranges hold under any style


@pytest.mark.parametrize("argv, flag", [
    (["--ensemble-model", "other"], "--ensemble-model"), (["--mbr", "2"], "--mbr"), (["--beam", "6", "--beam-groups", "2"], "--beam-groups"),
    (["--no-repeat-ngram", "3"], "--no-repeat-ngram"), (["--repetition-penalty", "1.2"], "--repetition-penalty"),
    (["--candidates", "c.json"], "--candidates"),
])
def test_every_conflict_is_named(capsys, argv, flag):
    err = _error(capsys, BASE + argv)
    assert flag in err.split("error:")[-1]
    assert "contrastive" in err.split("error:")[-1] or flag == "--candidates"     # (--candidates names the one style it goes with)


def test_decode_style_error_lists_the_new_style(capsys):
    assert "--decode-style must be greedy, beam_search, sample, contrastive or score" in _error(capsys, ["--decode-style", "contrast"])


def test_keyword_checks():
    from mtn_amd import decode as D
    assert D._contrastive(5, 0.6, (3, 1, 0)) == (5, 0.6, (3, 1, 0)) and D._contrastive(1, 0) == (1, 0.0, ()) and D._contrastive(16, 1)[0] == 16
    for k, alpha, banned in ((0, 0.5, ()), (17, 0.5, ()), (2.5, 0.5, ()), (5, -0.1, ()), (5, 1.5, ()), (5, float("nan"), ()), (5, 0.5, (1, 2, 3, 4, 5))):
        with pytest.raises(ValueError):
            D._contrastive(k, alpha, banned)
    ens = D.Ensemble.__new__(D.Ensemble)                          # (never run: the refusal comes first)
    with pytest.raises(ValueError, match="Ensemble"):
        D.contrastive_decode_many(ens, None, 20, 0, 2, 1)
    for kw in (dict(mbr=2), dict(no_repeat_ngram=3), dict(repetition_penalty=1.5), dict(contrastive=dict(k=0)), dict(contrastive=dict(alpha=2.0)), dict(candidates={}), dict(beam_groups=2),
               dict(diversity_penalty=0.5)):
        with pytest.raises(ValueError):
            G.generate_response(None, None, None, {"<eos>": 2}, decode_style="contrastive", **kw)
    with pytest.raises(ValueError):
        G.generate_response(ens, None, None, {"<eos>": 2}, decode_style="contrastive")


def test_build_result_writes_contrastive_only_when_given():
    original = {"dialogs": [{"image_id": "v1", "dialog": [{"question": "q1", "answer": "a1"}, {"question": "q2", "answer": "a2"}]}]}
    cs = [dict(score=-1.0, logp=[-0.5, -0.5], penalty=[0.1, 0.2], rank=[0, 1]), dict(score=-2.0, logp=[-2.0], penalty=[0.3], rank=[2])]
    res = G.build_result(original, False, ["x", "y"], contrastive=cs)
    assert [t["contrastive"] for t in res["dialogs"][0]["dialog"]] == cs and [t["answer"] for t in res["dialogs"][0]["dialog"]] == ["x", "y"]
    plain = G.build_result(original, False, ["x", "y"])
    assert all(set(t) == {"question", "answer"} for t in plain["dialogs"][0]["dialog"])
