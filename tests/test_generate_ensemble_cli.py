"""generate.py's ensemble flags at the command line, the conf checks behind them and mtn_ensemble_rows at the ABI boundary (no GPU needed)."""
import argparse
import ctypes
import os
import pickle
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_parse_accepts_the_four_flags(capsys):
    from mtn_amd import generate as G
    a = G.parse(["--model", "exp/mtn_best", "--model-conf", "exp/mtn.conf", "--ensemble-model", "s2/mtn_best", "s3/mtn_best",
                 "--ensemble-conf", "s2/mtn.conf", "s3/mtn.conf", "--ensemble-weights", "2", "1", "0.5", "--ensemble-mode", "logprob"])
    assert (a.model, a.model_conf) == ("exp/mtn_best", "exp/mtn.conf")                      # still single strings
    assert a.ensemble_model == ["s2/mtn_best", "s3/mtn_best"] and a.ensemble_conf == ["s2/mtn.conf", "s3/mtn.conf"]
    assert a.ensemble_weights == [2.0, 1.0, 0.5] and a.ensemble_mode == "logprob"
    b = G.parse(["--model", "m", "--ensemble-model", "n"])                                  # confs and weights are optional
    assert b.ensemble_model == ["n"] and b.ensemble_conf == [] and b.ensemble_weights is None and b.ensemble_mode == "prob"
    c = G.parse(["--decode-style", "beam_search"])                                          # without the flags: nothing of an ensemble
    assert c.ensemble_model == [] and c.ensemble_conf == [] and c.ensemble_weights is None and c.ensemble_mode == "prob"
    assert isinstance(c.model, str) and isinstance(c.model_conf, str)
    for style in ("greedy", "beam_search", "sample", "score"):
        assert G.parse(["--decode-style", style, "--ensemble-model", "n"]).decode_style == style


@pytest.mark.parametrize("argv,word", [
    (["--ensemble-model", "a", "b", "--ensemble-conf", "a.conf"], "--ensemble-conf"),          # conf count != model count
    (["--ensemble-conf", "a.conf"], "--ensemble-conf"),
    (["--ensemble-model", "a", "--ensemble-weights", "1", "1", "1"], "--ensemble-weights"),     # weight count != M
    (["--ensemble-model", "a", "--ensemble-weights", "1"], "--ensemble-weights"),
    (["--ensemble-model", "a", "--ensemble-weights", "1", "-0.5"], "--ensemble-weights"),       # a negative weight
    (["--ensemble-model", "a", "--ensemble-weights", "0", "0"], "--ensemble-weights"),          # all of them 0
    (["--ensemble-model", "a", "--ensemble-weights", "nan", "1"], "--ensemble-weights"),
    (["--ensemble-model", "a", "--ensemble-mode", "mean"], "--ensemble-mode"),                  # an unknown mode
    (["--ensemble-model"] + list("abcdefgh"), "8 members"),
])
def test_parse_error_exits(argv, word, capsys):
    from mtn_amd import generate as G
    with pytest.raises(SystemExit) as e:
        G.parse(argv)
    assert e.value.code == 2
    assert word in capsys.readouterr().err


def _conf(path, vocab, **over):
    from mtn_amd import generate as G
    fields = dict(G.REFERENCE_TRAIN_DEFAULTS, fea_type=["i3d", "vgg"], include_caption="caption,summary", separate_caption=1,
                  max_history_length=3, merge_source=0, nb_blocks=1, d_model=128)
    fields.update(over)
    with open(path, "wb") as f:
        pickle.dump((vocab, argparse.Namespace(**fields)), f)
    return str(path)


def test_conf_mismatches_end_the_run(tmp_path):
    from mtn_amd import generate as G
    vocab = {"<unk>": 0, "<blank>": 1, "<sos>": 2, "<eos>": 3, "a": 4, "b": 5}
    base = _conf(tmp_path / "m0.conf", vocab)
    # members may differ in architecture: depth, width, auto_encoder_ft
    other = _conf(tmp_path / "m1.conf", dict(vocab), nb_blocks=2, d_model=256, d_ff=512, auto_encoder_ft="caption")
    confs = G.load_ensemble_confs(base, ["x", "y"], [other, base])
    assert len(confs) == 3 and confs[1][1].nb_blocks == 2 and confs[0][0] == vocab
    assert len(G.load_ensemble_confs(base, ["x", "y"], [])) == 3                           # no --ensemble-conf: --model-conf for everyone
    # the same tokens under other ids, one token more, one token fewer: not the same map
    for bad_vocab in (dict(vocab, a=5, b=4), dict(vocab, c=6), {k: v for k, v in vocab.items() if k != "b"}):
        bad = _conf(tmp_path / "bad.conf", bad_vocab)
        with pytest.raises(SystemExit) as e:
            G.load_ensemble_confs(base, ["x"], [bad])
        assert "vocabulary" in str(e.value) and "bad.conf" in str(e.value)
    # every data-shaping field, named in the message
    for field, value in (("fea_type", ["i3d"]), ("include_caption", "caption"), ("separate_caption", 0), ("max_history_length", 2),
                         ("merge_source", 1)):
        bad = _conf(tmp_path / "bad.conf", vocab, **{field: value})
        with pytest.raises(SystemExit) as e:
            G.load_ensemble_confs(base, ["x", "y"], [base, bad])
        assert field in str(e.value) and "member 2" in str(e.value), str(e.value)
    # the FIRST differing field of the first differing member
    bad = _conf(tmp_path / "bad.conf", vocab, merge_source=1, include_caption="none")
    with pytest.raises(SystemExit) as e:
        G.load_ensemble_confs(base, ["x"], [bad])
    assert "include_caption" in str(e.value) and "merge_source" not in str(e.value)
    with pytest.raises(SystemExit):
        G.load_ensemble_confs(base, ["x", "y"], [base])                                    # one conf per member


def test_ensemble_weights_are_normalised_in_float64():
    import numpy as np
    from mtn_amd import ops
    w = ops.ensemble_weights(3, [2, 1, 1])
    assert w.dtype == np.float64 and w.tolist() == [0.5, 0.25, 0.25]
    assert ops.ensemble_weights(4).tolist() == [0.25] * 4
    assert ops.ensemble_weights(2, [0, 3]).tolist() == [0.0, 1.0]
    for bad in ([1.0], [1, -1], [0, 0], [float("inf"), 1], [float("nan"), 1]):
        with pytest.raises(ValueError):
            ops.ensemble_weights(2, bad)


def test_header_and_ctypes_agree_on_mtn_ensemble_args(tmp_path):
    from mtn_amd import lib
    hdr = open(os.path.join(ROOT, "include", "mtn_hip.h")).read()
    m = re.search(r"int\s+mtn_ensemble_rows\s*\(([^)]*)\)", hdr)
    assert m and re.match(r"\s*const\s+mtn_ensemble_args\s*\*", m.group(1))
    assert "mtn_ensemble_rows" in lib.SYMBOLS
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mtn_hip.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(mtn_ensemble_args),'
                   ' offsetof(mtn_ensemble_args, x), offsetof(mtn_ensemble_args, ld), offsetof(mtn_ensemble_args, w), offsetof(mtn_ensemble_args, out),'
                   ' offsetof(mtn_ensemble_args, ldo));return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    sizes = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    E = lib.EnsembleArgs
    assert sizes == [ctypes.sizeof(E), E.x.offset, E.ld.offset, E.w.offset, E.out.offset, E.ldo.offset]


def test_ensemble_class_refuses_misuse_without_a_gpu():
    import torch
    from mtn_amd import decode as D
    from mtn_amd import make_model
    mk = lambda v: make_model(v, v, N=1, d_model=32, d_ff=64, h=2, dropout=0.0, ft_sizes=[8], diff_encoder=True, auto_encoder_ft="query",
                              compute_dtype=torch.float32)
    a, b, c = mk(20), mk(20), mk(24)
    e = D.Ensemble([a, b], weights=[3, 1], mode="logprob")
    assert e.weights == (0.75, 0.25) and e.mode == "logprob" and e.vocab == 20 and e.active == [a, b]
    assert D.Ensemble([a, b], weights=[0, 1]).active == [b]
    assert e.same_members(D.Ensemble([a, b])) and not e.same_members(D.Ensemble([b, a])) and not e.same_members(a)
    assert e.signature() != D.Ensemble([a, b]).signature()                                  # weights and mode are part of a session's key
    for bad in (lambda: D.Ensemble([]), lambda: D.Ensemble([a, a]), lambda: D.Ensemble([a, c]), lambda: D.Ensemble([a, b], mode="mean"),
                lambda: D.Ensemble([a, b], weights=[1]), lambda: D.Ensemble([a, b], weights=[-1, 2]), lambda: D.Ensemble([a, b], weights=[0, 0]),
                lambda: D.Ensemble([mk(20) for _ in range(9)])):
        with pytest.raises(ValueError):
            bad()
