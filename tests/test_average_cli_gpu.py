"""`python average.py --inputs ... --output ...` (mtn_amd.average) on the GPU over three small checkpoints: every floating-point tensor is the
float64 weighted mean within 8 K 2^-24 max_k |x_k| per element (each of the K updates rounds three times, each time at most 2^-24 of a
magnitude no larger than 2 max |x|) and the running mean of tests/average_refs.py bit for bit; --weights is honoured; identical inputs
come back bit for bit; integer entries are copied; a missing key, a changed shape or dtype and bad weights end the run naming the cause."""
import os
import runpy
import sys

import numpy as np
import pytest
import torch

from tests import average_refs as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
SHAPES = {"enc.w": (7, 5), "enc.bias": (4099,), "dec.w": (64, 64), "dec.scale": (1,), "gen.proj": (3, 2, 9)}


def _values(rs, shape):
    n = int(np.prod(shape))
    x = (10.0 ** rs.uniform(-6, 3, n) * rs.choice([-1.0, 1.0], n)).astype(F)
    x[rs.rand(n) < 0.05] = 0.0
    return torch.from_numpy(x.reshape(shape))


def _checkpoint(seed):
    rs = np.random.RandomState(seed)
    sd = {}
    for i, (k, shape) in enumerate(SHAPES.items()):
        sd[k] = _values(rs, shape)
        if i == 1:                                                   # non-float entries between the float ones
            sd["steps"] = torch.tensor([3, 1, 4, 1, 5], dtype=torch.int64)
            sd["mask"] = torch.tensor([True, False, True])
    return sd


@pytest.fixture(scope="module")
def ckpts(tmp_path_factory):
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    tmp = tmp_path_factory.mktemp("average")
    sds = [_checkpoint(s) for s in (1, 2, 3)]
    prefixes = []
    for i, sd in enumerate(sds):
        prefixes.append(str(tmp / ("ck_%d" % i)))
        torch.save(sd, prefixes[-1] + ".pth.tar")
    return tmp, prefixes, sds


def _run(argv):
    from mtn_amd import average
    average.main(argv)


def _check_mean(out, sds, weights):
    K = len(sds)
    w = np.asarray(weights, dtype=np.float64)
    assert list(out) == list(sds[0])
    for k, v in sds[0].items():
        got = out[k]
        assert got.dtype == v.dtype and got.shape == v.shape, k
        if not v.is_floating_point():
            assert torch.equal(got, v), k
            continue
        xs = [sd[k].numpy() for sd in sds]
        ref = sum(wk * x.astype(np.float64) for wk, x in zip(w, xs)) / w.sum()
        big = np.max(np.abs(np.stack(xs)), axis=0)
        err = np.abs(got.numpy().astype(np.float64) - ref)
        assert np.all(err <= 8 * K * 2.0 ** -24 * big), (k, float(err.max()))
        assert np.array_equal(got.numpy().view(np.int32), R.running_mean(xs, list(weights)).view(np.int32)), k


@pytest.mark.parametrize("weights", [None, [1, 1, 2], [0, 1, 3]], ids=["uniform", "1-1-2", "0-1-3"])
def test_the_mean_of_three_checkpoints(ckpts, weights):
    tmp, prefixes, sds = ckpts
    out_prefix = str(tmp / "avg")
    _run(["--inputs"] + prefixes + ["--output", out_prefix] + ([] if weights is None else ["--weights"] + [str(w) for w in weights]))
    out = torch.load(out_prefix + ".pth.tar", weights_only=True)
    _check_mean(out, sds, [1, 1, 1] if weights is None else weights)
    if weights == [1, 1, 2]:
        uniform = sum(sd["dec.w"].double() for sd in sds) / 3
        assert not torch.allclose(out["dec.w"].double(), uniform)              # the weights are honoured


def test_the_root_script_runs_the_same_program(ckpts, monkeypatch, capsys):
    tmp, prefixes, sds = ckpts
    monkeypatch.setattr(sys, "argv", ["average.py", "--inputs"] + prefixes[:2] + ["--output", str(tmp / "two")])
    runpy.run_path(os.path.join(ROOT, "average.py"), run_name="__main__")
    assert "2 checkpoint(s)" in capsys.readouterr().out
    _check_mean(torch.load(str(tmp / "two") + ".pth.tar", weights_only=True), sds[:2], [1, 1])


def test_identical_inputs_come_back_bit_for_bit(ckpts):
    tmp, prefixes, sds = ckpts
    for extra in ([], ["--weights", "1", "1", "2"]):
        _run(["--inputs", prefixes[1], prefixes[1], prefixes[1], "--output", str(tmp / "same")] + extra)
        out = torch.load(str(tmp / "same") + ".pth.tar", weights_only=True)
        for k, v in sds[1].items():
            if v.is_floating_point():
                v = v + 0.0                                                  # (x + 0 * (x - x): a negative zero comes back positive)
                assert torch.equal(out[k].view(torch.int32), v.view(torch.int32)), k
            else:
                assert torch.equal(out[k], v), k


def _variant(tmp, name, sd, edit):
    sd = {k: v.clone() for k, v in sd.items()}
    edit(sd)
    torch.save(sd, str(tmp / name) + ".pth.tar")
    return str(tmp / name)


def test_a_difference_between_inputs_ends_the_run_naming_it(ckpts):
    tmp, prefixes, sds = ckpts
    cases = [
        (lambda sd: sd.pop("dec.w"), ["'dec.w'", "missing"]),
        (lambda sd: sd.update({"extra.w": torch.zeros(3)}), ["'extra.w'", "missing"]),
        (lambda sd: sd.update({"enc.bias": sd["enc.bias"][:4096].clone()}), ["'enc.bias'", "shape", "(4096,)"]),
        (lambda sd: sd.update({"dec.scale": sd["dec.scale"].double()}), ["'dec.scale'", "dtype", "float64"]),
        (lambda sd: sd.update({"steps": sd["steps"] + 1}), ["'steps'", "differs"]),
    ]
    for i, (edit, words) in enumerate(cases):
        bad = _variant(tmp, "bad_%d" % i, sds[2], edit)
        with pytest.raises(SystemExit) as e:
            _run(["--inputs", prefixes[0], prefixes[1], bad, "--output", str(tmp / "never")])
        for w in words:
            assert w in str(e.value), (w, str(e.value))
        assert "bad_%d" % i in str(e.value)
        assert not os.path.exists(str(tmp / "never") + ".pth.tar")
    # the FIRST key in the first input's order is the one named
    bad = _variant(tmp, "bad_two", sds[2], lambda sd: (sd.pop("gen.proj"), sd.update({"enc.w": torch.zeros(5, 7)})))
    with pytest.raises(SystemExit) as e:
        _run(["--inputs", prefixes[0], bad, "--output", str(tmp / "never")])
    assert "'enc.w'" in str(e.value) and "gen.proj" not in str(e.value)


@pytest.mark.parametrize("weights,word", [(["1", "1", "-2"], "negative"), (["1", "nan", "1"], "not finite"), (["0", "0", "0"], "all zero")])
def test_bad_weights_end_the_run_naming_the_cause(ckpts, weights, word, capsys):
    tmp, prefixes, _ = ckpts
    with pytest.raises(SystemExit) as e:
        _run(["--inputs"] + prefixes + ["--output", str(tmp / "never"), "--weights"] + weights)
    assert e.value.code == 2 and word in capsys.readouterr().err
    assert not os.path.exists(str(tmp / "never") + ".pth.tar")
