"""`python train.py --distill-model ...` (mtn_amd.train) on the GPU, end to end, on the mini AVSD fixture with a teacher checkpoint written
by a one-epoch run (the way tests/test_generate_ensemble_gpu.py makes its checkpoints): the distilled epoch ends with finite losses and
logs the distillation KL line, graphed and eager; --distill-alpha 0 gives the mean training loss of the run without the flag, exactly."""
import json
import math
import os
import re

import pytest
import torch

from tests.test_dataset_frontend import _features

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
KL_LINE = re.compile(r"^epoch 1 mean distillation KL per token: (\S+)$", re.M)


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    from mtn_amd import lib, train
    os.environ["MTN_EMBED_DETERMINISTIC"] = "1"          # the atomic-free embedding gradient: runs are bitwise reproducible
    lib.reload_env()
    tmp = tmp_path_factory.mktemp("train_distill")
    raw = json.load(open(os.path.join(GOLD, "mini_avsd.json")))
    _, fea_path = _features(tmp, raw)
    prefix = str(tmp / "teacher" / "mtn")
    base = ["--fea-type", "i3d", "vgg", "--train-path", fea_path, "--train-set", os.path.join(GOLD, "mini_avsd.json"), "--num-epochs", "1",
            "--batch-size", "4", "--max-length", "256", "--include-caption", "caption,summary", "--separate-caption", "1",
            "--max-history-length", "3", "--nb-blocks", "1", "--d-model", "128", "--d-ff", "256", "--att-h", "4", "--dropout", "0.1",
            "--warmup-steps", "20", "--report-interval", "1000"]
    train.main(base + ["--model", prefix, "--rand-seed", "7"])
    assert os.path.exists(prefix + "_1.pth.tar") and os.path.exists(prefix + ".conf")
    yield dict(base=base, flags=["--distill-model", prefix + "_1", "--distill-conf", prefix + ".conf"])
    del os.environ["MTN_EMBED_DETERMINISTIC"]
    lib.reload_env()


@pytest.mark.parametrize("eager", [False, True], ids=["graphed", "eager"])
def test_a_distilled_epoch_is_finite_and_logs_the_kl(run, capsys, eager):
    from mtn_amd import train
    capsys.readouterr()
    means = train.main(run["base"] + run["flags"] + ["--distill-temperature", "2"] + (["--eager"] if eager else []))
    out = capsys.readouterr().out
    assert len(means) == 1 and math.isfinite(means[0]) and means[0] > 0
    m = KL_LINE.search(out)
    assert m, out
    kd = float(m.group(1))
    assert math.isfinite(kd) and kd > 0
    assert "epoch 1 mean train loss per token" in out


def test_alpha_zero_is_the_run_without_the_flag(run, capsys):
    from mtn_amd import train
    plain = train.main(run["base"])
    assert not KL_LINE.search(capsys.readouterr().out)                   # without --distill-model the log is what it was
    zero = train.main(run["base"] + run["flags"] + ["--distill-alpha", "0"])
    out = capsys.readouterr().out
    assert plain == zero, (plain, zero)
    assert float(KL_LINE.search(out).group(1)) == 0.0


SYN = ["--corpus-videos", "4", "--num-epochs", "1", "--batch-size", "8", "--nb-blocks", "1", "--d-model", "64", "--d-ff", "128", "--att-h", "4",
       "--vocab-size", "64", "--ft-sizes", "16", "8", "--warmup-steps", "20", "--report-interval", "1000"]


@pytest.fixture(scope="module")
def syn_teacher(run, tmp_path_factory):
    """A teacher for the synthetic corpus (vocabulary 64, a multiple of 8: the fused HIP loss head runs, which the mini AVSD vocabulary
    does not allow): the checkpoint of a one-epoch run, and a conf written by hand — synthetic runs write none."""
    import pickle
    from mtn_amd import train
    tmp = tmp_path_factory.mktemp("train_distill_syn")
    prefix = str(tmp / "mtn")
    train.main(SYN + ["--model", prefix, "--rand-seed", "7"])
    with open(prefix + ".conf", "wb") as f:
        pickle.dump(({"w%d" % i: i for i in range(64)}, train.parse(SYN)), f, -1)
    return ["--distill-model", prefix + "_1", "--distill-conf", prefix + ".conf"]


@pytest.mark.parametrize("mode", ["graphed", "eager", "fixed-batch"])
def test_synthetic_data_with_a_teacher_through_the_hip_head(syn_teacher, capsys, mode):
    from mtn_amd import train
    if mode == "fixed-batch":
        assert SYN[:2] == ["--corpus-videos", "4"] and SYN[-2:] == ["--report-interval", "1000"]
        base = SYN[2:-2] + ["--steps-per-epoch", "6", "--lens", "8", "16", "12", "8", "10", "--report-interval", "6"]
    else:
        base = SYN + (["--eager"] if mode == "eager" else [])
    capsys.readouterr()
    step_loss = lambda text: re.findall(r"^Epoch: 1 Step: 6 Loss: (\S+)", text, re.M)      # fixed-batch mode returns nothing: its log line
    plain = train.main(base)
    plain_out = capsys.readouterr().out
    assert not KL_LINE.search(plain_out)
    zero = train.main(base + syn_teacher + ["--distill-alpha", "0"])
    out = capsys.readouterr().out
    assert plain == zero, (plain, zero)
    if mode == "fixed-batch":
        assert len(step_loss(plain_out)) == 1 and step_loss(plain_out) == step_loss(out)
    assert float(KL_LINE.search(out).group(1)) == 0.0
    dist = train.main(base + syn_teacher + ["--distill-temperature", "2"])
    out = capsys.readouterr().out
    kd = float(KL_LINE.search(out).group(1))
    assert math.isfinite(kd) and kd > 0
    if mode != "fixed-batch":
        assert math.isfinite(dist[0]) and dist[0] != plain[0]
