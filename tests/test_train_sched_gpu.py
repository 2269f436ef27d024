"""`python train.py --sched-sample-prob P` (mtn_amd.train) on the GPU, end to end, on a small synthetic corpus: every epoch logs its
scheduled-sampling line with consistent counters, validation and the checkpoint schema are what they are without the flag, generate.py's
loader takes the checkpoint, --resume continues the schedule and its draws, and --eager and the fixed synthetic batch take the flag too."""
import contextlib
import io
import math
import os
import re

import pytest
import torch

pytestmark = pytest.mark.gpu
SYN = ["--corpus-videos", "2", "--valid-videos", "1", "--num-epochs", "1", "--batch-size", "4", "--nb-blocks", "1", "--d-model", "64", "--d-ff", "128",
       "--att-h", "4", "--vocab-size", "64", "--ft-sizes", "16", "8", "--warmup-steps", "20", "--report-interval", "1000", "--rand-seed", "7"]
SCHED = ["--sched-sample-prob", "0.5", "--sched-sample-start", "1", "--sched-sample-ramp", "4", "--sched-sample-pick", "sample",
         "--sched-sample-temperature", "0.8", "--sched-sample-seed", "3"]
LINE = re.compile(r"^epoch (\d+) scheduled sampling: p (\S+) replaced (\d+) of (\d+) target tokens, (\d+) differ from gold$", re.M)
VALID = re.compile(r"^epoch: (\d+) validation loss: (\S+)$", re.M)


def _main(argv):
    from mtn_amd import train
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        means = train.main(argv)
    return means, buf.getvalue()


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    from mtn_amd import lib
    os.environ["MTN_EMBED_DETERMINISTIC"] = "1"
    lib.reload_env()
    tmp = tmp_path_factory.mktemp("train_sched")
    out = {}
    for key, extra in (("sched", SCHED), ("plain", [])):
        (tmp / key).mkdir()
        means, log = _main(SYN + ["--model", str(tmp / key / "m")] + extra)
        out[key] = dict(dir=tmp / key, means=means, log=log)
    yield out
    del os.environ["MTN_EMBED_DETERMINISTIC"]
    lib.reload_env()


def _load(path):
    return torch.load(str(path), map_location="cpu", weights_only=True)


def _updates(run):
    return int(torch.load(str(run["dir"] / "m_1_opt.pth.tar"), map_location="cpu")["step"])


def test_the_epoch_logs_consistent_counters(runs):
    from mtn_amd.train_step import SchedConfig
    got = LINE.findall(runs["sched"]["log"])
    assert len(got) == 1 and got[0][0] == "1", runs["sched"]["log"]
    p, k, n, d = float(got[0][1]), int(got[0][2]), int(got[0][3]), int(got[0][4])
    steps = _updates(runs["sched"])
    assert steps >= 5                                                        # the ramp (1 + 4 updates) ends inside the epoch
    assert abs(p - SchedConfig(0.5, start=1, ramp=4).prob_at(steps)) < 1e-6 and abs(p - 0.5) < 1e-6
    assert 0 <= d <= k <= n and 0 < k < n
    assert not LINE.search(runs["plain"]["log"])
    assert all(math.isfinite(v) for v in runs["sched"]["means"]) and runs["sched"]["means"] != runs["plain"]["means"]


def test_validation_and_the_checkpoint_schema_are_the_plain_runs(runs):
    vs, vp = VALID.findall(runs["sched"]["log"]), VALID.findall(runs["plain"]["log"])
    assert [e for e, _ in vs] == [e for e, _ in vp] == ["1"] and all(math.isfinite(float(v)) for _, v in vs)
    a, b = _load(runs["sched"]["dir"] / "m_1.pth.tar"), _load(runs["plain"]["dir"] / "m_1.pth.tar")
    assert list(a) == list(b) and all(a[k].shape == b[k].shape and a[k].dtype == b[k].dtype for k in a)
    assert any(not torch.equal(a[k], b[k]) for k in a)                       # it trained on other inputs
    assert _updates(runs["sched"]) == _updates(runs["plain"])
    oa = torch.load(str(runs["sched"]["dir"] / "m_1_opt.pth.tar"), map_location="cpu")["optimizer"]
    ob = torch.load(str(runs["plain"]["dir"] / "m_1_opt.pth.tar"), map_location="cpu")["optimizer"]
    assert set(oa) == set(ob)                                                # no new optimiser state: the stream is a function of the step


def test_generate_loads_the_checkpoint(runs):
    from mtn_amd import generate as gen
    from mtn_amd import train
    from mtn_amd.synthetic import synthetic_batch
    dev = torch.device("cuda:0")
    args = train.parse(SYN)
    vocab = {"w%d" % i: i for i in range(64)}
    sd = gen.load_state_dict(str(runs["sched"]["dir"] / "m_best") + ".pth.tar")
    model = gen.build_model(vocab, args, args.ft_sizes, sd, "bf16", dev)
    b = synthetic_batch(64, 4, 8, 16, 12, 8, [10, 10], args.ft_sizes, device=dev, seed=3)
    with torch.no_grad():
        out, _ = model.forward(b)
    assert out.shape[0] == 4 and bool(torch.isfinite(out.float()).all())


def test_resume_continues_the_schedule(runs, tmp_path):
    d = runs["sched"]["dir"]
    before = _updates(runs["sched"])
    means, log = _main(SYN + SCHED + ["--model", str(tmp_path / "r"), "--resume", str(d / "m_1")])
    got = LINE.findall(log)
    assert len(means) == 1 and math.isfinite(means[0]) and len(got) == 1
    k, n, dd = int(got[0][2]), int(got[0][3]), int(got[0][4])
    assert 0 <= dd <= k <= n and 0 < k < n and abs(float(got[0][1]) - 0.5) < 1e-6
    after = int(torch.load(str(tmp_path / "r_1_opt.pth.tar"), map_location="cpu")["step"])
    assert after == 2 * before                                               # the step word went on from the file's
    # past the ramp from its first update on: the resumed epoch replaces more than the first, which began at p = 0
    first = LINE.findall(runs["sched"]["log"])[0]
    assert n == int(first[3]) and k > int(first[2])


@pytest.mark.parametrize("mode", ["eager", "fixed-batch", "accum-clip-ul"])
def test_the_other_modes_take_the_flags(tmp_path, mode):
    if mode == "eager":
        argv = SYN + ["--eager"]
    elif mode == "accum-clip-ul":
        argv = SYN + ["--accum-steps", "2", "--clip-grad-norm", "1", "--unlikelihood-alpha", "0.5", "--ema-decay", "0.99", "--cut-a", "1"]
    else:
        argv = SYN[4:] + ["--steps-per-epoch", "6", "--lens", "8", "16", "12", "8", "10"]
    means, log = _main(argv + ["--model", str(tmp_path / "m"), "--sched-sample-prob", "0.5"])
    got = LINE.findall(log)
    assert len(got) == 1, log
    p, k, n, d = float(got[0][1]), int(got[0][2]), int(got[0][3]), int(got[0][4])
    assert abs(p - 0.5) < 1e-6 and 0 <= d <= k <= n and 0 < k < n
    assert abs(k - 0.5 * n) <= 5.0 * math.sqrt(0.25 * n)                     # the coin's rate, within its binomial interval
    assert (tmp_path / "m_1.pth.tar").exists()
