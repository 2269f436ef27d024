"""`python train.py --scst-samples S ...` (mtn_amd.train) on the GPU, end to end, on a tiny synthetic corpus (vocabulary 64, a multiple of
8: the fused HIP loss head runs): two epochs log finite rewards and baselines, graphed and --eager, with the leave-one-out baseline and
with --scst-baseline greedy --scst-xe-weight 0.5; --ema-decay rides along; the checkpoint loads through generate.py's loader; --resume
continues; a graphed run repeats bit for bit from its seed."""
import math
import os
import re

import pytest
import torch

pytestmark = pytest.mark.gpu
SYN = ["--corpus-videos", "3", "--valid-videos", "1", "--num-epochs", "2", "--batch-size", "8", "--nb-blocks", "1", "--d-model", "64", "--d-ff", "128",
       "--att-h", "4", "--vocab-size", "64", "--ft-sizes", "16", "8", "--warmup-steps", "20", "--report-interval", "1000", "--dropout", "0.0",
       "--max-length", "12", "--corpus-max-answer", "8", "--corpus-max-question", "8"]
RL_LINE = re.compile(r"^epoch (\d+) mean reward: (\S+) mean baseline: (\S+)$", re.M)
LOSS_LINE = re.compile(r"^epoch (\d+) mean train loss per token: (\S+)$", re.M)


@pytest.fixture(scope="module", autouse=True)
def deterministic():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    from mtn_amd import lib
    os.environ["MTN_EMBED_DETERMINISTIC"] = "1"          # the atomic-free embedding gradient: runs are bitwise reproducible
    lib.reload_env()
    yield
    del os.environ["MTN_EMBED_DETERMINISTIC"]
    lib.reload_env()


def _rewards(out, epochs=2):
    rows = RL_LINE.findall(out)
    assert [int(r[0]) for r in rows] == list(range(1, epochs + 1)), out
    vals = [(float(r[1]), float(r[2])) for r in rows]
    assert all(math.isfinite(r) and math.isfinite(b) and r >= 0.0 and b >= 0.0 for r, b in vals), vals
    return vals


@pytest.fixture(scope="module")
def mean_run(tmp_path_factory, deterministic):
    """Two epochs with two samples per dialogue, the leave-one-out baseline and an EMA: the run the other tests compare with and resume."""
    import contextlib
    import io
    from mtn_amd import train
    tmp = tmp_path_factory.mktemp("train_scst")
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        means = train.main(SYN + ["--scst-samples", "2", "--model", str(tmp / "m"), "--ema-decay", "0.99"])
    return dict(dir=tmp, means=means, log=buf.getvalue())


def test_two_epochs_log_finite_rewards_and_write_checkpoints(mean_run):
    out, d = mean_run["log"], mean_run["dir"]
    vals = _rewards(out)
    assert len(mean_run["means"]) == 2 and all(math.isfinite(m) for m in mean_run["means"])
    assert all(abs(r - b) < 1e-9 * max(1.0, r) for r, b in vals)          # leave-one-out: the mean baseline is the mean reward
    assert any(r > 0 for r, _ in vals)                                     # some sampled n-gram does occur in its answer
    assert len(LOSS_LINE.findall(out)) == 2 and "validation loss" in out    # validation stays the plain loss
    for e in (1, 2):
        for suffix in ("", "_opt", "_ema"):
            assert os.path.exists(d / ("m_%d%s.pth.tar" % (e, suffix)))
    assert os.path.exists(d / "m_best.pth.tar") and os.path.exists(d / "m_best_ema.pth.tar")


def test_the_checkpoint_loads_in_generate(mean_run):
    from mtn_amd import generate, train
    sd = generate.load_state_dict(str(mean_run["dir"] / "m_2.pth.tar"))
    vocab = {"w%d" % i: i for i in range(64)}
    model = generate.build_model(vocab, train.parse(SYN), [16, 8], sd, "bf16", torch.device("cuda:0"))
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())
    first = generate.load_state_dict(str(mean_run["dir"] / "m_1.pth.tar"))
    assert any(not torch.equal(sd[k], first[k]) for k in sd if sd[k].dtype.is_floating_point)      # the second epoch did train


def test_greedy_baseline_with_gold_rows(capsys, tmp_path):
    from mtn_amd import train
    capsys.readouterr()
    means = train.main(SYN + ["--scst-samples", "2", "--scst-baseline", "greedy", "--scst-xe-weight", "0.5", "--scst-reward", "rouge",
                              "--scst-top-k", "20", "--scst-top-p", "0.95", "--scst-temperature", "0.9"])
    vals = _rewards(capsys.readouterr().out)
    assert len(means) == 2 and all(math.isfinite(m) for m in means)
    assert all(0.0 <= r <= 1.0 and 0.0 <= b <= 1.0 for r, b in vals)        # ROUGE-L lies in [0, 1]


def test_eager_runs_the_same_steps_without_graphs(mean_run, capsys):
    """--eager drives the trainer's steps without captured graphs: as many steps, finite rewards, a loss that falls."""
    from mtn_amd import train
    capsys.readouterr()
    means = train.main(SYN + ["--scst-samples", "2", "--ema-decay", "0.99", "--eager"])
    vals = _rewards(capsys.readouterr().out)
    print("eager", vals, means, "graphed", _rewards(mean_run["log"]), mean_run["means"])
    assert len(means) == 2 and all(math.isfinite(m) for m in means) and means[1] < means[0]
    assert any(r > 0 for r, _ in vals)


def test_a_graphed_run_repeats_from_its_seed(mean_run, capsys):
    from mtn_amd import train
    capsys.readouterr()
    means = train.main(SYN + ["--scst-samples", "2", "--ema-decay", "0.99"])
    vals = _rewards(capsys.readouterr().out)
    assert vals == _rewards(mean_run["log"]) and means == mean_run["means"]


def test_resume_continues(mean_run, capsys):
    """One epoch resumed from the first epoch's checkpoint: the optimiser goes on from its step, the draws from theirs, rewards are logged."""
    from mtn_amd import train
    one = list(SYN)
    one[SYN.index("--num-epochs") + 1] = "1"
    d = mean_run["dir"]
    capsys.readouterr()
    means = train.main(one + ["--scst-samples", "2", "--ema-decay", "0.99", "--model", str(d / "r"), "--resume", str(d / "m_1")])
    out = capsys.readouterr().out
    vals = _rewards(out, epochs=1)
    assert len(means) == 1 and math.isfinite(means[0]) and os.path.exists(d / "r_1.pth.tar")
    # the resumed epoch starts from the first epoch's weights with the draws advanced: it is not the first epoch over again
    assert vals[0] != _rewards(mean_run["log"])[0]


def test_conflicts_end_the_run_with_a_message():
    from mtn_amd import train
    with pytest.raises(SystemExit) as e:
        train.main(["--scst-samples", "2"])
    assert e.value.code == 2
