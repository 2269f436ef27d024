"""`python train.py --clip-grad-norm C` (mtn_amd.train) on the GPU, end to end, on a synthetic corpus: graphed and --eager corpus mode and the
fixed synthetic batch train and log the epoch line; a cap far below the gradient's norm clips every step and changes the run, a cap of
inf measures and changes nothing; --clip-grad-norm 0 is the run without the flag."""
import contextlib
import io
import math
import os
import re

import pytest
import torch

pytestmark = pytest.mark.gpu
SYN = ["--corpus-videos", "4", "--num-epochs", "2", "--batch-size", "8", "--nb-blocks", "1", "--d-model", "64", "--d-ff", "128",
       "--att-h", "4", "--vocab-size", "64", "--ft-sizes", "16", "8", "--warmup-steps", "20", "--report-interval", "1000", "--rand-seed", "7"]
FIXED = ["--num-epochs", "1", "--steps-per-epoch", "3", "--batch-size", "4", "--nb-blocks", "1", "--d-model", "64", "--d-ff", "128", "--att-h", "4",
         "--vocab-size", "64", "--ft-sizes", "16", "8", "--lens", "6", "12", "8", "7", "4", "--warmup-steps", "20", "--report-interval", "1000"]
LINE = re.compile(r"^epoch (\d+) gradient norm: mean (\S+) max (\S+) clipped (\d+) of (\d+) steps$", re.M)


@pytest.fixture(scope="module")
def runs():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    from mtn_amd import lib, train
    os.environ["MTN_EMBED_DETERMINISTIC"] = "1"          # the atomic-free embedding gradient: runs are bitwise reproducible
    lib.reload_env()
    out = {}
    for key, argv in (("plain", SYN), ("zero", SYN + ["--clip-grad-norm", "0"]), ("inf", SYN + ["--clip-grad-norm", "inf"]),
                      ("tight", SYN + ["--clip-grad-norm", "0.01"]), ("eager", SYN + ["--clip-grad-norm", "0.01", "--eager"]),
                      ("fixed", FIXED + ["--clip-grad-norm", "0.01"])):
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            means = train.main(argv)
        out[key] = dict(means=means, log=buf.getvalue())
    yield out
    del os.environ["MTN_EMBED_DETERMINISTIC"]
    lib.reload_env()


def _lines(log):
    return [(int(e), float(mean), float(mx), int(k), int(n)) for e, mean, mx, k, n in LINE.findall(log)]


def test_zero_is_the_run_without_the_flag(runs):
    assert runs["zero"]["means"] == runs["plain"]["means"] and all(math.isfinite(m) for m in runs["plain"]["means"])
    assert not _lines(runs["plain"]["log"]) and not _lines(runs["zero"]["log"])


def test_every_mode_logs_the_epoch_line(runs):
    for key, epochs in (("inf", 2), ("tight", 2), ("eager", 2), ("fixed", 1)):
        got = _lines(runs[key]["log"])
        assert [g[0] for g in got] == list(range(1, epochs + 1)), (key, runs[key]["log"])
        for _, mean, mx, k, n in got:
            assert 0 < mean <= mx and math.isfinite(mx) and n > 0 and 0 <= k <= n
        assert len({g[4] for g in got}) == 1                                   # the block is reset every epoch: n is the epoch's steps
    assert _lines(runs["fixed"]["log"])[0][4] == 3


def test_a_tight_cap_clips_every_step_and_inf_clips_none(runs):
    assert all(k == 0 for _, _, _, k, _ in _lines(runs["inf"]["log"]))
    for key in ("tight", "eager", "fixed"):
        assert all(k == n for _, _, _, k, n in _lines(runs[key]["log"])), key
    # measuring takes the separate optimiser pass (other gradient tilings than the fused step's): the same training up to fp32 rounding
    for a, b in zip(runs["inf"]["means"], runs["plain"]["means"]):
        assert abs(a - b) < 2e-2 * abs(b), (a, b)
    assert runs["tight"]["means"][-1] != runs["inf"]["means"][-1] and all(math.isfinite(m) for m in runs["tight"]["means"] + runs["eager"]["means"])
    assert _lines(runs["tight"]["log"])[0][1] == pytest.approx(_lines(runs["inf"]["log"])[0][1], rel=0.5)      # the norm is measured before the clip
