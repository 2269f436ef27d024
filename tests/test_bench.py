"""bench.py's contract: a plain run measures the headline figure only (everything else is behind --full), --steps is the number
of timed steps, and --dump-outputs writes what the last timed step computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONTRACT = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "dtype")


def _parse(*argv):
    sys.path.insert(0, ROOT)
    import bench
    old = sys.argv
    sys.argv = ["bench.py", *argv]
    try:
        return bench.parse()
    finally:
        sys.argv = old


def test_bench_options():
    a = _parse("--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.full, a.steps, a.warmup, a.dump_outputs) == (False, 7, 2, None)
    assert _parse("--full").full
    assert _parse("--full-record", "record.json").full          # the verbose record is the full one
    assert _parse("--dump-outputs", "out").dump_outputs == "out"


@pytest.mark.gpu
def test_plain_bench_run_and_dumped_outputs(tmp_path):
    out = tmp_path / "dump"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(out)],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    line = json.loads(p.stdout.strip().splitlines()[-1])
    for k in CONTRACT:
        assert k in line, k
    assert line["steps"] == 3 and line["warmup"] == 1 and line["higher_is_better"] is True and line["dtype"] == "bf16"
    assert line["ms_per_step"] > 0 and abs(line["value"] - line["config"]["batch_per_gpu"] * 1e3 / line["ms_per_step"]) < 0.01 * line["value"]
    assert "roofline" not in line and "cpu_baseline" not in line and "window_ms_per_step" not in line["config"], "a plain run is headline only"
    names = sorted(f for f in os.listdir(out))
    assert names == ["adam_m.npy", "adam_v.npy", "loss.npy", "params.npy"], names
    assert sum(os.path.getsize(out / f) for f in names) <= 64 << 20
    arrays = {f[:-4]: np.load(out / f) for f in names}
    for k, a in arrays.items():
        assert a.dtype == np.float32 and np.isfinite(a).all(), k
    assert abs(float(arrays["loss"][0]) - line["config"]["normalised_loss_last_step"]) < 1e-3
    assert arrays["params"].shape == arrays["adam_m"].shape == arrays["adam_v"].shape
    assert (arrays["adam_v"] > 0).mean() > 0.5             # four steps of Adam: most sampled weights have a gradient history
