"""`python train.py --ema-decay D` (mtn_amd.train) on the GPU, end to end, on a synthetic corpus: the averaged checkpoints are written next to
the raw ones in the same schema, validation runs a second time under the averaged weights, the raw checkpoints are those of the run
without the flag, generate.py's loader takes an averaged checkpoint, and --resume carries the average on."""
import math
import os
import re

import pytest
import torch

pytestmark = pytest.mark.gpu
SYN = ["--corpus-videos", "4", "--valid-videos", "2", "--num-epochs", "2", "--batch-size", "8", "--nb-blocks", "1", "--d-model", "64", "--d-ff", "128",
       "--att-h", "4", "--vocab-size", "64", "--ft-sizes", "16", "8", "--warmup-steps", "20", "--report-interval", "1000", "--rand-seed", "7"]
EMA_LINE = re.compile(r"^epoch: (\d+) validation loss \(averaged weights\): (\S+)$", re.M)
RAW_LINE = re.compile(r"^epoch: (\d+) validation loss: (\S+)$", re.M)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """One run with --ema-decay and one without, same seed, with their captured output."""
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    import contextlib
    import io
    from mtn_amd import lib, train
    os.environ["MTN_EMBED_DETERMINISTIC"] = "1"          # the atomic-free embedding gradient: runs are bitwise reproducible
    lib.reload_env()
    tmp = tmp_path_factory.mktemp("train_ema")
    out = {}
    for key, extra in (("ema", ["--ema-decay", "0.99"]), ("plain", [])):
        (tmp / key).mkdir()                               # (synthetic runs write no conf, and so create no directory)
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            means = train.main(SYN + ["--model", str(tmp / key / "m")] + extra)
        out[key] = dict(dir=tmp / key, means=means, log=buf.getvalue())
    yield out
    del os.environ["MTN_EMBED_DETERMINISTIC"]
    lib.reload_env()


def _load(path):
    return torch.load(str(path), map_location="cpu", weights_only=True)


def test_averaged_checkpoints_are_written_in_the_raw_schema(runs):
    d = runs["ema"]["dir"]
    raw = _load(d / "m_1.pth.tar")
    for name in ("m_1_ema", "m_2_ema", "m_best_ema"):
        sd = _load(d / (name + ".pth.tar"))
        assert list(sd) == list(raw), name
        for k, v in raw.items():
            assert sd[k].shape == v.shape and sd[k].dtype == v.dtype, (name, k)
            assert bool(torch.isfinite(sd[k].float()).all()), (name, k)
    ema2, raw2 = _load(d / "m_2_ema.pth.tar"), _load(d / "m_2.pth.tar")
    differing = sum(int(not torch.equal(ema2[k], raw2[k])) for k in raw2 if raw2[k].is_floating_point())
    assert differing > len(raw2) // 2                                          # the average is not the raw weights
    opt = torch.load(str(d / "m_2_opt.pth.tar"), map_location="cpu")
    assert opt["optimizer"]["ema_decay"] == 0.99 and set(opt["optimizer"]["ema"]) == set(opt["optimizer"]["exp_avg"])
    # the file's average is the optimiser's: the averaged checkpoint holds the same tensors under the model's keys
    for k, v in opt["optimizer"]["ema"].items():
        assert torch.equal(v, ema2[k]), k
    assert not (runs["plain"]["dir"] / "m_1_ema.pth.tar").exists() and not (runs["plain"]["dir"] / "m_best_ema.pth.tar").exists()


def test_the_log_carries_the_averaged_validation(runs):
    log = runs["ema"]["log"]
    ema, raw = EMA_LINE.findall(log), RAW_LINE.findall(log)
    assert [e for e, _ in ema] == ["1", "2"] and [e for e, _ in raw] == ["1", "2"]
    assert all(math.isfinite(float(v)) and float(v) > 0 for _, v in ema)
    assert [v for _, v in ema] != [v for _, v in raw]
    assert not EMA_LINE.search(runs["plain"]["log"])
    assert RAW_LINE.findall(runs["plain"]["log"]) == raw                       # the raw weights' validation is what it is without the flag


def test_the_raw_checkpoints_are_those_of_the_run_without_the_flag(runs):
    assert runs["ema"]["means"] == runs["plain"]["means"]
    for name in ("m_1", "m_2", "m_best"):
        a, b = _load(runs["ema"]["dir"] / (name + ".pth.tar")), _load(runs["plain"]["dir"] / (name + ".pth.tar"))
        assert list(a) == list(b)
        for k in a:
            assert torch.equal(a[k], b[k]), (name, k)
    a = torch.load(str(runs["ema"]["dir"] / "m_2_opt.pth.tar"), map_location="cpu")["optimizer"]
    b = torch.load(str(runs["plain"]["dir"] / "m_2_opt.pth.tar"), map_location="cpu")["optimizer"]
    assert "ema" not in b and torch.equal(a["schedule"], b["schedule"])
    for k in b["exp_avg"]:
        assert torch.equal(a["exp_avg"][k], b["exp_avg"][k]) and torch.equal(a["exp_avg_sq"][k], b["exp_avg_sq"][k]), k


def test_generate_loads_an_averaged_checkpoint(runs):
    from mtn_amd import generate as gen
    from mtn_amd import train
    from mtn_amd.synthetic import synthetic_batch
    dev = torch.device("cuda:0")
    args = train.parse(SYN)
    vocab = {"w%d" % i: i for i in range(64)}
    sd = gen.load_state_dict(str(runs["ema"]["dir"] / "m_best_ema") + ".pth.tar")
    model = gen.build_model(vocab, args, args.ft_sizes, sd, "bf16", dev)
    b = synthetic_batch(64, 4, 8, 16, 12, 8, [10, 10], args.ft_sizes, device=dev, seed=3)
    with torch.no_grad():
        out, _ = model.forward(b)
    assert out.shape[0] == 4 and bool(torch.isfinite(out.float()).all())
    for k, p in model.named_parameters():
        assert torch.equal(p.detach().cpu(), sd[k]), k


@pytest.mark.parametrize("mode", ["eager", "fixed-batch"])
def test_the_other_training_modes_keep_the_average_too(runs, tmp_path, capsys, mode):
    """--eager (one eager step per batch) and the fixed synthetic batch: the averaged checkpoint is written and is not the raw one."""
    from mtn_amd import train
    if mode == "eager":
        argv = SYN + ["--eager"]
    else:
        assert SYN[:4] == ["--corpus-videos", "4", "--valid-videos", "2"]
        argv = SYN[4:] + ["--steps-per-epoch", "5", "--lens", "8", "16", "12", "8", "10"]
    capsys.readouterr()
    train.main(argv + ["--model", str(tmp_path / "m"), "--ema-decay", "0.99"])
    out = capsys.readouterr().out
    assert bool(EMA_LINE.search(out)) == (mode == "eager")                     # (the fixed batch has no validation)
    for epoch in (1, 2):
        raw, ema = _load(tmp_path / ("m_%d.pth.tar" % epoch)), _load(tmp_path / ("m_%d_ema.pth.tar" % epoch))
        assert list(raw) == list(ema)
        differing = sum(int(not torch.equal(ema[k], raw[k])) for k in raw if raw[k].is_floating_point())
        assert differing > len(raw) // 2 and all(bool(torch.isfinite(v.float()).all()) for v in ema.values())
    if mode == "eager":                                                       # the eager loop trains what the graphed one trains
        graphed = _load(runs["ema"]["dir"] / "m_2_ema.pth.tar")
        assert list(graphed) == list(ema)


def test_resume_carries_the_average_on(runs, capsys):
    from mtn_amd import train
    d = runs["ema"]["dir"]
    capsys.readouterr()
    one_epoch = list(SYN)
    one_epoch[SYN.index("--num-epochs") + 1] = "1"
    means = train.main(one_epoch + ["--model", str(d / "r"), "--ema-decay", "0.99", "--resume", str(d / "m_1")])
    out = capsys.readouterr().out
    assert len(means) == 1 and math.isfinite(means[0])
    assert EMA_LINE.search(out)
    before, after = torch.load(str(d / "m_1_opt.pth.tar"), map_location="cpu"), torch.load(str(d / "r_1_opt.pth.tar"), map_location="cpu")
    assert int(after["step"]) > int(before["step"]) > 0                        # it continued where m_1 stopped
    raw, ema = _load(d / "r_1.pth.tar"), _load(d / "r_1_ema.pth.tar")
    differing = sum(int(not torch.equal(ema[k], raw[k])) for k in raw if raw[k].is_floating_point())
    assert differing > len(raw) // 2
    # the average went on from the file's: the largest matrix's moved, and it is not the resumed masters'
    k = max((k for k in before["optimizer"]["ema"] if before["optimizer"]["ema"][k].dim() == 2), key=lambda k: before["optimizer"]["ema"][k].numel())
    assert not torch.equal(after["optimizer"]["ema"][k], before["optimizer"]["ema"][k])
