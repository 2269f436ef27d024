"""Knowledge distillation inside the training step (mtn_amd.train_step.TrainStep(teacher=...)) on the small configurations of
tests/test_model_gpu.py, with its helpers and its bars:
  (a) a teacher at alpha = 0 leaves the captured step what it was, bit for bit, and the student's part of the launch census unchanged;
  (b) a different teacher at alpha = 0.5, T = 2: loss and every parameter gradient against the CPU oracle (oracle forward of student and
      teacher, the composed loss of tests/distill_refs.py's definition — F.kl_div on log_softmax(z / T), softmax(q / T) over the rows whose
      target is not <pad> — and autograd), at the bars test_model_loss_and_grads_match_reference_golden holds its gradients to;
  (c) a two-member Ensemble teacher with weights 2:1, both modes, held as (b);
  (d) eager and captured steps give the same loss bits;
  (e) the layer-segmented schedule (one-rank gloo group, child process) gives the monolithic step's first loss within 1e-5 relative."""
import os
import socket
import sys

import pytest
import torch
import torch.nn.functional as F

from oracle import fixtures as fx
from oracle.mtn_oracle import label_smoothing_kl
from tests.step_helpers import _census, _student, deterministic_embed  # noqa: F401  (fixture)
from tests.test_model_gpu import build_model, dev_batch, raw_batch
from tests.util import DTYPES, TOL, relmax

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["small_shared", "cfg1_query"]


def _config(name):
    """The golden configuration with its vocabulary rounded up to a multiple of 8 (60 -> 64, 100 -> 104): what the fused HIP loss head
    takes (tests/test_model_gpu.py::test_fused_loss_head_matches_composed_loss does the same) — below it the step composes the loss
    from PyTorch ops and csrc/losshead.hip would not run."""
    c = fx.GOLDEN_CONFIGS[name]
    c = dict(c, vocab=-(-c["vocab"] // 8) * 8)
    assert c["vocab"] % 8 == 0
    return c


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


def _teacher(c, dtype, dev, seed):
    return build_model(c, dtype, dev, seed=seed).eval()


# ------------------------------------------------------------------------------------------ (a)
@pytest.mark.parametrize("name", NAMES)
def test_teacher_at_alpha_zero_leaves_the_step_bitwise(dev, name, deterministic_embed):
    from mtn_amd.train_step import TrainStep, teacher_rows
    c = _config(name)
    b = dev_batch(raw_batch(c), dev)

    def run(teacher):
        model = _student(c, torch.bfloat16, dev, 0.1)
        ts = TrainStep(model, b, c["vocab"], pad=fx.PAD, warmup=10, teacher=teacher, distill_alpha=0.0, distill_temperature=2.0)
        losses = [ts().clone() for _ in range(3)]
        torch.cuda.synchronize()
        return losses, model._flat.clone(), ts

    teacher = _teacher(c, torch.bfloat16, dev, 1)
    plain_l, plain_p, _ = run(None)
    dist_l, dist_p, ts = run(teacher)
    for a, d in zip(plain_l, dist_l):
        assert torch.equal(a.view(torch.int32), d.view(torch.int32)), (float(a), float(d))
    assert torch.equal(plain_p.view(torch.int32), dist_p.view(torch.int32))
    assert plain_l[0].item() != plain_l[2].item()                        # the steps did train
    assert float(ts.last_kd) == 0.0

    # the launch census: the distilled step is the teacher pass followed by exactly the undistilled step's launches
    def eager(teacher):
        model = _student(c, torch.bfloat16, dev, 0.1)
        ts = TrainStep(model, b, c["vocab"], pad=fx.PAD, warmup=10, teacher=teacher, distill_alpha=0.0, use_graph=False)
        step = ts._step_fused if ts._fused() else ts._fwd_bwd
        step()                                                           # (lazy set-up outside the census)
        return _census(step)

    plain_c, plain_f = eager(None)
    dist_c, dist_f = eager(teacher)
    teach_c, teach_f = _census(lambda: teacher_rows(teacher, b))
    assert len(teach_c) > 0 and len(plain_c) > 0
    assert dist_c == teach_c + plain_c
    assert dist_f == tuple(t + p for t, p in zip(teach_f, plain_f))


# ------------------------------------------------------------------------------------------ (b), (c)
def _oracle_reference(c, raw, teacher_seeds, weights, mode, alpha, T):
    """(loss, {parameter name: gradient}) of the distilled loss on the CPU oracle."""
    ob = fx.oracle_batch(raw)
    student, _ = fx.oracle_from_config(c, seed=0, requires_grad=True)
    out, ae = student.forward(ob)
    with torch.no_grad():
        logps = []
        for s in teacher_seeds:
            t, _ = fx.oracle_from_config(c, seed=s)
            logps.append(t.generator(t.forward(ob)[0]))
        w = torch.tensor(weights, dtype=logps[0].dtype) / sum(weights)
        stack = torch.stack(logps)
        if mode == "prob":
            q = torch.logsumexp(stack + w.log().view(-1, 1, 1, 1), dim=0)
        else:
            q = torch.log_softmax((stack * w.view(-1, 1, 1, 1)).sum(0), dim=-1)
    V = q.size(-1)
    logp = student.generator(out).reshape(-1, V)
    y = ob.trg_y.reshape(-1)
    norm = ob.ntokens.float()
    plain = student.loss(ob, out, ae)
    hard = label_smoothing_kl(logp, y, fx.PAD, 0.1) / norm
    kd = F.kl_div(torch.log_softmax(logp / T, dim=-1), torch.softmax(q.reshape(-1, V) / T, dim=-1), reduction="none").sum(-1)
    kd = torch.where(y != fx.PAD, kd, torch.zeros_like(kd)).sum()
    total = plain - alpha * hard + alpha * T * T * kd / norm
    total.backward()
    return float(total.detach()), {k: v.grad for k, v in student.p.items() if v.grad is not None}, float(kd.detach() / norm)


def _check_against_oracle(dev, name, dtype, teacher_seeds, weights, mode):
    from mtn_amd.decode import Ensemble
    from mtn_amd.train_step import TrainStep
    alpha, T = 0.5, 2.0
    c = _config(name)
    raw = raw_batch(c)
    ref_loss, ref_grads, ref_kd = _oracle_reference(c, raw, teacher_seeds, weights, mode, alpha, T)
    members = [_teacher(c, dtype, dev, s) for s in teacher_seeds]
    teacher = members[0] if len(members) == 1 else Ensemble(members, weights, mode)
    model = _student(c, dtype, dev, 0.0)
    ts = TrainStep(model, dev_batch(raw, dev), c["vocab"], pad=fx.PAD, warmup=10, use_graph=False, fuse_optimizer=False, teacher=teacher,
                   distill_alpha=alpha, distill_temperature=T)
    out, ae_out = model.forward(ts.batch)                               # the loss is the fused HIP head's, not the composed fallback's
    probe = ts._loss_of(out, ae_out, ts._teacher_pass())
    assert probe.grad_fn is not None and "GeneratorLossFn" in type(probe.grad_fn).__name__
    del probe, out, ae_out
    loss = ts._fwd_bwd()
    torch.cuda.synchronize()
    tol = TOL[dtype]
    print(f"{name} {dtype} {mode}: loss {float(loss):.6f} (oracle {ref_loss:.6f})  kd/token {float(ts.last_kd):.6f} (oracle {ref_kd:.6f})")
    assert abs(float(loss) - ref_loss) < tol * max(1.0, abs(ref_loss))
    assert abs(float(ts.last_kd) - ref_kd) < tol * max(1.0, abs(ref_kd))
    assert ref_kd > 1e-3                                                # the teacher does differ from the student
    gtol = 3e-3 if dtype == torch.float32 else 0.25                     # test_model_loss_and_grads_match_reference_golden's bars
    params = dict(model.named_parameters())
    worst, dot, n1, n2 = 0.0, 0.0, 0.0, 0.0
    checked = 0
    for k, ref in ref_grads.items():
        if k not in params:
            continue
        gr = params[k].grad
        assert gr is not None, k
        n, gn = float(ref.double().norm()), float(gr.double().norm())
        if n < 1e-6:
            assert gn < (1e-5 if dtype == torch.float32 else 1e-3), (k, gn)
            continue
        e = max(relmax(gr, ref), abs(gn - n) / n)
        dot += float((gr.double().cpu() * ref.double()).sum()); n1 += gn * gn; n2 += n * n
        worst = max(worst, e)
        checked += 1
        assert e < gtol, (k, e)
    cos = dot / (n1 ** 0.5 * n2 ** 0.5)
    print(f"worst grad rel err {worst:.2e} over {checked} tensors, cosine {cos:.7f}")
    assert checked > 20
    assert cos > (0.999999 if dtype == torch.float32 else 0.9995), cos


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", NAMES)
def test_distilled_loss_and_gradients_match_the_oracle(dev, name, dtype):
    _check_against_oracle(dev, name, dtype, [1], [1.0], "prob")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", ["prob", "logprob"])
def test_ensemble_teacher_matches_the_oracle(dev, mode, dtype):
    _check_against_oracle(dev, "small_shared", dtype, [1, 2], [2.0, 1.0], mode)


def test_teacher_argument_checks(dev):
    from mtn_amd.train_step import TrainStep
    c = _config("cfg1_query")
    b = dev_batch(raw_batch(c), dev)
    model = _student(c, torch.bfloat16, dev, 0.0)
    good = _teacher(c, torch.bfloat16, dev, 1)
    other = dict(c, vocab=c["vocab"] + 8)
    for kw in (dict(teacher="a path"), dict(teacher=model), dict(teacher=good, distill_alpha=1.5), dict(teacher=good, distill_temperature=0.0),
               dict(teacher=build_model(other, torch.bfloat16, dev, seed=1).eval()), dict(teacher=build_model(c, torch.bfloat16, torch.device("cpu"), seed=1))):
        with pytest.raises(ValueError):
            TrainStep(model, b, c["vocab"], pad=fx.PAD, **kw)


# ------------------------------------------------------------------------------------------ (d)
def test_eager_and_captured_steps_give_the_same_loss_bits(dev, deterministic_embed):
    from mtn_amd.train_step import TrainStep
    c = _config("small_shared")
    b = dev_batch(raw_batch(c), dev)
    teacher = _teacher(c, torch.bfloat16, dev, 1)
    runs = []
    for use_graph in (False, True):
        model = _student(c, torch.bfloat16, dev, 0.0)
        ts = TrainStep(model, b, c["vocab"], pad=fx.PAD, warmup=10, use_graph=use_graph, teacher=teacher, distill_alpha=0.5, distill_temperature=2.0)
        runs.append([(ts().clone(), ts.last_kd.clone()) for _ in range(3)])
    torch.cuda.synchronize()
    for (le, ke), (lg, kg) in zip(*runs):
        assert torch.equal(le.view(torch.int32), lg.view(torch.int32)), (float(le), float(lg))
        assert torch.equal(ke.view(torch.int32), kg.view(torch.int32))
    assert float(runs[0][0][1]) > 0 and float(runs[0][2][0]) != float(runs[0][0][0])


# ------------------------------------------------------------------------------------------ (e)
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _segmented_worker(rank, port, out_dir):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    import torch.distributed as dist
    from mtn_amd import dp
    from mtn_amd.train_step import TrainStep
    dev = torch.device("cuda:0")
    dist.init_process_group("gloo", rank=0, world_size=1)
    c = _config("cfg1_query")
    b = dev_batch(raw_batch(c), dev)
    teacher = _teacher(c, torch.bfloat16, dev, 1)
    out = {}
    for key in ("segmented", "monolithic"):
        model = _student(c, torch.bfloat16, dev, 0.0)
        sync = dp.GradSync(lambda: model.flat_buffers()[2]) if key == "segmented" else None
        ts = TrainStep(model, b, c["vocab"], pad=fx.PAD, warmup=10, grad_sync=sync, use_graph=True, overlap=True if sync is not None else None,
                       teacher=teacher, distill_alpha=0.5, distill_temperature=2.0)
        out[key] = (float(ts()), float(ts.last_kd))
        out[key + "_overlap"] = bool(ts.overlap)
    torch.cuda.synchronize()
    torch.save(out, os.path.join(out_dir, "losses.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_segmented_schedule_gives_the_monolithic_loss(tmp_path):
    import torch.multiprocessing as mp
    assert torch.cuda.is_available()
    mp.start_processes(_segmented_worker, args=(_free_port(), str(tmp_path)), nprocs=1, join=True, start_method="spawn")
    r = torch.load(tmp_path / "losses.pt")
    assert r["segmented_overlap"] and not r["monolithic_overlap"]
    (ls, ks), (lm, km) = r["segmented"], r["monolithic"]
    print(f"segmented {ls:.8f} / kd {ks:.8f}   monolithic {lm:.8f} / kd {km:.8f}")
    assert abs(ls - lm) <= 1e-5 * abs(lm)
    assert abs(ks - km) <= 1e-5 * abs(km) and km > 0
