"""mtn_sched_mix (csrc/sched.hip) through ops.sched_mix against its numpy definition (tests/sched_refs.py), at B <= 4, T <= 8 and
V in {1, 3, 255, 257, 1030, 4099}: below and above one pass of 256 threads, no multiple of 4, past 4096; row strides above V with NaN in
the columns that are never read; row starts off the 16-byte grid (the scalar path).
  ARGMAX  mixed and stats bit for bit, planted ties, rows of -inf, a banned maximum, a row with nothing admitted, NaN rows, <pad> at t = 0.
  SAMPLE  the coin and the replaced set are exact; for EVERY replaced position the reported score lies within E_pick of the float64 score
          of the picked column, and that float64 score is no further below the float64 maximum than fp32 can confuse the two
          (E_pick + E_best <= 2 max E).  tests/test_sched_refs.py shows that in these cases this leaves one admissible column in at
          least 99 % of the rows: the float64 arg-max.
Every output sits between guard elements that must survive, stats accumulate on top of what they held, and the inputs are unchanged."""
import numpy as np
import pytest
import torch

from tests import sched_refs as R

pytestmark = pytest.mark.gpu
GUARD = 64                        # elements on each side of every buffer (a multiple of 4: 16-byte alignment survives)
PICKS = {R.ARGMAX: "argmax", R.SAMPLE: "sample"}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    from mtn_amd import lib
    lib.load()
    return torch.device("cuda:0")


def _guarded(dev, n, dtype, fill, sentinel):
    buf = torch.full((GUARD + n + GUARD,), sentinel, dtype=dtype, device=dev)
    view = buf[GUARD:GUARD + n]
    view.fill_(fill)
    return buf, view


def _intact(buf, n, sentinel):
    b = buf.cpu()
    return bool((b[:GUARD] == sentinel).all() and (b[GUARD + n:] == sentinel).all())


def _run(dev, z, trg, key, step, *, ldx=None, offset=0, stats0=(0, 0, 0), score=True, **kw):
    """One launch.  z (B * T, V) float32 numpy; the device copy has row stride ``ldx`` with NaN behind column V and starts ``offset`` floats
    behind a 16-byte boundary.  Returns (mixed, stats, pick_score) as numpy after checking guards and inputs."""
    from mtn_amd import ops
    rows, V = z.shape
    B, T = trg.shape
    ldx = V if ldx is None else ldx
    flat = torch.full((GUARD + offset + rows * ldx + GUARD,), float("nan"), dtype=torch.float32, device=dev)
    assert flat.data_ptr() % 16 == 0
    zt = flat[GUARD + offset:GUARD + offset + rows * ldx].view(rows, ldx)[:, :V]
    zt.copy_(torch.from_numpy(z))
    assert (zt.data_ptr() % 16 == 0) == (offset % 4 == 0)
    flat0 = flat.clone()
    trg_t, key_t = torch.from_numpy(trg).to(dev), torch.from_numpy(key).to(dev)
    state = torch.tensor([float(step), 1e-3, 0.1, 0.02, 0, 0, 0, 0], dtype=torch.float32, device=dev)
    state0 = state.clone()
    mbuf, mixed = _guarded(dev, B * T, torch.int64, -5, -777)
    sbuf, stats = _guarded(dev, 3, torch.int64, 0, -777)
    stats.copy_(torch.tensor(stats0, dtype=torch.int64))
    pbuf, pscore = _guarded(dev, B * T, torch.float32, 55.0, 123.0)
    out = ops.sched_mix(zt, trg_t, key_t, state, pad=kw["pad"], prob=kw["p_max"], start=kw["start"], ramp=kw["ramp"], pick=PICKS[kw["pick"]],
                        temperature=1.0 / float(kw["inv_t"]), seed=kw["seed"], banned=kw["banned"], out=mixed.view(B, T), stats=stats,
                        pick_score=pscore.view(B, T) if score else None)
    torch.cuda.synchronize()
    assert out.data_ptr() == mixed.data_ptr()
    assert _intact(mbuf, B * T, -777) and _intact(sbuf, 3, -777) and _intact(pbuf, B * T, 123.0)
    assert torch.equal(trg_t.cpu(), torch.from_numpy(trg)) and torch.equal(key_t.cpu(), torch.from_numpy(key)) and torch.equal(state, state0)
    assert torch.equal(flat.view(torch.int32), flat0.view(torch.int32))
    if not score:
        assert bool((pscore == 55.0).all())
    return mixed.view(B, T).cpu().numpy(), stats.cpu().numpy() - np.asarray(stats0), pscore.view(B, T).cpu().numpy()


def _inv_t_roundtrip(case):
    """ops.sched_mix takes a temperature and hands the kernel fp32(1 / temperature): the cases' inv_t must survive that."""
    return np.float32(1.0 / (1.0 / float(case.inv_t))) == case.inv_t


@pytest.mark.parametrize("case", [c for c in R.CASES if c.pick == R.ARGMAX], ids=lambda c: c.name)
def test_argmax_is_bit_exact(dev, case):
    z, trg, key = case.data()
    ref = R.mix(z, trg, key, case.step, **case.kw())
    mixed, stats, score = _run(dev, z, trg, key, case.step, ldx=case.ldx, offset=case.offset, stats0=(5, 7, 9), **case.kw())
    print(case.name, "p", ref["p"], "stats", stats, "ref", ref["stats"])
    assert np.array_equal(mixed, ref["mixed"])
    assert np.array_equal(stats, ref["stats"])
    assert np.array_equal(np.isnan(score), ~ref["replaced"])
    assert np.array_equal(score[ref["replaced"]].astype(np.float64), ref["score"][ref["replaced"]])      # the winning logit itself


@pytest.mark.parametrize("case", [c for c in R.CASES if c.pick == R.SAMPLE], ids=lambda c: c.name)
def test_sample_picks_the_float64_gumbel_maximum_within_the_bound(dev, case):
    assert _inv_t_roundtrip(case)
    z, trg, key = case.data()
    ref = R.mix(z, trg, key, case.step, **case.kw())
    mixed, stats, score = _run(dev, z, trg, key, case.step, ldx=case.ldx, offset=case.offset, **case.kw())
    ok = R.admitted(case.V, case.pad, case.banned)
    replaced = ~np.isnan(score)
    assert np.array_equal(replaced, ref["replaced"])                      # the coin, and which rows yield a pick, are exact
    assert np.array_equal(mixed[~replaced], trg[~replaced])
    worst_score = worst_gap = 0.0
    for b, t in np.argwhere(replaced):
        c, s, E = int(mixed[b, t]), ref["s"][b, t], ref["E"][b, t]
        assert 0 <= c < case.V and ok[c]
        best = int(np.nonzero(ok)[0][np.argmax(s[ok])])
        if np.isinf(s[c]) or np.isinf(s[best]):
            assert float(score[b, t]) == s[c] and s[c] == s[best]
            continue
        worst_score = max(worst_score, abs(float(score[b, t]) - s[c]) / E[c])
        worst_gap = max(worst_gap, (s[best] - s[c]) / (E[c] + E[best]))
        assert abs(float(score[b, t]) - s[c]) <= E[c], (b, t, c, float(score[b, t]), s[c], E[c])
        assert s[c] >= s[best] - (E[c] + E[best]), (b, t, c, best, s[c], s[best], E[c], E[best])
    print(case.name, "replaced", int(replaced.sum()), "worst |score - s64| / E", worst_score, "worst gap / (E + E)", worst_gap,
          "picks equal to the float64 arg-max", int((mixed[replaced] == ref["mixed"][replaced]).sum()))
    assert np.array_equal(stats, [ref["stats"][0], replaced.sum(), (replaced & (mixed != trg)).sum()])


@pytest.mark.parametrize("pick", [R.ARGMAX, R.SAMPLE])
def test_p_zero_keeps_every_token_and_never_needs_the_logits(dev, pick):
    """p = 0 two ways (p_max = 0; start beyond the step) over a logits buffer that holds nothing but NaN."""
    case = R.Case("p0", 4, 8, 257, pick, ldx=260)
    z, trg, key = case.data()
    z[:] = np.nan
    for kw in (dict(p_max=0.0), dict(p_max=1.0, start=case.step + 1), dict(p_max=1.0, start=case.step + 1, ramp=5)):
        args = dict(case.kw(), **kw)
        mixed, stats, score = _run(dev, z, trg, key, case.step, ldx=case.ldx, **args)
        eligible = int(((np.arange(case.T)[None, :] >= 1) & (trg != case.pad)).sum())
        assert np.array_equal(mixed, trg) and np.isnan(score).all()
        assert np.array_equal(stats, [eligible, 0, 0])


@pytest.mark.parametrize("pick", [R.ARGMAX, R.SAMPLE])
def test_p_one_replaces_every_eligible_position(dev, pick):
    case = R.Case("p1", 4, 8, 1030, pick, ldx=1032, p_max=1.0)
    z, trg, key = case.data()
    mixed, stats, score = _run(dev, z, trg, key, case.step, ldx=case.ldx, score=False, **case.kw())
    eligible = (np.arange(case.T)[None, :] >= 1) & (trg != case.pad)
    assert stats[0] == stats[1] == eligible.sum() > 0
    assert np.array_equal(mixed[~eligible], trg[~eligible])
    assert not np.isin(mixed[eligible], (case.pad,) + case.banned).any()
    if pick == R.ARGMAX:
        assert np.array_equal(mixed, R.mix(z, trg, key, case.step, **case.kw())["mixed"])


def test_the_step_drives_the_draws(dev):
    """Another state[0], other coins and draws; the same state, the same bytes."""
    case = R.Case("steps", 4, 8, 4099, R.SAMPLE, ldx=4100, p_max=0.5, seed=99)
    z, trg, key = case.data()
    a = _run(dev, z, trg, key, 10, ldx=case.ldx, **case.kw())
    b = _run(dev, z, trg, key, 10, ldx=case.ldx, **case.kw())
    c = _run(dev, z, trg, key, 11, ldx=case.ldx, **case.kw())
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2].view(np.int32), b[2].view(np.int32))
    assert not np.array_equal(np.isnan(a[2]), np.isnan(c[2]))             # other coins
    for out, step in ((a, 10), (c, 11)):
        assert np.array_equal(~np.isnan(out[2]), R.mix(z, trg, key, step, **case.kw())["replaced"])
    # the ramp reads the step too: p = 0.5 * min(1, (step - 8) / 4)
    kw = dict(case.kw(), start=8, ramp=4)
    for step in (8, 9, 11, 12, 40):
        out = _run(dev, z, trg, key, step, ldx=case.ldx, **kw)
        assert np.array_equal(~np.isnan(out[2]), R.mix(z, trg, key, step, **kw)["replaced"]), step


def test_a_single_position_and_an_empty_batch(dev):
    from mtn_amd import ops
    case = R.Case("one", 1, 1, 257, R.ARGMAX)
    z, trg, key = case.data()
    trg[0, 0] = 7
    mixed, stats, score = _run(dev, z, trg, key, 0, **case.kw())
    assert mixed[0, 0] == 7 and np.array_equal(stats, [0, 0, 0]) and np.isnan(score).all()      # t = 0 is never eligible
    out = ops.sched_mix(torch.zeros(0, 16, device=dev), torch.zeros(0, 5, dtype=torch.int64, device=dev),
                        torch.zeros(0, dtype=torch.int64, device=dev), torch.zeros(8, device=dev), pad=1, prob=0.5)
    assert tuple(out.shape) == (0, 5)


def test_the_wrapper_refuses_what_the_kernel_would_misread(dev):
    from mtn_amd import ops
    z, trg, key, st = torch.zeros(8, 16, device=dev), torch.zeros(2, 4, dtype=torch.int64, device=dev), \
        torch.zeros(2, dtype=torch.int64, device=dev), torch.zeros(8, device=dev)
    for bad in (dict(logits=z[:6]), dict(logits=z.double()), dict(logits=z[:, ::2]), dict(trg=trg.int()), dict(key=key[:1]),
                dict(state=st.double()), dict(pick="greedy"), dict(temperature=0.0), dict(banned=(2, 3, 4, 5, 6)), dict(out=trg.clone()[:, :2]),
                dict(stats=torch.zeros(3, device=dev)), dict(pick_score=torch.zeros(2, 4, dtype=torch.float64, device=dev))):
        kw = dict(logits=z, trg=trg, key=key, state=st, pad=1, prob=0.5)
        kw.update(bad)
        a = [kw.pop(k) for k in ("logits", "trg", "key", "state")]
        with pytest.raises(ValueError):
            ops.sched_mix(*a, **kw)
    from mtn_amd.lib import MtnHipError
    with pytest.raises(MtnHipError, match="mtn_sched_mix"):
        ops.sched_mix(z, trg, key, st, pad=1, prob=0.5, out=trg)            # the gold ids must survive
    with pytest.raises(MtnHipError, match="mtn_sched_mix"):
        ops.sched_mix(z, trg, key, st, pad=1, prob=1.5)
