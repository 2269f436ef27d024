"""csrc/contrastive.hip against its numpy definition (tests/contrastive_refs.py), without a model: every case of R.GPU_CASES is a chain of
mtn_contrastive_advance launches on synthetic states and heads, compared after EVERY launch with the reference state machine — tokens,
pos, step, done, the token and rank logs exactly, cand_logp and the log-probability log bit for bit, the penalty log within the cosine
bound.  tests/test_contrastive_refs.py shows that every scored step of these inputs is decided by at least four error bounds, so an exact
comparison of the choices is a fair one.  Every buffer sits between canary words, the padding of a strided hidden tensor is NaN (a read
outside a state poisons a score), and every launch is run twice from the same state: the same bytes come out."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import contrastive_refs as R

pytestmark = pytest.mark.gpu
GUARD = 4                                  # canary words on either side of every buffer
CANARY = {np.dtype(np.float32): np.float32(-12345.678), np.dtype(np.int32): np.int32(0x5A5A5A5A), np.dtype(np.int64): np.int64(0x5A5A5A5A5A5A5A5A)}


@functools.lru_cache(maxsize=None)
def _reference(name):
    c = next(c for c in R.GPU_CASES if c["name"] == name)
    return c, R.make_case(c), R.run_case(c)


class Guarded:
    """A device buffer between canary words: .t is the payload, a view of the guarded allocation."""

    def __init__(self, host, dev, guard=GUARD):
        host = np.ascontiguousarray(host)
        full = np.full(host.size + 2 * guard, CANARY[host.dtype], dtype=host.dtype)
        full[guard:guard + host.size] = host.ravel()
        self.full, self.guard, self.shape = torch.from_numpy(full).to(dev), guard, host.shape
        self.t = self.full[guard:guard + host.size].view(*host.shape)

    def set(self, host):
        self.t.copy_(torch.from_numpy(np.ascontiguousarray(host)))

    def get(self):
        return self.t.cpu().numpy()

    def intact(self):
        f, g = self.full.cpu().numpy(), self.guard
        return bool((f[:g].view(np.uint8) == f[-g:].view(np.uint8)).all() and (f[:g] == CANARY[f.dtype]).all())


def _strided_hidden(hidden, c, dev):
    """hidden (W, L, d) laid out with the case's padded strides (NaN in the padding) behind a guard that keeps or breaks 16-byte alignment."""
    W, L, d = hidden.shape
    ps = d + c["pos_pad"]
    rs = L * ps + c["row_pad"]
    guard = 5 if c["name"].startswith("d20") else GUARD             # d = 20 with an odd base: the scalar path whatever the strides
    body = np.full(W * rs, np.nan, dtype=np.float32)
    for r in range(W):
        for j in range(L):
            body[r * rs + j * ps:r * rs + j * ps + d] = hidden[r, j]
    g = Guarded(body, dev, guard)
    return g, rs, ps


def _args(lib, c, eos, bufs, hid, rs, ps, top):
    a = lib.ContrastiveArgs()
    a.dialogues, a.k, a.L, a.d, a.k_top, a.alpha = c["D"], c["k"], c["L"], c["d"], c["k_top"], c["alpha"]
    a.eos, a.min_len, a.n_banned = eos, c["min_len"], len(c["banned"])
    for i, b in enumerate(c["banned"]):
        a.banned[i] = b
    a.hidden, a.row_stride, a.pos_stride, a.top = hid.t.data_ptr(), rs, ps, top.t.data_ptr()
    for name in ("tokens", "pos", "cand_logp", "step", "done", "log_tok", "log_logp", "log_pen", "log_rank"):
        setattr(a, name, bufs[name].t.data_ptr())
    return a


STATE = ("tokens", "pos", "cand_logp", "step", "done", "log_tok", "log_logp", "log_pen", "log_rank")


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint8)


@pytest.mark.parametrize("name", [c["name"] for c in R.GPU_CASES])
def test_launches_follow_the_reference_state_machine(name):
    from mtn_amd import lib
    c, (st, launches, eos), states = _reference(name)
    dev = torch.device("cuda", torch.cuda.current_device())
    h = lib.load()
    z = lambda dt: np.zeros((c["L"], c["D"]), dtype=dt)
    bufs = {"tokens": Guarded(st.tokens, dev), "pos": Guarded(np.array([st.pos], dtype=np.int64), dev), "cand_logp": Guarded(st.cand_logp, dev),
            "step": Guarded(st.step, dev), "done": Guarded(st.done, dev), "log_tok": Guarded(z(np.int32), dev), "log_logp": Guarded(z(np.float32), dev),
            "log_pen": Guarded(z(np.float32), dev), "log_rank": Guarded(z(np.int32), dev)}
    for i, (hidden, top) in enumerate(launches):
        hid, rs, ps = _strided_hidden(hidden, c, dev)
        tp = Guarded(top, dev)
        a = _args(lib, c, eos, bufs, hid, rs, ps, tp)
        before = {n: bufs[n].get().copy() for n in STATE}
        lib.check(h.mtn_contrastive_advance(C.byref(a), lib.stream_ptr()))
        torch.cuda.synchronize()
        got = {n: bufs[n].get().copy() for n in STATE}
        ref, what = states[i + 1], "%s, launch %d" % (name, i)
        for n in ("tokens", "step", "done", "log_tok", "log_rank"):
            assert (got[n] == getattr(ref, n)).all(), (what, n, got[n], getattr(ref, n))
        assert int(got["pos"][0]) == ref.pos, what
        for n in ("cand_logp", "log_logp"):
            assert (_bits(got[n]) == _bits(getattr(ref, n))).all(), (what, n)
        err = np.abs(got["log_pen"].astype(np.float64) - ref.log_pen)
        both_nan = np.isnan(got["log_pen"]) & np.isnan(ref.log_pen)
        print("%s: largest penalty error %.3g (bound %.3g)" % (what, float(np.nan_to_num(err).max()), R.cos_bound(c["d"])))
        assert (both_nan | (err <= R.cos_bound(c["d"]))).all(), (what, err.max())
        assert all(b.intact() for b in list(bufs.values()) + [hid, tp]), what
        # the same launch from the same state once more: the same bytes
        for n in STATE:
            bufs[n].set(before[n])
        lib.check(h.mtn_contrastive_advance(C.byref(a), lib.stream_ptr()))
        torch.cuda.synchronize()
        for n in STATE:
            assert (_bits(bufs[n].get()) == _bits(got[n])).all(), (what, n, "a second launch gave other bytes")


def test_the_operator_runs_a_chain_and_refuses_misuse():
    """ops.contrastive_advance on dense tensors: the chain of case d512_k5, and ValueError where the tensors do not fit."""
    from mtn_amd import ops
    c, (st, launches, eos), states = _reference("d512_k5")
    dev = torch.device("cuda", torch.cuda.current_device())
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    tokens, pos, cand, step, done = up(st.tokens), up(np.array([st.pos], dtype=np.int64)), up(st.cand_logp), up(st.step), up(st.done)
    log = (torch.zeros(c["L"], c["D"], dtype=torch.int32, device=dev), torch.zeros(c["L"], c["D"], device=dev),
           torch.zeros(c["L"], c["D"], device=dev), torch.zeros(c["L"], c["D"], dtype=torch.int32, device=dev))
    kw = dict(k=c["k"], alpha=c["alpha"], eos=eos, min_len=c["min_len"], banned=c["banned"])
    for hidden, top in launches:
        ops.contrastive_advance(up(hidden), up(top), tokens, pos, cand, step, done, log, **kw)
    ref = states[-1]
    assert (tokens.cpu().numpy() == ref.tokens).all() and (log[0].cpu().numpy() == ref.log_tok).all() and (log[3].cpu().numpy() == ref.log_rank).all()
    assert (_bits(log[1].cpu().numpy()) == _bits(ref.log_logp)).all() and int(pos.item()) == ref.pos
    hidden, top = up(launches[0][0]), up(launches[0][1])
    for bad in (dict(k=4), dict(k=0), dict(alpha=1.5), dict(alpha=float("nan")), dict(banned=(1, 2, 3, 4, 5))):
        with pytest.raises(ValueError):
            ops.contrastive_advance(hidden, top, tokens, pos, cand, step, done, log, **{**kw, **bad})
    with pytest.raises(ValueError):
        ops.contrastive_advance(hidden, top[:, :9].contiguous(), tokens, pos, cand, step, done, log, **kw)      # a head of 4 entries under k = 5
    with pytest.raises(ValueError):
        ops.contrastive_advance(hidden.double(), top, tokens, pos, cand, step, done, log, **kw)
    with pytest.raises(ValueError):
        ops.contrastive_advance(hidden, top, tokens.int(), pos, cand, step, done, log, **kw)
    assert (tokens.cpu().numpy() == ref.tokens).all()              # nothing was launched by the refused calls
