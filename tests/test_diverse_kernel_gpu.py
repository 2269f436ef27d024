"""csrc/diverse.hip against its numpy definition (tests/diverse_refs.py), without a model: mtn_topk_rows + mtn_diverse_advance over 6 steps
of seeded log-softmaxed rows.  The arithmetic is defined operation by operation, so after every step everything is held EXACTLY: tokens, pos,
anc, n_live, step, the integer logs, and lp / log_score / log_done bit for bit.  tests/test_diverse_refs.py shows that none of these inputs
holds a tie, so no case passes through the tie fallback."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import diverse_refs as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return torch.device("cuda:0")


class _Device:
    """The buffers of a search on the device, initialised as MegaDecodeSession._search_log initialises them."""

    def __init__(self, dev, D, B, G, L, k_top, k, lam):
        from mtn_amd import lib
        Bp, W, DG = B // G, D * B, D * G
        self.D, self.B, self.G, self.L, self.k_top = D, B, G, L, k_top
        tok = torch.full((W,), R.PAD, dtype=torch.int64)
        tok[::Bp] = R.START
        self.tokens, self.pos = tok.to(dev), torch.zeros(1, dtype=torch.int32, device=dev)
        self.anc = torch.arange(W, dtype=torch.int32).view(W, 1).repeat(1, L).to(dev)
        self.lp = torch.zeros(W, dtype=torch.float64, device=dev)
        self.n_live, self.step = torch.ones(DG, dtype=torch.int32, device=dev), torch.zeros(DG, dtype=torch.int32, device=dev)
        self.flags = torch.zeros(2, dtype=torch.int32, device=dev)
        self.log_parent, self.log_tok = (torch.zeros(L, W, dtype=torch.int32, device=dev) for _ in range(2))
        self.log_score, self.log_done = (torch.zeros(L, W, dtype=torch.float64, device=dev) for _ in range(2))
        self.log_n_old, self.log_n_new = (torch.zeros(L, DG, dtype=torch.int32, device=dev) for _ in range(2))
        da = lib.DiverseArgs()
        a = da.beam
        a.dialogues, a.width, a.L, a.k_top, a.k, a.beam, a.unk, a.eos, a.pad, a.min_len = DG, Bp, L, k_top, k, Bp, R.UNK, R.EOS, R.PAD, R.MIN_LEN
        a.penalty = R.PENALTY
        for name in ("tokens", "pos", "anc", "lp", "n_live", "step", "flags", "log_parent", "log_tok", "log_score", "log_done", "log_n_old", "log_n_new"):
            setattr(a, name, getattr(self, name).data_ptr())
        da.groups, da.diversity = G, lam
        self.args = da

    def advance(self, rows, plain=False):
        from mtn_amd import lib, ops
        top = ops.topk_rows(rows, self.k_top, R.EOS)
        self.args.beam.top = top.data_ptr()
        h = lib.load()
        rc = h.mtn_beam_advance(C.byref(self.args.beam), lib.stream_ptr()) if plain else h.mtn_diverse_advance(C.byref(self.args), lib.stream_ptr())
        lib.check(rc)
        torch.cuda.synchronize()

    def image(self):
        names = ("tokens", "pos", "anc", "lp", "n_live", "step", "flags", "log_parent", "log_tok", "log_score", "log_done", "log_n_old", "log_n_new")
        return {n: getattr(self, n).cpu().numpy() for n in names}


def _hold(img, st):
    for name in ("tokens", "anc", "n_live", "step", "log_parent", "log_tok", "log_n_old", "log_n_new"):
        assert np.array_equal(img[name], getattr(st, name)), name
    assert int(img["pos"][0]) == st.pos
    for name in ("lp", "log_score", "log_done"):
        assert img[name].tobytes() == getattr(st, name).tobytes(), name


@pytest.mark.parametrize("lam", R.KERNEL_LAMBDAS)
@pytest.mark.parametrize("D,B,G", R.KERNEL_SHAPES)
@pytest.mark.parametrize("V", R.KERNEL_V)
def test_every_step_equals_the_definition(dev, V, D, B, G, lam):
    k_top, k = B + 3, B // G + 2
    dv = _Device(dev, D, B, G, R.KERNEL_L, k_top, k, lam)
    st = R.State(D, B, G, R.KERNEL_L, R.START, R.PAD)
    for l in range(R.KERNEL_STEPS):
        rows = R.seeded_rows(V, D, B, G, l)
        R.advance(st, k_top, k, R.UNK, R.EOS, R.PENALTY, R.MIN_LEN, lam, heads=R.heads_of(rows, k_top, R.EOS))
        dv.advance(torch.from_numpy(rows).to(dev))
        img = dv.image()
        _hold(img, st)
        assert st.flag == 0 and int(img["flags"][0]) == 0


def test_tie_raises_the_flag(dev):
    D, B, G = 1, 4, 2
    rows = R.tie_rows(300, D * B)
    for lam, flag in ((0.5, 1), (0.0, 0)):
        dv = _Device(dev, D, B, G, R.KERNEL_L, B + 3, B // G + 2, lam)
        dv.advance(torch.from_numpy(rows).to(dev))
        assert int(dv.image()["flags"][0]) == flag, lam


@pytest.mark.parametrize("D,B", [(1, 5), (3, 4)])
def test_one_group_is_the_plain_kernel_bit_for_bit(dev, D, B):
    k_top, k = B + 3, B + 2
    new, old = (_Device(dev, D, B, 1, R.KERNEL_L, k_top, k, 0.0) for _ in range(2))
    for l in range(R.KERNEL_STEPS):
        rows = torch.from_numpy(R.seeded_rows(300, D, B, 1, l)).to(dev)
        new.advance(rows)
        old.advance(rows, plain=True)
        a, b = new.image(), old.image()
        for name in a:
            assert a[name].tobytes() == b[name].tobytes(), (l, name)
    assert int(a["step"][0]) == R.KERNEL_STEPS and int(a["n_live"][0]) == B


def test_bad_arguments_are_refused_without_a_launch(dev):
    from mtn_amd import lib
    h = lib.load()
    rows = torch.from_numpy(R.seeded_rows(300, 1, 4, 2, 0)).to(dev)
    bad = [dict(groups=0), dict(groups=3), dict(groups=16), dict(diversity=-0.5), dict(diversity=float("nan")), dict(diversity=float("inf")),
           dict(k_top=6), dict(k_top=17), dict(k=0), dict(k=8), dict(width=0), dict(beam=3), dict(lp=None), dict(log_done=None)]
    for change in bad:
        dv = _Device(dev, 1, 4, 2, R.KERNEL_L, 7, 4, 0.5)
        from mtn_amd import ops
        top = ops.topk_rows(rows, 7, R.EOS)
        dv.args.beam.top = top.data_ptr()
        for name, value in change.items():
            setattr(dv.args if name in ("groups", "diversity") else dv.args.beam, name, value)
        before = dv.image()
        rc = h.mtn_diverse_advance(C.byref(dv.args), lib.stream_ptr())
        assert rc != 0 and b"mtn_diverse_advance" in h.mtn_last_error(), change
        torch.cuda.synchronize()
        after = dv.image()
        assert all(before[n].tobytes() == after[n].tobytes() for n in before), change
    assert h.mtn_diverse_advance(None, lib.stream_ptr()) != 0
