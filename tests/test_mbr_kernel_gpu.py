"""mtn_mbr_select (csrc/mbr.hip) against its definition (tests/mbr_refs.py) on the GPU.  Every operation of the definition is integer or
one IEEE double operation in a stated order, so nothing here has a tolerance: util and expected are compared as bytes, best and order as
integers.  Explicit hypotheses with given and with NULL (uniform) weights, the sample-log source against the explicit one on the host-cut
lists, a set alone against the same set inside a launch of four, and two launches against each other."""
import functools
import random

import numpy as np
import pytest
import torch

from tests import mbr_refs as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _case(name):
    """(sets of hypotheses, K, L, N, n_hyp per set or None): the shapes of the issue's table, seeded."""
    rng = random.Random(sum(map(ord, name)))
    if name == "minimal":
        return [[[7]]], 1, 1, 1, None
    if name == "lengths-below-n":
        return [[[1, 2, 3], [2, 3]]], 2, 3, 4, None
    if name == "heavy-clipping":
        return [R.random_set(rng, 5, 9, 5) for _ in range(3)], 5, 9, 2, None
    if name == "repeats-mixed-lengths":                          # the sets tests/test_mbr_refs.py shows to move the answer off index 0
        sets = [hyps for hyps, _ in R.seeded_sets(2024, 2, 16, 30, 12)]
        sets[0][3], sets[1][0], sets[1][15] = [], [], []
        return sets, 16, 30, 4, None
    if name == "largest":                                        # long repeats over 5 values; some hypotheses fill all 128 positions
        hyps = R.random_set(rng, 16, 128, 5, min_len=90)
        hyps[2], hyps[9] = [rng.randrange(5) for _ in range(128)], [1, 2] * 64
        return [hyps], 16, 128, 4, None
    if name == "varying-n-hyp":
        return [R.random_set(rng, n, 20, 6) for n in (4, 3, 1, 0)], 4, 20, 3, [4, 3, 1, 0]
    if name == "wide-ids":                                       # token ids near +-2^30: compared as int32, nothing is an index
        vals = [2 ** 30 - 1, 2 ** 30, 2 ** 30 + 1, -2 ** 30, -2 ** 30 - 1, -2 ** 30 + 1, 2 ** 31 - 1, -2 ** 31]
        return [[[vals[rng.randrange(8)] for _ in range(rng.randint(0, 10))] for _ in range(4)] for _ in range(2)], 4, 10, 3, None
    if name == "duplicates":
        h, g = [4, 5, 6, 4, 5], [9, 9, 4]
        return [[g, h, [1], h, g, h]], 6, 5, 3, None
    raise KeyError(name)


CASES = ["minimal", "lengths-below-n", "heavy-clipping", "repeats-mixed-lengths", "largest", "varying-n-hyp", "wide-ids", "duplicates"]


@functools.lru_cache(maxsize=None)
def _reference(name, weighted):
    sets, K, L, N, n_hyp = _case(name)
    rng = random.Random(len(name))
    ws = [R.sorted_weights(rng, K) for _ in sets] if weighted else None
    ref = [R.select(hyps, N, None if ws is None else ws[s], K=K) for s, hyps in enumerate(sets)]
    return sets, K, L, N, n_hyp, ws, ref


def _pack(sets, K, L, n_hyp=None, ws=None, ldl=None):
    ldl = L if ldl is None else ldl
    tok = np.full((len(sets), K, ldl), -7, dtype=np.int64)       # (what lies past a hypothesis' length is never read as a token)
    length = np.zeros((len(sets), K), dtype=np.int32)
    for s, hyps in enumerate(sets):
        for k, h in enumerate(hyps):
            tok[s, k, :len(h)] = h
            length[s, k] = len(h)
    n = np.asarray([len(h) for h in sets] if n_hyp is None else n_hyp, dtype=np.int32)
    up = lambda a: torch.from_numpy(a).to(DEV)
    w = None if ws is None else up(np.asarray(ws, dtype=np.float64))
    return up(tok.astype(np.int32))[:, :, :L] if ldl != L else up(tok.astype(np.int32)), up(length), up(n), w


def _launch(N, **kw):
    from mtn_amd import ops
    expected, best, order, util = ops.mbr_select(N, util=True, **kw)
    torch.cuda.synchronize()
    return util.cpu().numpy(), expected.cpu().numpy(), best.cpu().numpy(), order.cpu().numpy()


def _check(got, ref, what):
    util, expected, best, order = got
    for s, (r_util, r_exp, r_best, r_order) in enumerate(ref):
        assert util[s].tobytes() == r_util.tobytes(), (what, s, "util", np.abs(util[s] - r_util).max())
        assert expected[s].tobytes() == r_exp.tobytes(), (what, s, "expected", expected[s], r_exp)
        assert int(best[s]) == r_best, (what, s, "best")
        assert np.array_equal(order[s], r_order), (what, s, "order")


@pytest.mark.parametrize("weighted", [True, False], ids=["given-weights", "null-weights"])
@pytest.mark.parametrize("name", CASES)
def test_kernel_equals_the_definition(name, weighted):
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    sets, K, L, N, n_hyp, ws, ref = _reference(name, weighted)
    tok, length, n, w = _pack(sets, K, L, n_hyp, ws)
    _check(_launch(N, tok=tok, length=length, n_hyp=n, w=w), ref, name)
    if name == "duplicates" and not weighted:
        assert ref[0][3].tolist() == [1, 3, 5, 0, 4, 2]                          # equal hypotheses tie; the lower index goes first
    if name == "varying-n-hyp":
        assert [r[2] for r in ref][3] == -1 and ref[1][1][3] == -1.0              # n_hyp = 0: best -1; past n_hyp: expected -1


def test_a_padded_token_stride_and_clamped_counts():
    """ldl > L reads the same tokens; a length outside [0, L] and an n_hyp outside [0, K] are clamped."""
    sets, K, L, N, n_hyp, ws, ref = _reference("heavy-clipping", True)
    tok, length, n, w = _pack(sets, K, L, n_hyp, ws, ldl=L + 3)
    assert tok.stride(1) == L + 3
    _check(_launch(N, tok=tok, length=length, n_hyp=n, w=w), ref, "ldl")
    full = [[h + [0] * (L - len(h)) if k == 1 else ([] if k == 2 else h) for k, h in enumerate(hyps)] for hyps in sets]
    tok, length, n, w = _pack(full, K, L, None, ws)
    length[:, 1], length[:, 2], n[:] = L + 5, -3, K + 2
    want = [R.select(hyps, N, ws[s], K=K) for s, hyps in enumerate(full)]
    _check(_launch(N, tok=tok, length=length, n_hyp=n, w=w), want, "clamped")


def test_sample_log_source_equals_explicit_on_the_host_cut():
    """2 sets x 4 columns, L = 12: an <eos> at position 0, one mid-column, one in the last position, columns without one."""
    eos, S, K, L, N = 3, 2, 4, 12, 3
    rng = random.Random(5)
    log = np.asarray([[rng.choice([4, 5, 6, 7]) for _ in range(S * K)] for _ in range(L)], dtype=np.int32)
    log[0, 1] = eos
    log[5, 2], log[8, 2] = eos, eos                              # the first one cuts
    log[L - 1, 6] = eos
    log[4, 7] = eos
    hyps = R.cut_log(log, eos)
    assert [len(h) for h in hyps] == [11, 0, 5, 11, 11, 11, 11, 4]
    sets = [hyps[:K], hyps[K:]]
    ref = [R.select(h, N, K=K) for h in sets]
    got = _launch(N, log_tok=torch.from_numpy(log).to(DEV), sets=S, eos=eos)
    _check(got, ref, "log")
    tok, length, n, _ = _pack(sets, K, L)
    explicit = _launch(N, tok=tok, length=length, n_hyp=n)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, explicit))


def test_a_set_does_not_depend_on_its_neighbours_and_launches_repeat():
    sets = [hyps for hyps, _ in R.seeded_sets(77, 4, 16, 30, 12)]
    ws = [w for _, w in R.seeded_sets(77, 4, 16, 30, 12)]
    four = _launch(4, **dict(zip(("tok", "length", "n_hyp", "w"), _pack(sets, 16, 30, None, ws))))
    again = _launch(4, **dict(zip(("tok", "length", "n_hyp", "w"), _pack(sets, 16, 30, None, ws))))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(four, again))
    alone = _launch(4, **dict(zip(("tok", "length", "n_hyp", "w"), _pack(sets[2:3], 16, 30, None, ws[2:3]))))
    assert all(a[2:3].tobytes() == b.tobytes() for a, b in zip(four, alone))
    assert len({int(b) for b in four[2]}) > 1 or int(four[2][0]) != 0            # (the answers are not all index 0)
