"""mtn_sample_rows (csrc/sample.hip) through the C ABI against the float64 restatement of its definitions (tests/sample_refs.py).

Tolerance of the admissibility check: eps = 2e-5 in CDF units, for the kernel's fp32 arithmetic on the IDENTICAL fp32 input.  A mass
is the sum of <= 2^15 non-negative terms reduced as 256 sequential per-thread chunks (<= 128 terms) plus an 8-level tree: relative
error <= (128 + 8) x 2^-24 = 8e-6 worst case, about 4e-6 with the error of expf (2 ulp) and of the rounded argument (x - max) / T; eps is
5 times that."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import sample_refs as R

pytestmark = pytest.mark.gpu
EPS = 2e-5
SEED = 0x1234567887654321


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    from mtn_amd import lib
    lib.load()
    return torch.device("cuda:0")


def _sample(dev, logp, keys, step, prm, seed=SEED, rows=None, L=None, books=False):
    """One kernel call: logp (n, V) float32 numpy, per-row keys / positions.  Returns (token, logp[token], u) per row (+ bookkeeping)."""
    from mtn_amd import ops
    x = torch.from_numpy(np.ascontiguousarray(logp, dtype=np.float32)).to(dev)
    rows = x.size(0) if rows is None else rows
    L = int(max(step)) + 2 if L is None else L
    seed_t = torch.tensor([seed if seed < 2 ** 63 else seed - 2 ** 64], dtype=torch.int64, device=dev)
    keys_t = torch.tensor(np.asarray(keys, dtype=np.int64), device=dev)
    step_t = torch.tensor(np.asarray(step, dtype=np.int32), device=dev)
    log = (torch.full((L, rows), -7, dtype=torch.int32, device=dev), torch.zeros(L, rows, device=dev), torch.zeros(L, rows, device=dev))
    kw = dict(temperature=prm.temperature, top_k=prm.top_k, top_p=prm.top_p, banned=prm.banned, eos=prm.eos, min_len=prm.min_len, rows=rows)
    extra = None
    if books:
        extra = (torch.full((rows,), -1, dtype=torch.int64, device=dev), torch.full((1,), -1, dtype=torch.int32, device=dev),
                 torch.full((rows, L), -1, dtype=torch.int32, device=dev))
        kw.update(tokens=extra[0], pos=extra[1], anc=extra[2])
    ops.sample_rows(x, seed_t, keys_t, step_t, log, **kw)
    torch.cuda.synchronize()
    at = (torch.tensor(np.asarray(step, dtype=np.int64), device=dev), torch.arange(rows, device=dev))
    out = tuple(t[at].cpu().numpy() for t in log)
    # nothing but the rows' own log entries was written
    assert int((log[0] != -7).sum()) == rows
    return out + ((step_t.cpu().numpy(),) + tuple(t.cpu().numpy() for t in extra) if books else (step_t.cpu().numpy(),))


def _rows(V, seed):
    """Random (Gaussian logits), peaked (one token holds most of the mass) and flat (near-uniform, distinct values) rows."""
    rs = np.random.RandomState(seed)
    lsm = lambda z: (z - z.max() - np.log(np.exp(z - z.max()).sum())).astype(np.float32)
    peaked = rs.randn(V) * 2.0
    peaked[rs.randint(V)] += 12.0
    return [lsm(rs.randn(V) * 3.0), lsm(peaked), lsm(rs.randn(V) * 0.05), lsm(rs.randn(V) * 6.0)]


def _generator_row(dev, V):
    """A real generator row: log-probabilities of a random bf16 Generator of vocabulary V through the product path."""
    from mtn_amd import ops
    g = torch.Generator().manual_seed(V)
    w = (torch.randn(V, 128, generator=g) * 0.3).to(dev).to(torch.bfloat16)
    b = (torch.randn(V, generator=g) * 0.5).to(dev)
    x = torch.randn(1, 128, generator=g).to(dev)
    return ops.generator_log_probs(x, w, b)[0].cpu().numpy()


@pytest.mark.parametrize("V", [37, 3000, 8191, 20000])
def test_every_token_is_admissible_and_u_is_the_hash(dev, V):
    """(a) T x top_k x top_p grid on random / peaked / flat rows and one generator row, with bans and min_len: the returned token is in
    admissible(..., eps), the logged u IS the numpy hash, the logged log-probability is the model's."""
    rows = _rows(V, V) + [_generator_row(dev, V)]
    eos = 3 % V
    worst = 0
    for ti, T in enumerate((0.7, 1.0, 1.5)):
        for ki, top_k in enumerate((0, 1, 5, 40, V)):
            for pi, top_p in enumerate((1.0, 0.9, 0.3)):
                banned = (0, 1, 2) if (ti + ki + pi) % 2 == 0 else (int(np.argmax(rows[0])),)
                prm = R.Params(T, min(top_k, V), top_p, banned=banned, eos=eos, min_len=2)
                # several draws per row: different keys and positions (below and at min_len)
                reps = 6
                x = np.stack([r for r in rows for _ in range(reps)])
                keys = [(1 << 33) * (i % 3) + 17 * i + ki for i in range(len(x))]
                step = [i % 4 for i in range(len(x))]
                tok, lp, u, new_step = _sample(dev, x, keys, step, prm)
                want_u = R.uniform24(SEED, np.asarray(keys, dtype=np.int64), np.asarray(step))
                assert (u.astype(np.float64) == want_u).all()
                assert (new_step == np.asarray(step) + 1).all()
                for i in range(len(x)):
                    ok = R.admissible(x[i], float(want_u[i]), prm, EPS, position=step[i])
                    assert int(tok[i]) in ok, (V, T, top_k, top_p, i, int(tok[i]), sorted(ok)[:8])
                    assert lp[i] == x[i][tok[i]]
                    assert tok[i] not in prm.banned_at(step[i])
                    worst = max(worst, len(ok))
    print(f"V = {V}: largest admissible set {worst} tokens")


@pytest.mark.parametrize("V", [37, 3000, 20000])
def test_top_k_one_is_argmax(dev, V):
    """(b) top_k = 1 at any temperature / top_p returns the arg-max of what is not banned, whatever u."""
    rows = _rows(V, V + 1)
    x = np.stack([r for r in rows for _ in range(8)])
    keys = np.arange(len(x)) * 31 + 5
    for T, top_p, banned in ((1.0, 1.0, ()), (0.7, 0.3, ()), (1.5, 0.9, (int(np.argmax(rows[1])),))):
        tok, _, _, _ = _sample(dev, x, keys, [0] * len(x), R.Params(T, 1, top_p, banned=banned))
        want = x.copy()
        for b in banned:
            want[:, b] = -np.inf
        assert (tok == want.argmax(axis=1)).all()


def _chi2_pvalue(stat, dof):
    z = ((stat / dof) ** (1.0 / 3.0) - (1.0 - 2.0 / (9.0 * dof))) / math.sqrt(2.0 / (9.0 * dof))
    return 0.5 * math.erfc(z / math.sqrt(2.0))


@pytest.mark.parametrize("top_p", [1.0, 0.9])
def test_distribution_of_65536_rows_reading_one_row(dev, top_p):
    """(c) 65 536 rows with ldx = 0, each with its own key: the token histogram against the float64 filtered distribution — chi-square
    over the bins of expected count >= 20 (the rest lumped into one), p-value >= 1e-6."""
    n, V = 65536, 3000
    x = _rows(V, 99)[0]
    prm = R.Params(0.9, 200, top_p, banned=(0, 1, 2), eos=3, min_len=1)
    tok, _, u, _ = _sample(dev, x[None, :], np.arange(n, dtype=np.int64) * 3 + 11, [0] * n, prm, rows=n)
    p = R.filtered(x, prm, position=0)
    assert (p[tok] > 0).mean() > 0.999                     # (a token beside a threshold may differ: the admissibility test bounds that)
    counts = np.bincount(tok, minlength=V).astype(np.float64)
    expect = p * n
    big = expect >= 20
    obs = np.concatenate([counts[big], [counts[~big].sum()]])
    exp = np.concatenate([expect[big], [expect[~big].sum()]])
    if exp[-1] < 20:                                       # (the lump itself too small: merge it into the smallest bin)
        j = int(np.argmin(exp[:-1]))
        obs[j] += obs[-1]
        exp[j] += exp[-1]
        obs, exp = obs[:-1], exp[:-1]
    stat = float(((obs - exp) ** 2 / exp).sum())
    pv = _chi2_pvalue(stat, len(obs) - 1)
    print(f"top_p {top_p}: {len(obs)} bins, chi-square {stat:.1f}, p = {pv:.3g}")
    assert len(obs) >= 30 and pv >= 1e-6


def test_permuting_rows_with_their_keys_permutes_the_outputs(dev):
    """(d) a row's draw depends on its own (distribution, key, position) only."""
    V = 3000
    rs = np.random.RandomState(5)
    x = np.stack(_rows(V, 7) * 4)
    keys = rs.randint(0, 1 << 40, size=len(x)).astype(np.int64)
    step = rs.randint(0, 5, size=len(x))
    prm = R.Params(0.8, 50, 0.95, banned=(1,), eos=3, min_len=2)
    a = _sample(dev, x, keys, step, prm, L=8)
    perm = rs.permutation(len(x))
    b = _sample(dev, x[perm], keys[perm], step[perm], prm, L=8)
    for u, v in zip(a[:3], b[:3]):
        assert (u[perm] == v).all()
    assert len(set(a[0].tolist())) > 4


def test_bookkeeping_for_the_next_decode_step(dev):
    """(e) tokens / pos / anc after a call: the newest token of every row, position + 1, identity ancestors at the new position —
    and nothing else."""
    V, L = 500, 6
    x = np.stack(_rows(V, 11))
    prm = R.Params(1.0, 0, 1.0)
    tok, _, _, step, tokens, pos, anc = _sample(dev, x, [1, 2, 3, 4], [2, 2, 2, 2], prm, L=L, books=True)
    assert (tokens == tok).all() and pos[0] == 3 and (step == 3).all()
    want = np.full((4, L), -1)
    want[:, 3] = np.arange(4)
    assert (anc == want).all()
    # the last position of the log: no ancestor slot beyond the table
    tok, _, _, step, tokens, pos, anc = _sample(dev, x, [1, 2, 3, 4], [L - 1] * 4, prm, L=L, books=True)
    assert (anc == -1).all() and pos[0] == L and (tokens == tok).all()
    # bad arguments are reported
    from mtn_amd import lib, ops
    with pytest.raises(lib.MtnHipError):
        _sample(dev, x, [1, 2, 3, 4], [0] * 4, R.Params(0.0))
    with pytest.raises(lib.MtnHipError):
        _sample(dev, x, [1, 2, 3, 4], [0] * 4, R.Params(1.0, 0, 1.5))
    assert lib.load().mtn_version() >= 115
