"""mtn_constrain_rows (csrc/constrain.hip) through ops.constrain_rows against its numpy definitions (tests/constrain_refs.py), and the two
selection kernels behind it (mtn_topk_rows, mtn_sample_rows) on rows that hold -inf.

The bar is exact: the transform is one fp32 multiply per penalised column and -inf writes, so the set of -inf columns must be the
reference's and EVERY column — penalised, banned or untouched — must hold the reference's bits.  Shapes: vocabularies that are no
multiple of 4 or of the workgroup (259, 1003) and run.sh's 3004; row strides V and V + 5 (rows that are not 16-byte aligned: the scalar
copy); 1, 5 and 16 rows; L = 12; history lengths 0, 1, N-2, N-1, L; both history sources; in place and out of place."""
import numpy as np
import pytest
import torch

from tests.constrain_refs import constrain_row, history_from_log

pytestmark = pytest.mark.gpu
L = 12
NGRAMS = (0, 1, 2, 3, 4, 8)
THETAS = (1.0, 1.3)
PAD_BITS = 0x7FC01234                                        # a NaN pattern in the columns V..ldx-1: they must keep it


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    from mtn_amd import lib
    lib.load()
    return torch.device("cuda:0")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _logp(rs, rows, V):
    z = rs.randn(rows, V) * 3.0
    z = z - z.max(1, keepdims=True)
    return (z - np.log(np.exp(z).sum(1, keepdims=True))).astype(np.float32)


def _alphabet(rs, V):
    """Six tokens the histories are drawn from — few, so that n-grams do repeat — with the first and the last column among them."""
    return np.concatenate([[0, V - 1], rs.choice(np.arange(1, V - 1), 4, replace=False)]).astype(np.int64)


def _histories(rs, V, N):
    """Histories of the lengths that matter for N (0, 1, N-2, N-1, L) plus full-length ones that do hold repeats: random over the small
    alphabet, period 2 and constant (the only ones an 8-gram of L = 12 can repeat in)."""
    al = _alphabet(rs, V)
    draw = lambda n: [int(t) for t in al[rs.randint(0, al.size, size=n)]]
    lens = sorted({0, 1, max(N - 2, 0), max(N - 1, 0), min(N, L), L})
    hs = [draw(n) for n in lens]
    hs += [draw(L), draw(7), [int(al[2]), int(al[1])] * (L // 2), [int(al[3])] * L, [int(al[0])] * (L - 1)]
    return hs


def _padded(dev, x, ld, fill_bits=PAD_BITS):
    """x (rows, V) float32 numpy -> a device tensor of row stride ld whose first V columns hold x; the view over them."""
    rows, V = x.shape
    buf = np.full((rows, ld), fill_bits, dtype=np.uint32)
    buf[:, :V] = _bits(x)
    t = torch.from_numpy(buf.view(np.float32)).to(dev)
    return t, t[:, :V]


def _check(got_buf, want, V, what):
    got = got_buf.cpu().numpy()
    g, w = _bits(got[:, :V]), _bits(want)
    assert np.array_equal(np.isneginf(got[:, :V]), np.isneginf(want)), what          # the banned set
    assert np.array_equal(g, w), (what, np.argwhere(g != w)[:4])                      # every column, bit for bit
    assert (got.view(np.uint32)[:, V:] == PAD_BITS).all(), what                        # nothing past V is written


@pytest.mark.parametrize("rows", [1, 5, 16])
@pytest.mark.parametrize("pad", [0, 5], ids=["ldx=V", "ldx=V+5"])
@pytest.mark.parametrize("V", [259, 1003, 3004])
def test_explicit_history_equals_reference_bitwise(dev, V, pad, rows):
    from mtn_amd import ops
    rs = np.random.RandomState(V + 7 * pad + rows)
    banned_any = {N: 0 for N in NGRAMS}
    for N in NGRAMS:
        hs = _histories(rs, V, N)
        for g0 in range(0, len(hs), rows):
            group = [hs[(g0 + i) % len(hs)] for i in range(rows)]
            x = _logp(rs, rows, V)
            hist = np.full((rows, L + 3), -5, dtype=np.int32)              # (a table wider than L: row stride ldh = L + 3)
            for r, h in enumerate(group):
                hist[r, :len(h)] = h
            hist_t = torch.from_numpy(hist).to(dev)
            len_t = torch.tensor([len(h) for h in group], dtype=torch.int32, device=dev)
            for theta in THETAS:
                want = np.stack([constrain_row(x[r], group[r], N, theta) for r in range(rows)])
                banned_any[N] += int(np.isneginf(want).sum())
                # out of place: the input keeps its bits
                src_buf, src = _padded(dev, x, V + pad)
                dst_buf, dst = _padded(dev, np.zeros_like(x), V + pad)
                ops.constrain_rows(src, N, theta, hist=hist_t, hist_len=len_t, log_len=L, out=dst)
                _check(dst_buf, want, V, ("out of place", N, theta, g0))
                _check(src_buf, x, V, ("input of out of place", N, theta, g0))
                # in place
                ret = ops.constrain_rows(src, N, theta, hist=hist_t, hist_len=len_t, log_len=L)
                assert ret.data_ptr() == src.data_ptr()
                _check(src_buf, want, V, ("in place", N, theta, g0))
    assert banned_any[0] == 0 and all(banned_any[N] > 0 for N in NGRAMS if N), banned_any       # the cases do ban something for every N


def _beam_log(rs, V, Lg, D, width, steps):
    """A step log as mtn_beam_advance leaves it: per step and dialogue a random number of live rows with parents among the rows live a
    step earlier (non-identity), tokens over a small alphabet; every entry past the live count holds arbitrary in-range values."""
    al = _alphabet(rs, V)
    rows = D * width
    tok = rs.randint(0, V, size=(Lg, rows)).astype(np.int32)               # (dead rows: any token, any parent in [0, width))
    par = rs.randint(0, width, size=(Lg, rows)).astype(np.int32)
    for d in range(D):
        live_prev = 1
        for j in range(Lg):
            live = int(rs.randint(1, width + 1)) if j else min(width, 3)
            for i in range(live):
                tok[j, d * width + i] = al[rs.randint(0, al.size)]
                par[j, d * width + i] = rs.randint(0, live_prev)
            live_prev = live
    return tok, par, np.asarray(steps, dtype=np.int32)


@pytest.mark.parametrize("inplace", [True, False], ids=["in-place", "out-of-place"])
@pytest.mark.parametrize("V", [259, 1003, 3004])
def test_step_log_history_of_a_beam_equals_reference_bitwise(dev, V, inplace):
    """2 dialogues x width 4 (rows_per_step = width: a step counter per dialogue), non-identity parents, dead rows holding arbitrary
    in-range values; the step counters cover 0, 1, N-2, N-1, L (and L + 5: clamped)."""
    from mtn_amd import ops
    D, width = 2, 4
    rows = D * width
    rs = np.random.RandomState(V + int(inplace))
    any_ban = 0
    for N in NGRAMS:
        for steps in ([0, 1], [max(N - 2, 0), max(N - 1, 0)], [L, 7], [L + 5, min(N, L)]):
            tok, par, st = _beam_log(rs, V, L, D, width, steps)
            x = _logp(rs, rows, V)
            tok_t, par_t, st_t = (torch.from_numpy(a).to(dev) for a in (tok, par, st))
            for theta in THETAS:
                hs = [history_from_log(tok, par, st[r // width], r, width) for r in range(rows)]
                want = np.stack([constrain_row(x[r], hs[r], N, theta) for r in range(rows)])
                any_ban += int(np.isneginf(want).sum())
                src_buf, src = _padded(dev, x, V + 5)
                dst_buf, dst = (src_buf, src) if inplace else _padded(dev, np.zeros_like(x), V + 5)
                ops.constrain_rows(src, N, theta, log_tok=tok_t, log_parent=par_t, step=st_t, width=width, rows_per_step=width,
                                   out=None if inplace else dst)
                _check(dst_buf, want, V, (N, theta, steps))
                # raw device pointers, as a captured search passes them
                src_buf, src = _padded(dev, x, V)
                ops.constrain_rows(src, N, theta, log_tok=tok_t.data_ptr(), log_parent=par_t.data_ptr(), step=st_t.data_ptr(), width=width,
                                   rows_per_step=width, log_len=L)
                _check(src_buf, want, V, ("pointers", N, theta, steps))
    assert any_ban > 0


@pytest.mark.parametrize("rows", [1, 5, 16])
def test_step_log_history_without_parents_is_the_rows_own_column(dev, rows):
    """The sampling search's log: no parents (NULL = identity), a step counter per row."""
    from mtn_amd import ops
    V = 1003
    rs = np.random.RandomState(rows)
    al = _alphabet(rs, V)
    for N in NGRAMS:
        tok = al[rs.randint(0, al.size, size=(L, rows))].astype(np.int32)
        st = np.asarray([[0, 1, max(N - 2, 0), max(N - 1, 0), L][r % 5] for r in range(rows)], dtype=np.int32)
        if rows == 1:
            st[0] = L
        x = _logp(rs, rows, V)
        hs = [history_from_log(tok, None, st[r], r, 1) for r in range(rows)]
        for theta in THETAS:
            want = np.stack([constrain_row(x[r], hs[r], N, theta) for r in range(rows)])
            src_buf, src = _padded(dev, x, V)
            ops.constrain_rows(src, N, theta, log_tok=torch.from_numpy(tok).to(dev), step=torch.from_numpy(st).to(dev), width=1, rows_per_step=1)
            _check(src_buf, want, V, (N, theta))


def test_long_step_log_is_walked_in_chunks_and_stale_values_are_clamped(dev):
    """L = 300 positions (the kernel stages 128 per round: three rounds, the walk's row carried across them), width 8, and a log whose dead
    rows hold parents and tokens outside their ranges: parents are clamped, such tokens name no column."""
    from mtn_amd import ops
    V, Lg, D, width = 259, 300, 2, 8
    rows = D * width
    rs = np.random.RandomState(5)
    tok, par, st = _beam_log(rs, V, Lg, D, width, [Lg, 131])
    for j, r, p, t in [(3, 7, 11, V + 40), (140, 15, -3, -1), (299, 6, 8, 1 << 24), (130, 12, 200, V)]:
        par[j, r], tok[j, r] = p, t
    x = _logp(rs, rows, V)
    hs = [history_from_log(tok, par, st[r // width], r, width) for r in range(rows)]
    assert len(hs[0]) == Lg and len(hs[8]) == 131
    for N, theta in [(3, 1.3), (4, 1.0), (1, 1.3)]:
        want = np.stack([constrain_row(x[r], hs[r], N, theta) for r in range(rows)])
        src_buf, src = _padded(dev, x, V + 5)
        ops.constrain_rows(src, N, theta, log_tok=torch.from_numpy(tok).to(dev), log_parent=torch.from_numpy(par).to(dev),
                           step=torch.from_numpy(st).to(dev), width=width, rows_per_step=width)
        _check(src_buf, want, V, (N, theta))
        assert np.isneginf(want).any()


def test_bad_arguments_are_refused(dev):
    from mtn_amd import lib, ops
    x = torch.zeros(4, 64, device=dev)
    h, n = torch.zeros(4, L, dtype=torch.int32, device=dev), torch.zeros(4, dtype=torch.int32, device=dev)
    assert lib.load().mtn_version() >= 117
    for kw in (dict(ngram=9), dict(ngram=-1), dict(theta=0.9), dict(theta=float("nan"))):
        with pytest.raises(ValueError):
            ops.constrain_rows(x, **dict(dict(ngram=2, theta=1.0, hist=h, hist_len=n), **kw))
    with pytest.raises(ValueError):
        ops.constrain_rows(x, 2, 1.0)                                      # no history source
    with pytest.raises(ValueError):
        ops.constrain_rows(x, 2, 1.0, log_tok=h.t().contiguous()[:, :3].contiguous(), step=n, width=3)       # rows no multiple of width
    with pytest.raises(ValueError):
        ops.constrain_rows(x, 2, 1.0, hist=h, hist_len=n, out=torch.zeros(4, 63, device=dev))
    with pytest.raises(ValueError):
        ops.constrain_rows(x, 2, 1.0, hist=h)                              # an explicit table without its lengths
    buf = torch.zeros(5, 64, device=dev)
    with pytest.raises(ValueError):
        ops.constrain_rows(buf[:4], 2, 1.0, hist=h, hist_len=n, out=buf[1:])       # out overlaps logp and is not logp
    assert ops.constrain_rows(buf[:4], 2, 1.0, hist=h, hist_len=n, out=buf[:4]).data_ptr() == buf.data_ptr()     # logp itself: in place
    wide = torch.zeros(4, 128, device=dev)
    ops.constrain_rows(wide[:, :64], 2, 1.0, hist=h, hist_len=n, out=wide[:, 64:])    # two column blocks of one buffer do not overlap
    with pytest.raises(ValueError):
        ops.constrain_rows(wide[:, :64], 2, 1.0, hist=h, hist_len=n, out=wide[:, 32:96])
    with pytest.raises(ValueError):
        ops.constrain_rows(x.double(), 2, 1.0, hist=h, hist_len=n)
    with pytest.raises(Exception):
        ops.constrain_rows(torch.zeros(4, 64), 2, 1.0, hist=h, hist_len=n)  # CPU rows
    with pytest.raises(lib.MtnHipError):                                   # the library's own check: a history longer than it stages
        big = torch.zeros(4, 1025, dtype=torch.int32, device=dev)
        ops.constrain_rows(x, 2, 1.0, hist=big, hist_len=n)


# ------------------------------------------------------------------------------------------------ the selection kernels on rows with -inf
def _banned_rows(rs, rows, V, counts):
    x = _logp(rs, rows, V)
    sets = []
    for r in range(rows):
        nb = counts[r % len(counts)]
        order = np.argsort(-x[r], kind="stable")
        # half of the banned columns are the row's MOST probable ones, the rest random
        b = set(int(c) for c in order[:nb // 2])
        rest = [c for c in rs.permutation(V) if int(c) not in b]
        b |= set(int(c) for c in rest[:nb - len(b)])
        x[r, sorted(b)] = -np.inf
        sets.append(b)
    return x, sets


@pytest.mark.parametrize("V,k", [(259, 7), (1003, 16), (3004, 8), (4100, 7)])
def test_topk_rows_heads_hold_no_banned_column(dev, V, k):
    """Rows with -inf entries (V = 4100: the path that re-reads rows longer than its registers): while V - banned >= k, the head is the k
    largest FINITE entries in the documented order (descending, equal values by ascending column) and names no banned column."""
    from mtn_amd import ops
    rs = np.random.RandomState(V)
    counts = [0, 1, 10, V // 2, V - k - 1, V - k]
    x, sets = _banned_rows(rs, len(counts), V, counts)
    x[2, [c for c in range(V) if c not in sets[2]][:3]] = np.float32(-1.25)          # a tie among finite entries next to the -inf ones
    eos = 3
    out = ops.topk_rows(torch.from_numpy(x).to(dev), k, eos).cpu().numpy()
    for r, b in enumerate(sets):
        assert V - len(b) >= k
        order = sorted(range(V), key=lambda c: (-x[r, c], c))[:k]
        cols = [int(c) for c in out[r, k:2 * k]]
        assert cols == order and not (set(cols) & b), r
        assert np.array_equal(_bits(out[r, :k]), _bits(x[r, order])) and np.isfinite(out[r, :k]).all(), r
        assert _bits(out[r, 2 * k:])[0] == _bits(x[r, eos:eos + 1])[0]              # the extra column travels as it is, -inf included


@pytest.mark.parametrize("V", [259, 3004, 4100])
@pytest.mark.parametrize("filt", [dict(), dict(top_k=5), dict(top_p=0.9, temperature=0.7), dict(top_k=1)], ids=["plain", "top-k", "top-p", "argmax"])
def test_sample_rows_never_draws_a_banned_token(dev, V, filt):
    """-inf columns have probability 0 under every filter: 16 rows x 12 positions of draws, the most probable columns banned among them."""
    from mtn_amd import ops
    rs = np.random.RandomState(V + len(filt))
    rows, steps = 16, 12
    counts = [0, 4, 40, V // 2, V - 2, V - 1]
    x, sets = _banned_rows(rs, rows, V, counts)
    xt = torch.from_numpy(x).to(dev)
    seed = torch.tensor([12345], dtype=torch.int64, device=dev)
    keys = torch.arange(rows, dtype=torch.int64, device=dev)
    step = torch.zeros(rows, dtype=torch.int32, device=dev)
    log = None
    for _ in range(steps):
        log = ops.sample_rows(xt, seed, keys, step, log, max_len=steps, **filt)
    tok, lp = log[0].cpu().numpy(), log[1].cpu().numpy()
    assert step.cpu().tolist() == [steps] * rows
    for r in range(rows):
        drawn = set(int(t) for t in tok[:, r])
        assert not (drawn & sets[r]), (r, sorted(drawn & sets[r]))
        assert np.isfinite(lp[:, r]).all() and np.array_equal(_bits(lp[:, r]), _bits(x[r, tok[:, r]]))
