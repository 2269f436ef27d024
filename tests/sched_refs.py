"""Scheduled sampling's token mix (include/mtn_hip.h mtn_sched_mix) restated in numpy: the counter hash (tests/sample_refs.py, integer
arithmetic, bit-exact with the kernel's), the float32 schedule and coin (bit-exact too: separately rounded operations), the arg-max pick,
and the Gumbel-max pick in float64 with a per-column bound E_c on |s_fp32 - s_fp64| for the kernel's fp32 scores.  ``CASES`` are the
shapes the GPU test runs; tests/test_sched_refs.py checks on the CPU that they can tell a wrong pick from a right one.

The bound.  eps = 2^-24 is fp32's unit roundoff; HIP's math API documents logf and log1pf at 1 ulp, a relative error of at most 2 eps.
The kernel computes, per admitted column, from EXACT fp32 inputs (u_c below one half, 1 - u_c above):
    w  = -logf(u) or -log1pf(-(1 - u))          w32 = w (1 + d1),                 |d1| <= 2 eps
    g  = -logf(w)                                g32 = (g - log(1 + d1)) (1 + d2), |d2| <= 2 eps   =>  |g32 - g| <= 2 eps (1 + |g|) (1 + o)
    zt = z * inv_temperature                     zt32 = zt (1 + d3),               |d3| <= eps
    s  = zt + g                                  s32 = (zt32 + g32) (1 + d4),      |d4| <= eps
so  |s32 - s| <= eps |zt| + 2 eps (1 + |g|) + eps |s|, times (1 + 2^-20) for the second-order terms, plus 2^-126 for a subnormal result.
An infinite score (z = +-inf) is exact: E = 0.  A product at or beyond 2^127 may overflow in fp32: E = inf there."""
import numpy as np

from tests.sample_refs import sample_hash

ARGMAX, SAMPLE = 0, 1
F = np.float32
EPS = 2.0 ** -24
LOG_ULP = 1.0                     # HIP math API: logf 1 ulp, log1pf 1 ulp
COIN_POS = 0xFFFFFFFF
M64 = 0xFFFFFFFFFFFFFFFF


def prob(step, p_max, start, ramp):
    """p at ``step`` in the kernel's fp32 arithmetic: a subtract, a max, a divide, a min, a multiply."""
    step, p_max = F(step), F(p_max)
    if ramp == 0:
        return p_max if step >= F(start) else F(0.0)
    d = np.maximum(F(0.0), F(step - F(start)))
    q = F(d / F(ramp))
    return F(p_max * np.minimum(F(1.0), q))


def _words(seed, step, key, T):
    """(seed word, key words (B, T) as int64 bit patterns) of the coin and the draws."""
    sw = (int(seed) + int(step)) & M64
    kw = (np.asarray(key, dtype=np.int64).view(np.uint64)[:, None] << np.uint64(12)) | np.arange(T, dtype=np.uint64)[None, :]
    return sw, kw.view(np.int64)


def coin(seed, step, key, T):
    """u (B, T) float32 in [0, 1): exact."""
    sw, kw = _words(seed, step, key, T)
    return ((sample_hash(sw, kw, COIN_POS) >> np.uint64(8)).astype(np.float64) / 16777216.0).astype(F)


def column_bits(seed, step, key, T, V):
    """k (B, T, V) uint64: the top 24 bits of each column's hash at each position."""
    sw, kw = _words(seed, step, key, T)
    return sample_hash(sw, kw[:, :, None], np.arange(V, dtype=np.uint64)[None, None, :]) >> np.uint64(8)


def gumbel64(k):
    """g = -log(-log(u)), u = (k + 0.5) 2^-24, in float64 (u near 1 through log1p of the exact 1 - u)."""
    k = np.asarray(k, dtype=np.float64)
    u = (k + 0.5) / 16777216.0
    v = (16777215.0 - k + 0.5) / 16777216.0
    with np.errstate(divide="ignore", invalid="ignore"):
        w = np.where(k < 8388608.0, -np.log(u), -np.log1p(-v))
    return -np.log(w)


def gumbel32(k):
    """The kernel's operations in numpy float32."""
    k = np.asarray(k)
    lo = k < (1 << 23)
    u = (k.astype(F) + F(0.5)) * F(2.0 ** -24)
    v = ((16777215 - k.astype(np.int64)).astype(F) + F(0.5)) * F(2.0 ** -24)
    with np.errstate(divide="ignore", invalid="ignore"):
        w = np.where(lo, -np.log(np.where(lo, u, F(0.5))), -np.log1p(-np.where(lo, F(0.25), v))).astype(F)
        return (-np.log(w)).astype(F)


def scores64(z, inv_t, k):
    """(s, E): the float64 Gumbel scores of logits z (..., V) and the bound on the kernel's fp32 scores' distance from them."""
    zt = np.asarray(z, dtype=np.float64) * float(F(inv_t))
    g = gumbel64(k)
    with np.errstate(invalid="ignore"):
        s = zt + g
        E = (EPS * np.abs(zt) + 2.0 * LOG_ULP * EPS * (1.0 + np.abs(g)) + EPS * np.abs(s)) * (1.0 + 2.0 ** -20) + 2.0 ** -126
        E = np.where(np.abs(zt) >= 2.0 ** 127, np.inf, E)         # the fp32 product may overflow where float64's does not: no bound
    return s, np.where(np.isfinite(s), E, 0.0)


def scores32(z, inv_t, k):
    """The kernel's fp32 scores: a multiply, then an add."""
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.asarray(z, dtype=F) * F(inv_t)).astype(F) + gumbel32(k)


def admitted(V, pad, banned):
    ok = np.ones(V, dtype=bool)
    for c in (pad,) + tuple(banned):
        if 0 <= c < V:
            ok[c] = False
    return ok


def pick_row(s, ok):
    """(column, score) of the largest admitted score, ties to the lowest column; (-1, nan): nothing admitted, or a NaN among them."""
    if not ok.any() or np.isnan(s[ok]).any():
        return -1, np.nan
    cols = np.nonzero(ok)[0]
    c = int(cols[np.argmax(s[cols])])                     # (argmax returns the first of equal values)
    return c, s[c]


def mix(logits, trg, key, step, *, pad, banned=(), p_max, start=0, ramp=0, pick=ARGMAX, inv_t=1.0, seed=0):
    """The definition.  logits (B * T, V) float32.  Returns a dict: mixed (B, T) int64, stats (3,) int64, coin (B, T) bool (eligible and
    u < p), replaced (B, T) bool, score (B, T) float64 (the winning score, NaN where gold stays), and for SAMPLE s / E (B, T, V) float64
    of the rows at t - 1 (rows of positions whose coin did not fall are left 0)."""
    trg = np.asarray(trg, dtype=np.int64)
    B, T = trg.shape
    V = logits.shape[1]
    p = prob(step, p_max, start, ramp)
    u = coin(seed, step, key, T)
    eligible = (np.arange(T)[None, :] >= 1) & (trg != pad)
    fell = eligible & (u < p)
    ok = admitted(V, pad, banned)
    mixed, replaced, score = trg.copy(), np.zeros((B, T), bool), np.full((B, T), np.nan)
    out = dict(p=p, coin=fell)
    if pick == SAMPLE:
        kb = column_bits(seed, step, key, T, V)
        S, E = np.zeros((B, T, V)), np.zeros((B, T, V))
    for b in range(B):
        for t in range(T):
            if not fell[b, t]:
                continue
            z = logits[b * T + t - 1]
            if pick == SAMPLE:
                S[b, t], E[b, t] = scores64(z, inv_t, kb[b, t])
                s = S[b, t]
            else:
                s = z.astype(np.float64)
            c, sc = pick_row(s, ok)
            if c >= 0:
                mixed[b, t], replaced[b, t], score[b, t] = c, True, sc
    if pick == SAMPLE:
        out.update(s=S, E=E)
    out.update(mixed=mixed, replaced=replaced, score=score,
               stats=np.array([eligible.sum(), replaced.sum(), (replaced & (mixed != trg)).sum()], dtype=np.int64))
    return out


# ---- the GPU cases: B <= 4, T <= 8, V below and above one pass of 256 threads, no multiple of 4, and past 4096
class Case:
    def __init__(self, name, B, T, V, pick, p_max=1.0, ldx=None, offset=0, pad=1, banned=(2,), step=3, start=0, ramp=0, temperature=1.0,
                 seed=0, plant=()):
        self.name, self.B, self.T, self.V, self.pick, self.p_max = name, B, T, V, pick, p_max
        self.ldx = V if ldx is None else ldx               # row stride in floats; columns V..ldx-1 hold NaN
        self.offset = offset                               # floats between a 16-byte boundary and the first row (1..3: the scalar path)
        self.pad, self.banned, self.step, self.start, self.ramp = pad, tuple(banned), step, start, ramp
        self.inv_t, self.seed, self.plant = F(1.0 / temperature), seed, tuple(plant)

    def kw(self):
        return dict(pad=self.pad, banned=self.banned, p_max=self.p_max, start=self.start, ramp=self.ramp, pick=self.pick, inv_t=self.inv_t,
                    seed=self.seed)

    def data(self):
        """(logits (B * T, V) float32, trg (B, T) int64, key (B,) int64): deterministic.  <pad> stands at t = 0 of row 0, at the end of
        every row, and every row starts on <sos> otherwise.  ``plant``: "ties" (the row maximum twice more, once at a lower column),
        "neginf" (rows of -inf), "banned" (the maximum on a banned column and on <pad>), "nan" (a NaN in one row), "posinf"."""
        rs = np.random.RandomState(1000 + self.V * 7 + self.B * 3 + self.T + self.pick)
        B, T, V = self.B, self.T, self.V
        z = (rs.randn(B * T, V) * 3.0).astype(F)
        trg = rs.randint(3, max(4, V), size=(B, T)).astype(np.int64)
        trg[:, 0] = 2
        trg[0, 0] = self.pad
        for b in range(B):
            trg[b, T - 1 - (b % 3):] = self.pad
        key = (rs.randint(0, 1 << 40, size=B).astype(np.int64) << 8) + np.arange(B)
        rows = B * T
        if "ties" in self.plant and V >= 8:
            for r in range(0, rows, 2):
                m = z[r].max() + F(1.0)
                z[r, [V // 2, V // 3, V - 1]] = m
        if "neginf" in self.plant:
            z[1::5] = -np.inf
        if "banned" in self.plant:
            for r in range(2, rows, 3):
                for c in self.banned + (self.pad,):
                    if c < V:
                        z[r, c] = F(1.0e6)
        if "posinf" in self.plant and V >= 8:
            z[3::7, V - 2] = np.inf
        if "nan" in self.plant and V >= 8:
            z[4, V // 2 + 1] = np.nan
        return z, trg, key


CASES = [
    Case("argmax_V1", 2, 4, 1, ARGMAX),
    Case("argmax_V3_all_excluded", 2, 4, 3, ARGMAX, banned=(0, 2)),
    Case("argmax_V3", 3, 5, 3, ARGMAX, banned=(), plant=("neginf",)),
    Case("argmax_V255", 4, 8, 255, ARGMAX, ldx=256, plant=("ties", "neginf", "banned", "nan")),
    Case("argmax_V257_scalar", 4, 8, 257, ARGMAX, ldx=259, offset=1, plant=("ties", "banned", "posinf")),
    Case("argmax_V257_vec_tail", 3, 7, 257, ARGMAX, ldx=260, plant=("ties", "neginf")),
    Case("argmax_V1030", 4, 8, 1030, ARGMAX, ldx=1032, p_max=0.5, plant=("ties", "banned")),
    Case("argmax_V4099", 4, 8, 4099, ARGMAX, ldx=4100, plant=("ties", "neginf", "banned")),
    Case("argmax_V4099_scalar", 2, 8, 4099, ARGMAX, offset=3, p_max=1.0, start=1, ramp=4, plant=("ties",)),
    Case("sample_V1", 2, 4, 1, SAMPLE),
    Case("sample_V3", 3, 5, 3, SAMPLE, banned=(), temperature=0.7),
    Case("sample_V255", 4, 8, 255, SAMPLE, ldx=256, plant=("banned",)),
    Case("sample_V257_scalar", 4, 8, 257, SAMPLE, ldx=259, offset=2, temperature=1.3, plant=("banned", "posinf")),
    Case("sample_V1030", 4, 8, 1030, SAMPLE, ldx=1032, p_max=0.5, seed=12345, plant=("nan",)),
    Case("sample_V4099", 4, 8, 4099, SAMPLE, ldx=4100, temperature=0.5),
    Case("sample_V4099_scalar", 2, 8, 4099, SAMPLE, offset=1, p_max=0.8, start=1, ramp=4, seed=(1 << 40) + 7),
]
