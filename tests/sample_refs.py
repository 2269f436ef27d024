"""The sampling decode's definitions (include/mtn_hip.h mtn_sample_rows) restated in numpy: the counter hash in integer arithmetic
(bit-exact with the kernel's), the ban / temperature / top-k / top-p filter and the draw in float64, and ``admissible``: the tokens a
correct implementation may return when its arithmetic is only eps-close to float64."""
import numpy as np

M32 = 0xFFFFFFFF
DROP_HI_MUL = 0x9E3779B1


def mix32(x):
    x = np.asarray(x, dtype=np.uint64) & M32
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & M32
    x ^= x >> 16
    return x


def sample_hash(seed, key, pos):
    """32-bit hash of (seed, key, position); seed / key: (signed or unsigned) 64-bit integers, broadcast against each other."""
    seed = np.asarray(seed).astype(np.int64).view(np.uint64) if np.ndim(seed) else np.uint64(int(seed) & 0xFFFFFFFFFFFFFFFF)
    key = np.asarray(key, dtype=np.int64).view(np.uint64) if np.ndim(key) else np.uint64(int(key) & 0xFFFFFFFFFFFFFFFF)
    pos = np.asarray(pos, dtype=np.uint64) & M32
    k0 = mix32((seed & M32) ^ 0x9E3779B9)
    k1 = mix32(((seed >> 32) + 0x85EBCA6B + 0x165667B1) & M32)
    r = mix32((((key & M32) ^ k0) + ((key >> 32) * DROP_HI_MUL & M32) + k1) & M32)
    return mix32((r + (pos * 0x9E3779B1 & M32) + 0x7F4A7C15) & M32)


def uniform24(seed, key, pos):
    """u in [0, 1): the hash's top 24 bits / 2^24 (exact in float32 and float64)."""
    return (sample_hash(seed, key, pos) >> 8).astype(np.float64) / 16777216.0


class Params:
    def __init__(self, temperature=1.0, top_k=0, top_p=1.0, banned=(), eos=-1, min_len=0):
        self.temperature, self.top_k, self.top_p = float(temperature), int(top_k), float(top_p)
        self.banned, self.eos, self.min_len = tuple(int(b) for b in banned), int(eos), int(min_len)

    def banned_at(self, position):
        return set(self.banned) | ({self.eos} if (position < self.min_len and self.eos >= 0) else set())


def _masses(logp_row, params, position):
    """x (float64, banned at -inf) and e = exp((x - max) / T) (0 where banned)."""
    x = np.asarray(logp_row, dtype=np.float64).copy()
    for b in params.banned_at(position):
        if 0 <= b < x.size:
            x[b] = -np.inf
    e = np.where(np.isfinite(x), np.exp((x - x.max()) / params.temperature), 0.0)
    return x, e


def filtered(logp_row, params, position=0):
    """The float64 filter: probabilities over the kept set (0 elsewhere), summing to 1."""
    x, e = _masses(logp_row, params, position)
    keep = np.isfinite(x)
    if 0 < params.top_k < x.size:
        kth = np.sort(x)[::-1][params.top_k - 1]
        keep &= x >= kth
    e = np.where(keep, e, 0.0)
    if params.top_p < 1.0:
        # i stays iff the mass strictly above it is below top_p x mass  (<=> p_i >= t*, t* the largest threshold whose mass reaches top_p)
        order = np.argsort(-e, kind="stable")
        es = e[order]
        csum = np.cumsum(es)
        first_of_value = np.searchsorted(-es, -es, side="left")                 # index of the first element equal to es[j]
        above = np.where(first_of_value > 0, csum[np.maximum(first_of_value - 1, 0)], 0.0)
        stay = above < params.top_p * csum[-1]
        k2 = np.zeros_like(keep)
        k2[order] = stay
        e = np.where(k2 & keep, e, 0.0)
    return e / e.sum()


def draw(p, u):
    """The first index whose running mass exceeds u x mass."""
    c = np.cumsum(p)
    i = int(np.searchsorted(c, u * c[-1], side="right"))
    return min(i, int(np.nonzero(p)[0][-1]))


def admissible(logp_row, u, params, eps, position=0):
    """The set of tokens a correct implementation may return for this row and u when its log-probabilities, the top-k / top-p
    thresholds and the running masses are only eps-close to float64.  eps = 0: the single token of the definition.
    A token within eps of the top-k threshold (in log-probability) or of the top-p threshold (in mass fraction) is OPTIONAL; token
    i may be returned if, for some choice of the optional tokens, u lies within eps of [mass before i, mass through i) / mass."""
    exact = draw(filtered(logp_row, params, position), u)
    if eps == 0:
        return {exact}
    x, e = _masses(logp_row, params, position)
    alive = np.isfinite(x)
    sure, maybe = alive.copy(), np.zeros_like(alive)
    if 0 < params.top_k < x.size:
        kth = np.sort(x)[::-1][params.top_k - 1]
        # (no token within eps below the threshold: nothing can trade places with the k-th, the exact set stands)
        contested = bool((alive & (x < kth) & (x >= kth - eps)).any())
        sure = alive & (x >= (kth + eps if contested else kth))
        maybe = alive & (x >= kth - eps) & ~sure
    if params.top_p < 1.0:
        # fraction of the mass strictly above i: its smallest and largest plausible value
        order = np.argsort(-x, kind="stable")
        xs = x[order]
        e_sure, e_any = np.where(sure, e, 0.0)[order], np.where(sure | maybe, e, 0.0)[order]
        cs_sure, cs_any = np.concatenate([[0.0], np.cumsum(e_sure)]), np.concatenate([[0.0], np.cumsum(e_any)])
        n_hi = np.searchsorted(-xs, -(xs - eps), side="right")     # count of x_j >= x_i - eps  (i and its near-ties included)
        n_lo = np.searchsorted(-xs, -(xs + eps), side="left")      # count of x_j > x_i + eps
        ei = e[order]
        a_hi = cs_any[n_hi] - ei * (sure | maybe)[order]            # everything plausibly above (near-ties included), i itself not
        a_lo = cs_sure[n_lo]
        g_hi = a_hi / np.maximum(a_hi + (cs_sure[-1] - cs_sure[n_hi]) + ei, 1e-300)
        g_lo = a_lo / np.maximum(a_lo + (cs_any[-1] - cs_any[n_lo]), 1e-300)
        p_sure, p_maybe = np.zeros_like(alive), np.zeros_like(alive)
        p_sure[order] = g_hi < params.top_p - eps
        p_maybe[order] = g_lo < params.top_p + eps
        maybe = (sure | maybe) & p_maybe & ~(sure & p_sure)
        sure = sure & p_sure
    m_sure, m_any = np.where(sure, e, 0.0), np.where(sure | maybe, e, 0.0)
    b_lo, b_hi = np.cumsum(m_sure) - m_sure, np.cumsum(m_any) - m_any              # mass before i
    aft_lo, aft_hi = m_sure.sum() - np.cumsum(m_sure), m_any.sum() - np.cumsum(m_any)  # mass behind i
    lo = b_lo / np.maximum(b_lo + e + aft_hi, 1e-300) - eps
    hi = (b_hi + e) / np.maximum(b_hi + e + aft_lo, 1e-300) + eps
    ok = (sure | maybe) & (e > 0) & (lo <= u) & (u <= hi)
    return set(int(i) for i in np.nonzero(ok)[0]) | {exact}
