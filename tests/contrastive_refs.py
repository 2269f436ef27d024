"""numpy form of contrastive search as include/mtn_hip.h mtn_contrastive_advance defines it, in float64: `penalties` / `scores` / `winner`
are the pieces of one dialogue's step, `advance` is one launch on the device layout (what csrc/contrastive.hip reads and writes), and a
`State` carried through several `advance` calls is the state machine.  `bound` is the distance allowed between the kernel's fp32 score and
this float64 one, `cos_bound` its cosine part; `emulate_f32` computes the scores in numpy float32 with the kernel's summation order (every
multiply and add rounded, where the kernel fuses them: an emulation of fp32 arithmetic, not of the kernel's bits; the bound is held to it on
the CPU).  `GPU_CASES` / `make_case` are the inputs of tests/test_contrastive_kernel_gpu.py; tests/test_contrastive_refs.py
asserts that every one of their steps is decided by a margin of at least 4 bounds."""
import numpy as np

U = 2.0 ** -24          # unit roundoff of float32


def cos_bound(d):
    """|fp32 cosine - float64 cosine|: a dot product in any order errs by at most d u |a||b|, each norm by at most (d / 2 + 1) u relatively,
    two square roots, a product and a division by a few u more: (2 d + 8) u."""
    return (2 * d + 8) * U


def bound(alpha, d):
    """|s_r - float64 s_r|: expf plus one multiply errs by at most 4 u at p <= 1, the penalty by its cosine bound."""
    return ((1.0 - alpha) * 4 + alpha * (2 * d + 8)) * U


def penalties(h, l):
    """h (k, L, d) states of a dialogue's rows -> (k,) float64: pen_r = max over j < l of cos(h[r][l], h[r][j]); 0 where a norm is 0; NaN
    where any cosine is NaN."""
    h = np.asarray(h, dtype=np.float64)
    c, p = h[:, l], h[:, :l]
    with np.errstate(invalid="ignore", divide="ignore"):
        dot = np.einsum("kd,kjd->kj", c, p)
        nc, npj = np.sqrt((c * c).sum(-1))[:, None], np.sqrt((p * p).sum(-1))
        cos = np.where((nc == 0) | (npj == 0), 0.0, dot / (nc * npj))
    return cos.max(axis=1)                                         # (np.max keeps a NaN)


def scores(alpha, cand_logp, pen):
    a = float(np.float32(alpha))
    with np.errstate(invalid="ignore"):
        return (1.0 - a) * np.exp(np.asarray(cand_logp, dtype=np.float64)) - a * np.asarray(pen, dtype=np.float64)


def winner(s, cand_logp):
    """(r*, margin): the row of largest score among the rows that can win (score not NaN, cand_logp not -inf), ties to the lowest row, row 0
    if none can; margin = its score minus the largest score strictly below it (inf without one).  Rows with equal float64 scores are rows
    with identical inputs in every case here — the rule decides them, no rounding does."""
    ok = ~np.isnan(s) & ~np.isneginf(np.asarray(cand_logp, dtype=np.float64))
    if not ok.any():
        return 0, np.inf
    best = s[ok].max()
    r = int(np.flatnonzero(ok & (s == best))[0])
    below = s[ok & (s < best)]
    return r, (best - below.max() if below.size else np.inf)


class State:
    """The device state of D dialogues of k rows: tokens (D * k, L) int64, pos, cand_logp (D * k,) float32, step / done (D,) int32 and the
    four logs (L, D); log_pen is float64 here (the kernel's is compared within cos_bound).  margins[(l, dialogue)] is each scored step's
    margin."""

    def __init__(self, D, k, L, pad=1):
        self.D, self.k, self.L = D, k, L
        self.tokens = np.full((D * k, L), pad, dtype=np.int64)
        self.pos = 0
        self.cand_logp = np.zeros(D * k, dtype=np.float32)
        self.step, self.done = np.zeros(D, dtype=np.int32), np.zeros(D, dtype=np.int32)
        self.log_tok, self.log_rank = np.zeros((L, D), dtype=np.int32), np.zeros((L, D), dtype=np.int32)
        self.log_logp, self.log_pen = np.zeros((L, D), dtype=np.float32), np.zeros((L, D), dtype=np.float64)
        self.margins = {}

    def copy(self):
        c = State.__new__(State)
        for name, v in self.__dict__.items():
            setattr(c, name, v.copy() if hasattr(v, "copy") else v)
        return c


def deal(head, k, l, eos, min_len, banned):
    """head (2 * k_top + 1,) -> (columns (k,), values (k,) float32): the first k admitted entries, then the last admitted column at -inf."""
    k_top = (len(head) - 1) // 2
    adm = [(int(head[k_top + i]), np.float32(head[i])) for i in range(k_top)
           if int(head[k_top + i]) not in banned and not (int(head[k_top + i]) == eos and l < min_len)]
    last = adm[-1][0] if adm else int(head[k_top])
    adm = adm[:k] + [(last, np.float32(-np.inf))] * (k - len(adm))
    return np.array([a[0] for a in adm], dtype=np.int64), np.array([a[1] for a in adm], dtype=np.float32)


def advance(st, hidden, top, *, alpha, eos, min_len, banned=()):
    """One launch: hidden (D * k, L, d) and top (D * k, 2 * k_top + 1) float32; ``st`` is advanced in place."""
    D, k, L = st.D, st.k, st.L
    banned = tuple(int(b) for b in banned)
    for dlg in range(D):
        l, base = int(st.step[dlg]), dlg * k
        st.step[dlg] = l + 1
        if dlg == 0:
            st.pos = min(max(l + 1, 0), L - 1)
        if st.done[dlg] or not 0 <= l < L:
            continue
        r, more = 0, l + 1 < L
        if l >= 1:
            pen = penalties(hidden[base:base + k], l)
            s = scores(alpha, st.cand_logp[base:base + k], pen)
            r, st.margins[(l, dlg)] = winner(s, st.cand_logp[base:base + k])
            y = int(st.tokens[base + r, l])
            st.log_tok[l, dlg], st.log_logp[l, dlg], st.log_pen[l, dlg], st.log_rank[l, dlg] = y, st.cand_logp[base + r], pen[r], r
            st.tokens[base:base + k, l] = y
            if y == eos:
                st.done[dlg], more = 1, False
        if more:
            st.tokens[base:base + k, l + 1], st.cand_logp[base:base + k] = deal(top[base + r], k, l, eos, min_len, banned)
    return st


def response(log_tok, log_logp, dlg, eos, penalty=0.0):
    """(tokens up to <eos>, score, number of logged steps used) of dialogue ``dlg`` from the logs of a whole search: score = sum of the chosen
    tokens' log-probabilities, <eos> included, + penalty * (length + 1) — a finished sample's formula."""
    col = [int(t) for t in log_tok[1:, dlg]]
    n = col.index(eos) if eos in col else len(col)
    used = n + 1 if eos in col else n
    return col[:n], float(np.asarray(log_logp[1:1 + used, dlg], dtype=np.float64).sum()) + penalty * (n + 1), used


def emulate_f32(h, l, alpha, cand_logp):
    """(scores, penalties) of a dialogue's rows in numpy float32, sums in the kernel's order (but each product rounded before it is added,
    where the kernel's fmaf rounds once): lane `lane` of a wave owns elements
    4 * (lane + 64 t) + c, adds them chunk by chunk, component by component, and the 64 lanes are summed by an xor butterfly."""
    f = np.float32
    h = np.asarray(h, dtype=f)
    k, _, d = h.shape

    def wsum(x, y):
        part = np.zeros(64, dtype=f)
        for t in range((d + 255) // 256):
            for c in range(4):
                e = 4 * (np.arange(64) + 64 * t) + c
                m = e < d
                part[m] = (part[m] + (x[e[m]] * y[e[m]]).astype(f)).astype(f)
        for o in (32, 16, 8, 4, 2, 1):
            part = (part + part[np.arange(64) ^ o]).astype(f)
        return part[0]

    pen = np.zeros(k, dtype=f)
    for r in range(k):
        cn = wsum(h[r, l], h[r, l])
        cs = []
        for j in range(l):
            hn = wsum(h[r, j], h[r, j])
            cs.append(f(0) if cn == 0 or hn == 0 else f(wsum(h[r, l], h[r, j]) / f(np.sqrt(cn) * np.sqrt(hn))))
        pen[r] = max(cs)
    a = f(alpha)
    s = (((f(1) - a) * np.exp(np.asarray(cand_logp, dtype=f))).astype(f) - (a * pen).astype(f)).astype(f)
    return s, pen


# ---------------------------------------------------------------- the GPU cases
# name, dialogues, k, L, d, alpha, first step, launches, extra elements per row / position of hidden, vocabulary, seed, what is special
def _case(name, D, k, L, d, alpha, l0, n, seed, row_pad=0, pos_pad=0, V=1000, eos=2, min_len=1, banned=(), k_top=None, special=None):
    k_top = min(16, k + len(banned) + 1) if k_top is None else k_top
    return dict(name=name, D=D, k=k, L=L, d=d, alpha=alpha, l0=l0, n=n, seed=seed, row_pad=row_pad, pos_pad=pos_pad, V=V, eos=eos,
                min_len=min_len, banned=tuple(banned), k_top=k_top, special=special)


GPU_CASES = [
    # six chained launches from the bootstrap, every d x k; odd strides on the scalar path, strides in multiples of 4 on the 16-byte path
    _case("d8_k1", 3, 1, 9, 8, 0.6, 0, 6, 0), _case("d8_k2", 1, 2, 9, 8, 0.6, 0, 6, 1, pos_pad=4), _case("d8_k5", 3, 5, 9, 8, 0.5, 0, 6, 2, row_pad=8),
    _case("d8_k16", 3, 16, 9, 8, 0.6, 0, 6, 3, row_pad=4, pos_pad=4),
    _case("d20_k1", 1, 1, 9, 20, 0.6, 0, 6, 4, pos_pad=3), _case("d20_k2", 3, 2, 9, 20, 0.4, 0, 6, 5, row_pad=5, pos_pad=1),
    _case("d20_k5", 3, 5, 9, 20, 0.6, 0, 6, 6), _case("d20_k16", 1, 16, 9, 20, 0.6, 0, 6, 7, row_pad=7),
    _case("d128_k1", 3, 1, 9, 128, 0.6, 0, 6, 8, row_pad=4), _case("d128_k2", 3, 2, 9, 128, 0.6, 0, 6, 9, pos_pad=2),
    _case("d128_k5", 1, 5, 9, 128, 0.7, 0, 6, 10, pos_pad=8), _case("d128_k16", 3, 16, 9, 128, 0.6, 0, 6, 11),
    _case("d512_k1", 1, 1, 9, 512, 0.6, 0, 6, 12), _case("d512_k2", 3, 2, 9, 512, 0.6, 0, 6, 13, row_pad=12, pos_pad=4),
    _case("d512_k5", 3, 5, 9, 512, 0.6, 0, 6, 14), _case("d512_k16", 3, 16, 9, 512, 0.3, 0, 6, 15, pos_pad=1),
    # d no multiple of 4: the scalar path's zero-filled tail of the last 4-element group
    _case("d10_k5", 3, 5, 9, 10, 0.6, 0, 6, 35, pos_pad=1), _case("d21_k2", 3, 2, 9, 21, 0.6, 0, 6, 36), _case("d7_k16", 1, 16, 9, 7, 0.5, 0, 6, 37, row_pad=3),
    # L = 2, 9, 33 at l = 0, 1, L - 2, L - 1 (the last launch writes no candidates, the one after it only advances the step)
    _case("L2_l0", 3, 5, 2, 128, 0.6, 0, 3, 16), _case("L2_l1", 3, 5, 2, 20, 0.6, 1, 2, 17),
    _case("L9_l1", 3, 5, 9, 512, 0.6, 1, 1, 18), _case("L9_l7", 3, 5, 9, 128, 0.6, 7, 3, 19), _case("L9_l8", 1, 2, 9, 8, 0.6, 8, 2, 20),
    _case("L33_l0", 1, 5, 33, 128, 0.6, 0, 2, 21), _case("L33_l1", 3, 2, 33, 512, 0.6, 1, 2, 22),
    _case("L33_l31", 3, 5, 33, 512, 0.6, 31, 3, 23, pos_pad=4), _case("L33_l32", 3, 16, 33, 20, 0.6, 32, 2, 24),
    # the rules
    _case("eos_done", 3, 5, 9, 128, 0.6, 3, 3, 25, special="eos_chosen"),
    _case("eos_barred", 3, 5, 9, 128, 0.6, 2, 3, 26, min_len=4, special="eos_heads"),
    _case("eos_allowed", 3, 5, 9, 128, 0.0, 2, 3, 27, min_len=2, special="eos_heads"),
    _case("banned", 3, 5, 9, 20, 0.6, 0, 6, 28, banned=(7, 11, 13, 17), special="banned_heads"),
    _case("few_admitted", 3, 16, 9, 128, 0.6, 0, 4, 29, banned=(7, 11), min_len=9, k_top=16, special="banned_heads"),
    _case("tie", 3, 5, 9, 512, 0.1, 4, 2, 30, special="tie"),
    _case("alpha0", 3, 5, 9, 128, 0.0, 0, 6, 31), _case("alpha1", 3, 5, 9, 128, 1.0, 0, 6, 32),
    _case("nan_row", 3, 5, 9, 128, 0.1, 4, 2, 33, special="nan"),
    _case("short_head", 3, 5, 9, 20, 0.6, 0, 6, 34, V=3, eos=-1, k_top=6, special="short_head"),
]


def make_case(c):
    """(initial State, [(hidden (D * k, L, d) float32, top (D * k, 2 * k_top + 1) float32) per launch], eos) of a case — a pure function of it.
    States are a per-row direction scaled per position plus noise, so cosines spread over (-1, 1); heads are sorted log-probabilities of a
    random distribution over distinct columns.  The state is as l0 steps would have left it: a common random prefix per dialogue, distinct
    candidates at position l0 with descending cand_logp."""
    rng = np.random.default_rng(1000 + c["seed"])
    D, k, L, d, V, k_top, l0, sp = c["D"], c["k"], c["L"], c["d"], c["V"], c["k_top"], c["l0"], c["special"]
    W, eos = D * k, c["eos"]
    lo = 20 if V > 40 else 0                                       # ordinary columns stay clear of <eos> and the banned ids

    def logps(n):
        p = np.sort(rng.dirichlet(np.full(n + 1, 0.7)))[::-1][:n]
        return np.log(np.maximum(p, 1e-6)).astype(np.float32)

    st = State(D, k, L)
    st.step[:] = l0
    st.pos = min(l0, L - 1)
    st.tokens[:, 0] = 0
    for dlg in range(D):
        rows = slice(dlg * k, dlg * k + k)
        if l0 >= 1:
            st.tokens[rows, 1:l0] = rng.integers(lo, V, size=l0 - 1)[None, :]
            st.tokens[rows, l0] = lo + rng.permutation(V - lo)[:k] if V - lo >= k else rng.integers(0, V, size=k)
            st.cand_logp[rows] = logps(k)
    launches = []
    for i in range(c["n"]):
        direction, scale = rng.standard_normal((W, 1, d)), rng.uniform(-1.0, 1.5, size=(W, L, 1))
        hidden = (direction * scale + 0.6 * rng.standard_normal((W, L, d))).astype(np.float32)
        top = np.zeros((W, 2 * k_top + 1), dtype=np.float32)
        for r in range(W):
            n = min(k_top, V)
            top[r, :n] = logps(n)
            top[r, n:k_top] = -np.inf                              # fewer than k_top columns: (-inf, column 0), as mtn_topk_rows fills
            top[r, k_top:k_top + n] = lo + rng.permutation(V - lo)[:n]
            if sp == "eos_heads":
                top[r, k_top] = eos                                # <eos> is every row's most probable next token
            if sp == "banned_heads":
                top[r, k_top + 1], top[r, k_top + 2] = c["banned"][0], c["banned"][1]
                top[r, k_top + 4] = eos
            top[r, 2 * k_top] = rng.standard_normal()
        if i == 0 and sp == "tie":                                 # rows 0 and 1 of every dialogue: the same state, the same probability
            for dlg in range(D):
                hidden[dlg * k + 1] = hidden[dlg * k]
                st.cand_logp[dlg * k + 1] = st.cand_logp[dlg * k]
        if i == 0 and sp == "nan":                                 # the most probable row holds a NaN, the next one cannot win either
            for dlg in range(D):
                hidden[dlg * k, l0, d // 2] = np.nan
                st.cand_logp[dlg * k + 1] = -np.inf
        launches.append((hidden, top))
    if sp == "eos_chosen":                                         # <eos> is the token the middle dialogue chooses at the first launch
        probe = advance(st.copy(), *launches[0], alpha=c["alpha"], eos=-1, min_len=c["min_len"], banned=c["banned"])
        eos = int(probe.log_tok[l0, D // 2])
    return st, launches, eos


def run_case(c):
    """The reference state after every launch of a case: [State, ...] (the initial one first)."""
    st, launches, eos = make_case(c)
    states = [st.copy()]
    for hidden, top in launches:
        advance(st, hidden, top, alpha=c["alpha"], eos=eos, min_len=c["min_len"], banned=c["banned"])
        states.append(st.copy())
    return states
