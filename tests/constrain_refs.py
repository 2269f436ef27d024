"""The definitions of constrained decoding (include/mtn_hip.h mtn_constrain_rows) in numpy: what csrc/constrain.hip must give bit for bit.
The transform is one float32 multiply and -inf writes, so these references are exact by construction: no tolerance anywhere."""
import numpy as np


def constrain_row(logp_f32, hist, ngram, theta):
    """One row of fp32 log-probabilities under the history ``hist`` (generated tokens, oldest first, no <sos>): every distinct token of
    the history is multiplied by float32(theta) once (theta == 1: off), then every token that would complete a second occurrence of an
    ``ngram``-gram is set to -inf (ngram == 0: off; a ban overrides the penalty).  Tokens outside [0, V) take part in the comparisons
    but name no column.  Returns a new float32 array; every other column keeps its bits."""
    x = np.asarray(logp_f32)
    assert x.dtype == np.float32 and x.ndim == 1
    out = x.copy()
    V = x.shape[0]
    h = [int(t) for t in hist]
    n, N = len(h), int(ngram)
    th = np.float32(theta)
    if th != np.float32(1.0):
        for c in sorted(set(h)):
            if 0 <= c < V:
                out[c] = np.float32(x[c]) * th
    if N >= 1 and n >= N - 1:
        suffix = h[n - N + 1:] if N > 1 else []
        for j in range(0, n - N + 1):
            if h[j:j + N - 1] == suffix:
                c = h[j + N - 1]
                if 0 <= c < V:
                    out[c] = -np.inf
    return out


def history_from_log(log_tok, log_parent, step, row, width):
    """The history of ``row`` out of a search's step log, as the host rebuilds a hypothesis: log_tok / log_parent are (L, rows) arrays
    (log_parent None: every row is its own parent), parents relative to the first row of the row's group of ``width``; ``step`` is the
    number of tokens generated so far (clamped to [0, L]), every parent is clamped to [0, width)."""
    L = log_tok.shape[0]
    l = min(max(int(step), 0), L)
    base, r = row - row % width, row % width
    h = [0] * l
    for j in range(l - 1, -1, -1):
        h[j] = int(log_tok[j][base + r])
        if log_parent is not None:
            r = min(max(int(log_parent[j][base + r]), 0), width - 1)
    return h


def has_repeated_ngram(tokens, N):
    """True if some N consecutive tokens occur twice in ``tokens`` (overlapping occurrences count)."""
    toks = [int(t) for t in tokens]
    seen = set()
    for j in range(len(toks) - N + 1):
        g = tuple(toks[j:j + N])
        if g in seen:
            return True
        seen.add(g)
    return False
