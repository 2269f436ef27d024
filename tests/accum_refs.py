"""Gradient accumulation as include/mtn_hip.h states it for mtn_grad_accum, in numpy float32, operation for operation: the three modes,
a whole window, the float64 value of the definition G = (sum_k w_k g_k) / (sum_k w_k) — and the cases tests/test_accum_kernel_gpu.py
runs, so that tests/test_accum_refs.py can check them without a GPU.  numpy rounds every float32 array operation separately (it never
fuses a multiply into an add), which is what the kernel does with contraction off."""
import numpy as np

FIRST, ADD, LAST = 0, 1, 2                         # MTN_ACCUM_FIRST / _ADD / _LAST
THREADS, GRID_CAP = 256, 2048                      # csrc/gradnorm_common.h: threads per workgroup, the cap of the grid
CAP_ELEMS = 4 * THREADS * GRID_CAP                 # the smallest buffer whose every thread holds one 16-byte vector
SIZES = [1, 3, 4, 5, 1023, 1024, 256 * 1024 + 7, 2 * CAP_ELEMS + 5]
WINDOWS = [2, 3]


def _f32(x):
    return np.asarray(x, dtype=np.float32)


def first(g, w):
    """MTN_ACCUM_FIRST -> (acc, total)."""
    w = np.float32(w)
    return w * _f32(g), w


def add(acc, g, w, total):
    """MTN_ACCUM_ADD -> (acc, total): a multiply, then an add."""
    w = np.float32(w)
    p = w * _f32(g)
    return _f32(acc) + p, np.float32(total) + w


def last(acc, g, w, total):
    """MTN_ACCUM_LAST -> (g, total): inv = (float)(1.0 / (double)t)."""
    w = np.float32(w)
    t = np.float32(total) + w
    with np.errstate(divide="ignore"):
        inv = np.float32(np.float64(1.0) / np.float64(t))
    p = w * _f32(g)
    s = _f32(acc) + p
    with np.errstate(invalid="ignore", over="ignore"):
        return s * inv, t


def window(gs, ws):
    """The launches of one window of K >= 1 micro-steps -> (G, total).  A window of one launches nothing: G is g_1 itself."""
    K = len(gs)
    assert K == len(ws) and K >= 1
    if K == 1:
        return _f32(gs[0]).copy(), np.float32(ws[0])
    with np.errstate(invalid="ignore", over="ignore"):
        acc, total = first(gs[0], ws[0])
        for k in range(1, K - 1):
            acc, total = add(acc, gs[k], ws[k], total)
        return last(acc, gs[K - 1], ws[K - 1], total)


def exact(gs, ws):
    """(the definition in float64, the bound's scale sum_k |w_k g_k| / sum_k w_k in float64)."""
    w = [np.float64(np.float32(x)) for x in ws]
    num = sum(wk * np.asarray(g, dtype=np.float64) for wk, g in zip(w, gs))
    mag = sum(wk * np.abs(np.asarray(g, dtype=np.float64)) for wk, g in zip(w, gs))
    return num / sum(w), mag / sum(w)


# ------------------------------------------------------------------------------------------ the cases of the GPU test
CASES = [dict(id="n%d-K%d" % (n, K), n=n, K=K) for n in SIZES for K in WINDOWS]


def data(case):
    """(gs, ws) of a case: K float32 buffers of N(0, 1) whose elements are scaled by 1, 1e-30 or 1e30 in turn (the same scale at an
    index in every buffer, so that no sum cancels two huge values into noise), one NaN in the middle of g_1 and one inf at the end of
    g_K (the tail, when n % 4 != 0); integer weights in 1..2000, as token counts are."""
    n, K = case["n"], case["K"]
    rng = np.random.default_rng(1000 * n + K)
    scale = np.array([1.0, 1e-30, 1e30], dtype=np.float32)[np.arange(n) % 3]
    gs = [rng.standard_normal(n).astype(np.float32) * scale for _ in range(K)]
    gs[0][n // 2] = np.float32("nan")
    gs[K - 1][n - 1] = np.float32("inf")
    ws = [np.float32(w) for w in rng.integers(1, 2001, size=K)]
    return gs, ws


def same_bytes(got, want):
    """Bit for bit, except that a NaN is a NaN whatever its sign and payload (the hardware's default NaN is not numpy's)."""
    got, want = _f32(got), _f32(want)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.int32), want[~nan].view(np.int32))
