"""Gradient clipping by global norm as include/mtn_hip.h states it for mtn_grad_sumsq / mtn_clip_scale, in numpy and math.fsum: the
norm in float64 (exactly rounded: the square of a float is exact in double and fsum adds without error), the coefficient of
torch.nn.utils.clip_grad_norm_ (its 1e-6 included), the float32 scale and the stats block — and the cases tests/test_clip_kernel_gpu.py
runs, so that tests/test_clip_refs.py can check each case's own condition without a GPU."""
import functools
import math

import numpy as np

THREADS, GRID_CAP = 256, 2048                     # csrc/gradnorm.hip: threads per workgroup, the cap of the grid (= of the partials)
CAP_ELEMS = 4 * THREADS * GRID_CAP                # the smallest buffer whose every thread holds one 16-byte vector
SIZES = [1, 3, 4, 5, 1023, 1025, CAP_ELEMS - 1, CAP_ELEMS + 5, 3 * 2 ** 20 + 7]
INF, NAN = float("inf"), float("nan")


def partials(n):
    """mtn_grad_sumsq_partials."""
    return 0 if n <= 0 else max(1, min(GRID_CAP, ((n >> 2) + THREADS - 1) // THREADS))


def norm_of(x, base=None):
    """sqrt(sum x^2) * |base| in float64, the sum exactly rounded; inf / nan as IEEE addition gives them."""
    sq = np.asarray(x, dtype=np.float64) ** 2
    if np.isnan(sq).any():
        s = NAN
    elif np.isinf(sq).any():
        s = INF
    else:
        s = math.fsum(sq.tolist())
    b = 1.0 if base is None else abs(float(np.float32(base)))
    return math.sqrt(s) * b


def coef_of(norm, max_norm):
    """min(1, max_norm / (norm + 1e-6)) in float64; NaN when the norm is not finite.  max_norm is the float32 the entry point takes."""
    if not math.isfinite(norm):
        return NAN
    return min(1.0, float(np.float32(max_norm)) / (norm + 1e-6))


def scale_of(coef, base=None):
    """The float32 Adam multiplies by: the base's own bits (1.0f without one) when coef == 1, else (float)(base * coef), rounded once."""
    b = np.float32(1.0 if base is None else base)
    if coef == 1.0:
        return b
    return np.float32(np.float64(b) * np.float64(coef))


def stats_update(stats, norm, coef):
    """One call's update of the five doubles, in place; returns them."""
    if math.isfinite(norm):
        stats[0] += norm
        stats[1] = max(stats[1], norm)
    else:
        stats[4] += 1.0
    stats[2] += 1.0
    if coef < 1.0:
        stats[3] += 1.0
    return stats


def clip(x, max_norm, base=None):
    """(norm, coef, scale) of one call."""
    norm = norm_of(x, base)
    coef = coef_of(norm, max_norm)
    return norm, coef, scale_of(coef, base)


# ------------------------------------------------------------------------------------------ the cases of the GPU test
def _case(n, kind, scale, factor, base=None):
    """max_norm = factor * sqrt(n) * scale (the size of an N(0, scale^2) buffer's norm) as a float32; factor inf = measure only."""
    approx = math.sqrt(n) * scale * (1.0 if base is None else abs(base))
    c = INF if factor == INF else float(np.float32(factor * (approx if kind != "zeros" else 1.0)))
    name = "n%d-%s-s%g-f%g%s" % (n, kind, scale, factor, "" if base is None else "-b%g" % base)
    return dict(id=name, n=n, kind=kind, scale=scale, max_norm=c, base=base)


def _cases():
    out, k = [], 0
    for n in SIZES:
        for scale in (1.0, 1e-25, 1e25):
            out.append(_case(n, "randn", scale, (0.5, 2.0, INF)[k % 3]))
            k += 1
        k += 1                                      # every size sees another rotation of the three factors
    out += [_case(1025, "randn", 1.0, 0.5, base=0.125), _case(1025, "randn", 1.0, 2.0, base=-3.0),
            _case(CAP_ELEMS + 5, "randn", 1e25, 0.5, base=-0.015625), _case(CAP_ELEMS + 5, "randn", 1.0, INF, base=0.3)]
    out += [_case(5, "zeros", 1.0, 1.0), _case(CAP_ELEMS + 5, "zeros", 1.0, 1.0, base=0.5)]
    out += [_case(3, "nan", 1.0, 0.5), _case(1025, "nan", 1.0, INF), _case(SIZES[-1], "nan", 1.0, 2.0)]
    out += [_case(4, "inf", 1.0, 0.5), _case(CAP_ELEMS - 1, "inf", 1.0, INF)]
    return out


CASES = _cases()


def data(case):
    """The case's buffer, float32: N(0, 1) from a generator seeded with n, times the scale in float32; one NaN in the middle or one inf at
    the end (the tail, when n % 4 != 0) for those kinds."""
    n = case["n"]
    if case["kind"] == "zeros":
        return np.zeros(n, dtype=np.float32)
    x = np.random.default_rng(n).standard_normal(n).astype(np.float32) * np.float32(case["scale"])
    if case["kind"] == "nan":
        x[n // 2] = np.float32(NAN)
    if case["kind"] == "inf":
        x[n - 1] = np.float32(INF)
    return x


@functools.lru_cache(maxsize=None)
def expected(case_id):
    """(norm, coef, scale) of a case, computed once per process."""
    case = next(c for c in CASES if c["id"] == case_id)
    return clip(data(case), case["max_norm"], case["base"])
