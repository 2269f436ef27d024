"""mtn_ensemble_rows' definitions (include/mtn_hip.h) restated in float64 with numpy, the same closed form in float32 with torch on the CPU,
and the case list of tests/test_ensemble_kernel_gpu.py; validated without a GPU by tests/test_ensemble_refs.py.  Plain helpers, no fixtures.

With x_m the row of member m, w_m >= 0 its weight (sum 1) and lse_m = logsumexp_c x_m[c]:

    prob     out[c] = log sum_m w_m exp(x_m[c] - lse_m)        as max_m a_m + log sum_m exp(a_m - max), a_m = log w_m + x_m[c] - lse_m
    logprob  s[c] = sum_{m: w_m > 0} w_m (x_m[c] - lse_m);  out[c] = s[c] - logsumexp_c s[c]

    w_m == 0   the member contributes nothing in either mode, whatever its entries (it is dropped: no 0 * inf)
    -inf       prob: the entry contributes 0; a column that is -inf in every weighted member gives -inf
               logprob: a -inf entry in any weighted member gives -inf
    Every weighted member row holds at least one finite entry (a precondition, not checked).
"""
from collections import namedtuple

import numpy as np
import torch

MODES = ("prob", "logprob")
EnsCase = namedtuple("EnsCase", "rows M V lds weights inputs")
ENS_SEED = 4000
CASES = [
    EnsCase(1, 1, 1, (1,), "uniform", "logits"),
    EnsCase(1, 2, 3, (3, 5), "skewed", "logits"),
    EnsCase(5, 3, 255, (255, 256, 259), "uniform", "logits"),
    EnsCase(5, 2, 257, (257, 260), "skewed", "identical"),
    EnsCase(16, 3, 1000, (1003, 1003, 1003), "zero", "zero_inf"),
    EnsCase(5, 8, 4099, (4099, 4100, 4101, 4102, 4103, 4104, 4099, 4100), "uniform", "logits"),
    EnsCase(16, 2, 257, (260, 264), "uniform", "neginf"),
    EnsCase(5, 3, 1000, (1003, 1000, 1004), "skewed", "logp"),
    EnsCase(1, 8, 3, (3, 4, 5, 6, 7, 8, 9, 10), "skewed", "neginf"),
    EnsCase(16, 1, 4099, (4100,), "uniform", "logits"),
    EnsCase(5, 3, 1, (1, 2, 4), "zero", "logits"),
    EnsCase(5, 2, 255, (255, 257), "zero", "zero_inf"),
    EnsCase(1, 3, 4099, (4099, 4099, 4099), "skewed", "neginf"),
    EnsCase(16, 8, 255, (256,) * 8, "zero", "identical"),
]


def ens_cases():
    return list(CASES)


def ens_case_id(c):
    return f"r{c.rows}-M{c.M}-V{c.V}-ld{c.lds[0]}-{c.weights}-{c.inputs}"


def ens_weights(case):
    """Normalised float64 weights of a case: uniform; skewed (0.9 for member 0, 0.1 shared by the others); zero (uniform, member 1 at 0)."""
    M = case.M
    if case.weights == "uniform" or M == 1:
        w = np.ones(M)
    elif case.weights == "skewed":
        w = np.array([0.9] + [0.1 / (M - 1)] * (M - 1))
    else:
        w = np.ones(M)
        w[1] = 0.0
    return w / w.sum()


def ens_inputs(case, seed):
    """M float32 (rows, ld_m) tensors from a seeded CPU generator; columns V..ld_m-1 hold NaN (never read).
    logits: uniform in [-40, 40], so one member dominates some columns.  logp: rows already normalised.  identical: member 1 (if any) is a copy
    of member 0.  neginf: member 0 is -inf in the columns c % 3 == 0 and EVERY member in the columns c % 5 == 1 (never in column V - 1: each row
    keeps a finite entry).  zero_inf: member 1 — the zero-weight one of the 'zero' weights — is -inf in every even column."""
    g = torch.Generator().manual_seed(seed)
    rows, M, V = case.rows, case.M, case.V
    cols = torch.arange(V)
    vals = []
    for m in range(M):
        x = (torch.rand(rows, V, generator=g) * 80.0 - 40.0).float()
        if case.inputs == "logp":
            x = torch.log_softmax((torch.randn(rows, V, generator=g) * 4.0).float(), dim=1)
        if case.inputs == "identical" and m == 1:
            x = vals[0].clone()
        if case.inputs == "neginf":
            if m == 0:
                x[:, (cols % 3 == 0) & (cols != V - 1)] = float("-inf")
            x[:, (cols % 5 == 1) & (cols != V - 1)] = float("-inf")
        if case.inputs == "zero_inf" and m == 1:
            x[:, cols % 2 == 0] = float("-inf")
        vals.append(x)
    out = []
    for m, x in enumerate(vals):
        buf = torch.full((rows, case.lds[m]), float("nan"))
        buf[:, :V] = x
        out.append(buf)
    return out


def _lse(x, xp):
    mx = x.max(-1, keepdims=True) if xp is np else x.max(-1, keepdim=True).values
    return mx + xp.log(xp.exp(x - mx).sum(-1, keepdims=True) if xp is np else xp.exp(x - mx).sum(-1, keepdim=True))


def ensemble_ref64(xs, w, mode):
    """float64 numpy: xs = M arrays (rows, V), w normalised weights -> (rows, V)."""
    xs = [np.asarray(x, dtype=np.float64) for x in xs]
    w = np.asarray(w, dtype=np.float64)
    keep = [m for m in range(len(xs)) if w[m] > 0]
    ninf = -np.inf
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        lp = [xs[m] - _lse(xs[m], np) for m in keep]
        if mode == "prob":
            a = np.stack([np.log(w[m]) + l for m, l in zip(keep, lp)])
            mx = a.max(0)
            safe = np.where(np.isfinite(mx), mx, 0.0)
            return np.where(np.isfinite(mx), safe + np.log(np.exp(a - safe).sum(0)), ninf)
        s = np.zeros_like(lp[0])
        for m, l in zip(keep, lp):
            s = s + w[m] * l
        fin = np.isfinite(s)
        mx = np.where(fin, s, ninf).max(-1, keepdims=True)
        ls = mx + np.log(np.where(fin, np.exp(np.where(fin, s, 0.0) - mx), 0.0).sum(-1, keepdims=True))
        return np.where(fin, s - ls, ninf)


def closed_form_f32(xs, w, mode):
    """The same closed form in float32 with torch on the CPU (weights rounded to float32, as the kernel receives them).  Not a reference:
    the yardstick for what float32 delivers on these formulas."""
    w32 = [float(np.float32(v)) for v in w]
    keep = [m for m in range(len(xs)) if w32[m] > 0]
    xs = [torch.as_tensor(x).float() for x in xs]
    ninf = torch.tensor(float("-inf"))
    lp = [xs[m] - _lse(xs[m], torch) for m in keep]
    if mode == "prob":
        a = torch.stack([l + float(np.float32(np.log(w32[m]))) for m, l in zip(keep, lp)])
        mx = a.max(0).values
        fin = torch.isfinite(mx)
        safe = torch.where(fin, mx, torch.zeros_like(mx))
        return torch.where(fin, safe + torch.exp(a - safe).sum(0).log(), ninf)
    s = torch.zeros_like(lp[0])
    for m, l in zip(keep, lp):
        s = s + w32[m] * l
    fin = torch.isfinite(s)
    mx = torch.where(fin, s, ninf).max(-1, keepdim=True).values
    ls = mx + torch.where(fin, torch.exp(torch.where(fin, s, torch.zeros_like(s)) - mx), torch.zeros_like(s)).sum(-1, keepdim=True).log()
    return torch.where(fin, s - ls, ninf)


def case_views(case, seed):
    """(the M float32 buffers, their (rows, V) float64 numpy views, normalised float64 weights) of a case."""
    bufs = ens_inputs(case, seed)
    return bufs, [b[:, :case.V].double().numpy() for b in bufs], ens_weights(case)


def worst_abs_error(got, ref):
    """Worst |got - ref| over the finite entries of ref (the -inf pattern is compared exactly, elsewhere)."""
    fin = np.isfinite(ref)
    return float(np.abs(np.asarray(got, dtype=np.float64)[fin] - ref[fin]).max()) if fin.any() else 0.0


# What float32 delivers: the worst |closed_form_f32 - ensemble_ref64| over ens_cases() x MODES (seeds ENS_SEED + index), measured with torch on
# a CPU.  logprob on the +-40 logits sets it: s[c] reaches about -80 per weighted member, half an ulp of 80 is 3.8e-6, and lse_m, the products,
# their sum and the final subtraction each round once.  tests/test_ensemble_refs.py re-measures it (within a factor 2: summation order differs
# between CPUs); the GPU test holds the kernel to 4 x this.
CPU_F32_ENSEMBLE_ABS = 1.41e-5
