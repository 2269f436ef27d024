"""float64 references and case lists for the direct tests of the row / optimiser / elementwise kernels
(tests/test_row_kernels_gpu.py); validated without a GPU by tests/test_row_refs.py.  Plain helpers, no fixtures.

Loss head     composed: float64 log_softmax -> oracle.mtn_oracle.label_smoothing_kl per segment -> sum coef / norm; gradient by
              autograd.  `closed_form_f32` evaluates the kernel's closed form (header of csrc/losshead.hip) in float32 with torch on
              the CPU: its error against the composed reference is what the kernel's bounds are derived from.
Adam / Noam   torch.optim.Adam semantics (the formula in csrc/common.h) and the Noam state [step, lr, 1 - b1^t, 1 - b2^t] in float64.
"""
import math
from collections import namedtuple

import torch

from oracle.mtn_oracle import label_smoothing_kl, noam_rate

# ------------------------------------------------------------------------------------------ loss head: cases
# pads: how <pad> targets are placed, applied to every segment unless stated
#   none       no <pad> row
#   tail       <pad> rows at local index > 0 only (zeroed)
#   lone0      one <pad>, at local row 0 (label_smoothing.py:29: NOT zeroed, td = eps on V - 1 columns)
#   zero_plus  <pad> at local row 0 and at another row (both zeroed)
#   lone0_late segment 0 has ordinary (tail) pads, the only <pad> of segment 2 (segment 1 of a two-segment layout) is its row 0
LossCase = namedtuple("LossCase", "V segs ldz_pad ldd_pad pads smoothing scale offset pad")
PAD_KINDS = ("none", "tail", "lone0", "zero_plus", "lone0_late")
COEF = (1.0, 0.7, 0.3, 1.9)
NORM = (7.0, 13.0, 3.0, 29.0)
GLOSS = 0.37


def _lc(V, segs, ldz_pad, ldd_pad, pads, smoothing=0.1, scale=1.0, offset=0.0, pad=1):
    return LossCase(V, tuple(segs), ldz_pad, ldd_pad, pads, smoothing, scale, offset, pad)


def loss_cases():
    """A covering list: every V, layout, ldz, ldd, pad placement, smoothing and (scale, offset) of the issue appears; V = 3000
    and V = 3004 meet every pad placement."""
    L1, L5, L2, L3, L4 = (1,), (5,), (18, 15), (640, 100, 7), (3, 1, 1, 2)
    cases = []
    # V = 3000 / 3004 x every pad placement, layouts / strides / logit statistics rotated
    rot = [(L3, 0, 0, 1.0, 0.0), (L2, 12, 4, 8.0, 0.0), (L4, 0, 60, 1.0, 50.0), (L5, 12, 0, 1.0, -50.0), (L4, 12, 60, 1.0, 0.0)]
    for V in (3000, 3004):
        for k, kind in enumerate(PAD_KINDS):
            segs, zp, dp, s, o = rot[(k + (V == 3004) * 2) % 5]
            if kind == "lone0_late" and len(segs) < 3:
                segs = L3 if V == 3000 else L4
            cases.append(_lc(V, segs, zp, dp, kind, scale=s, offset=o))
    # the other vocabulary sizes: one sweep with idle lanes (8, 104), exactly one sweep (256), one sweep + one float4 (260), multi-sweep
    cases += [
        _lc(8, L1, 0, 0, "none"), _lc(8, L4, 12, 4, "lone0_late", pad=0), _lc(8, L2, 0, 60, "zero_plus", pad=7),
        _lc(104, L2, 0, 0, "tail"), _lc(104, L1, 12, 60, "lone0"), _lc(104, L5, 0, 4, "zero_plus", scale=8.0),
        _lc(256, L5, 12, 0, "tail", offset=50.0), _lc(256, L4, 0, 4, "lone0", pad=255), _lc(256, L3, 0, 60, "lone0_late"),
        _lc(260, L2, 12, 4, "lone0", offset=-50.0), _lc(260, L1, 0, 0, "lone0"), _lc(260, L4, 0, 60, "none", scale=8.0),
        _lc(1024, L3, 12, 4, "zero_plus"), _lc(1024, L5, 0, 60, "none", offset=50.0), _lc(1024, L4, 12, 0, "lone0_late", pad=1023),
        _lc(8192, L2, 0, 4, "lone0_late", scale=8.0), _lc(8192, L5, 12, 60, "tail", offset=-50.0), _lc(8192, L1, 0, 0, "lone0", pad=0),
        # smoothing = 0: eps = 0 (the eps > 0 guard), and a lone <pad> row whose whole target row is then zero
        _lc(3000, L2, 0, 0, "tail", smoothing=0.0), _lc(260, L4, 12, 4, "lone0", smoothing=0.0), _lc(104, L3, 0, 60, "none", smoothing=0.0),
        # smoothing = 1: conf = 0 (the conf > 0 guard)
        _lc(1024, L2, 0, 0, "tail", smoothing=1.0),
    ]
    return cases


def loss_case_id(c):
    return (f"V{c.V}-{'x'.join(map(str, c.segs))}-ldz{c.ldz_pad}-ldd{c.ldd_pad}-{c.pads}-sm{c.smoothing:g}-s{c.scale:g}"
            f"o{c.offset:g}-pad{c.pad}")


def loss_inputs(case, seed):
    """(logits float32 [rows, V], [target int64 per segment]) from a seeded CPU generator."""
    g = torch.Generator().manual_seed(seed)
    rows = sum(case.segs)
    z = torch.randn(rows, case.V, generator=g) * case.scale + case.offset
    targets = []
    for s, n in enumerate(case.segs):
        t = torch.randint(0, case.V - 1, (n,), generator=g)
        t = t + (t >= case.pad).long()                      # uniform over the non-<pad> columns
        if n > 1:
            t[1] = case.V - 1 if case.pad != case.V - 1 else 0        # the edge columns as targets
        if n > 3:
            t[3] = 0 if case.pad != 0 else case.V - 1
        kind = case.pads
        if kind == "lone0_late":
            kind = "tail" if s == 0 else ("lone0" if s == min(2, len(case.segs) - 1) else "none")
        if kind == "tail" and n > 1:
            t[n - 1] = case.pad
            if n > 4:
                t[2] = case.pad; t[n // 2] = case.pad
        elif kind == "lone0":
            t[0] = case.pad
        elif kind == "zero_plus":
            t[0] = case.pad
            if n > 1:
                t[n - 1 if n < 4 else 2] = case.pad
        targets.append(t)
    return z, targets


def zeroed_rows(target, pad):
    """Rows label_smoothing.py:29 zeroes: <pad> rows, if the sum of their indices is positive."""
    is_pad = target == pad
    idx_sum = int((torch.arange(target.numel()) * is_pad).sum())
    return is_pad & (idx_sum > 0)


def smoothed_targets(target, V, pad, smoothing, dtype=torch.float64):
    td = torch.full((target.numel(), V), smoothing / (V - 2), dtype=dtype)
    td.scatter_(1, target.unsqueeze(1), 1.0 - smoothing)
    td[:, pad] = 0
    td[zeroed_rows(target, pad)] = 0
    return td


def composed_loss(logits, targets, case, coef=COEF, norm=NORM, gloss=GLOSS):
    """float64: dict(lse [rows], rowloss [rows], total, dlogits [rows, V] = gloss * d total / d logits, zero [rows] bool,
    sum_td [rows]).  The total is built from oracle.mtn_oracle.label_smoothing_kl; the per-row values restate its target
    distribution and are checked here against it segment by segment."""
    z = logits.double().clone().requires_grad_()
    logp = torch.log_softmax(z, dim=1)
    total, rowloss, zero, sum_td, base = 0.0, [], [], [], 0
    for s, t in enumerate(targets):
        n = t.numel()
        seg = logp[base:base + n]
        kl = label_smoothing_kl(seg, t, case.pad, case.smoothing)
        total = total + coef[s] * kl / norm[s]
        td = smoothed_targets(t, case.V, case.pad, case.smoothing)
        safe = torch.where(td > 0, td, torch.ones_like(td))
        rows = (td * (safe.log() - seg.detach())).sum(1)
        assert abs(float(rows.sum()) - float(kl.detach())) <= 1e-12 * max(1.0, abs(float(kl.detach()))), (float(rows.sum()), float(kl.detach()))
        rowloss.append(rows * (coef[s] / norm[s]))
        zero.append(zeroed_rows(t, case.pad))
        sum_td.append(td.sum(1))
        base += n
    (grad,) = torch.autograd.grad(total, z)
    return dict(lse=torch.logsumexp(z.detach(), dim=1), rowloss=torch.cat(rowloss), total=float(total.detach()), dlogits=gloss * grad,
                zero=torch.cat(zero), sum_td=torch.cat(sum_td), softmax=logp.detach().exp())


def closed_form_f32(logits, targets, case, coef=COEF, norm=NORM, gloss=GLOSS):
    """The closed form of csrc/losshead.hip evaluated in float32 with torch on the CPU (torch's exp / log / summation order):
    (lse, rowloss, dlogits).  Not a reference: the yardstick for what float32 can deliver on this formula."""
    f = torch.float32
    z = logits.to(f)
    V = case.V
    t = torch.cat(targets)
    zero = torch.cat([zeroed_rows(x, case.pad) for x in targets])
    scale = torch.cat([torch.full((x.numel(),), coef[s], dtype=f) / torch.tensor(norm[s], dtype=f) for s, x in enumerate(targets)])
    eps = torch.tensor(case.smoothing, dtype=f) / torch.tensor(float(V - 2), dtype=f)
    conf = torch.tensor(1.0, dtype=f) - torch.tensor(case.smoothing, dtype=f)
    lse = torch.logsumexp(z, dim=1)
    S = z.sum(1)
    zt = z.gather(1, t.unsqueeze(1)).squeeze(1)
    zp = z[:, case.pad]
    t_is_pad = t == case.pad
    xlogx = lambda v: v * torch.log(v) if float(v) > 0 else torch.zeros((), dtype=f)
    n2, n1 = torch.tensor(float(V - 2), dtype=f), torch.tensor(float(V - 1), dtype=f)
    sum_tdz = torch.where(t_is_pad, eps * (S - zp), eps * (S - zt - zp) + conf * zt)
    sum_td = torch.where(t_is_pad, n1 * eps, n2 * eps + conf)
    sum_tdlog = torch.where(t_is_pad, n1 * xlogx(eps), n2 * xlogx(eps) + xlogx(conf))
    rowloss = torch.where(zero, torch.zeros((), dtype=f), (sum_tdlog - sum_tdz + lse * sum_td) * scale)
    td = torch.full_like(z, float(eps))
    td.scatter_(1, t.unsqueeze(1), float(conf))
    td[:, case.pad] = 0
    g = torch.tensor(gloss, dtype=f) * scale
    sum_td = torch.where(zero, torch.zeros((), dtype=f), sum_td)
    dz = g.unsqueeze(1) * (torch.exp(z - lse.unsqueeze(1)) * sum_td.unsqueeze(1) - td)
    dz[zero] = 0
    return lse, rowloss, dz


def loss_errors(got_lse, got_rowloss, got_dz, ref):
    """(lse absolute, rowloss relative to the case's largest |rowloss|, dlogits relative to max |ref|)"""
    e_lse = float((got_lse.double() - ref["lse"]).abs().max())
    e_row = float((got_rowloss.double() - ref["rowloss"]).abs().max() / max(1e-30, float(ref["rowloss"].abs().max())))
    e_dz = float((got_dz.double() - ref["dlogits"]).abs().max() / max(1e-30, float(ref["dlogits"].abs().max())))
    return e_lse, e_row, e_dz


# What float32 delivers on the closed form: the worst error of closed_form_f32 against composed_loss over loss_cases() (seeds
# LOSS_SEED + index), measured with torch on a CPU: lse absolute, rowloss relative to the case's largest |rowloss|, dlogits relative
# to max |ref|.  The logits with a common offset of +-50 reach 2.1e-6 on lse (half an ulp of lse ~ 58) and the N(0, 8^2) logits the
# same (lse ~ 36): neither needs a looser bound than the other, so one constant per quantity serves every case.
# tests/test_row_refs.py re-measures them (within a factor 2: summation order differs between CPUs).
LOSS_SEED = 1000
CPU_F32_LSE_ABS = 2.15e-6
CPU_F32_ROWLOSS_REL = 8.54e-7
CPU_F32_DLOGITS_REL = 2.03e-6
# torch.log_softmax in float32 on the CPU against float64 over the lsm_cases() WITHOUT a common offset (seeds LSM_SEED + index):
# half an ulp of the -80 the dominant-logit row produces
LSM_SEED = 2000
CPU_F32_LSM_ABS = 3.82e-6

# ------------------------------------------------------------------------------------------ log-softmax rows: cases
LsmCase = namedtuple("LsmCase", "rows V ldx_pad ldo_pad inplace offset")


def lsm_cases():
    """rows x V in full; row strides, in-place and the common offset rotated over them (every value meets every V)."""
    variants = [(0, 0, False, 0.0), (5, 0, False, 1e4), (0, 5, False, -1e4), (5, 5, True, 0.0), (0, 0, True, 1e4), (5, 5, False, 0.0),
                (5, 5, True, -1e4)]
    cases, k = [], 0
    for V in (1, 7, 255, 256, 257, 3000, 5003):
        for rows in (1, 5, 64):
            cases.append(LsmCase(rows, V, *variants[k % len(variants)]))
            k += 3                      # 3 and 7 are coprime: each V meets three different variants, each variant every rows
    return cases


def lsm_inputs(case, seed):
    """float32 [rows, V]: N(0, 2^2) + offset; row 0 holds one dominant logit (+80 over the rest)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(case.rows, case.V, generator=g) * 2.0
    x[0, case.V // 2] += 80.0
    return (x + case.offset).float()


# ------------------------------------------------------------------------------------------ Adam / Noam
BETA1, BETA2, ADAM_EPS = 0.9, 0.98, 1e-9


def noam_state64(step, model_size, warmup, factor, beta1=BETA1, beta2=BETA2):
    """[step, lr, 1 - beta1^step, 1 - beta2^step] in float64 (python floats; lr = oracle.mtn_oracle.noam_rate)."""
    return [float(step), noam_rate(step, model_size, warmup, factor), 1.0 - beta1 ** step, 1.0 - beta2 ** step]


def adam_step64(p, g, m, v, lr, bc1, bc2, grad_scale=1.0, beta1=BETA1, beta2=BETA2, eps=ADAM_EPS):
    """One step of torch.optim.Adam (no weight decay, no amsgrad) on float64 tensors -> (p, m, v); csrc/common.h:
    m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g^2;  p -= (lr / bc1) * m / (sqrt(v) / sqrt(bc2) + eps)."""
    g = g * grad_scale
    m = beta1 * m + (1.0 - beta1) * g
    v = beta2 * v + (1.0 - beta2) * g * g
    p = p - (lr / bc1) * m / (v.sqrt() / math.sqrt(bc2) + eps)
    return p, m, v


def adam_inputs(n, seed):
    """p, g, m, v (v >= 0) as float32 CPU tensors; the first elements hold exact zeros (g = m = v = 0 leaves p unchanged:
    0 / eps) and a zero second moment under a live gradient."""
    gen = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=gen)
    g = torch.randn(n, generator=gen) * 0.3
    m = torch.randn(n, generator=gen) * 0.01
    v = torch.rand(n, generator=gen) * 1e-3 + 1e-8
    g[0] = 0.0; m[0] = 0.0; v[0] = 0.0
    v[1] = 0.0
    if n > 2:
        g[2] = 0.0
    return p, g, m, v


def bf16_ulp(x):
    """Spacing of bfloat16 at |x| (float64 tensor): 2^(floor(log2 |x|) - 7), the subnormal spacing 2^-133 below 2^-126."""
    _, ex = torch.frexp(x.abs().double())                       # |x| = mant * 2^ex, mant in [0.5, 1)
    return torch.pow(2.0, (ex.clamp(min=-125) - 8).double())
