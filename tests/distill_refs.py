"""float64 reference and case list for the distillation loss head (csrc/losshead.hip; include/mtn_hip.h mtn_distill_args), validated
without a GPU by tests/test_distill_refs.py and used on the device by tests/test_distill_kernel_gpu.py.  Plain helpers, no fixtures.

composed         the hard part is row_refs.composed_loss (float64 log_softmax -> oracle label_smoothing_kl -> coef / norm, gradient by
                 autograd); the soft part is F.kl_div(log_softmax(z / T), softmax(q / T)) per row, zeroed on rows whose target is
                 <pad>, its gradient by autograd; the two are combined as the header states:
                     rowloss = scale [(1 - alpha) KL_ls + alpha T^2 kd]     on segments with a teacher, when alpha > 0
                     rowloss = scale KL_ls                                   elsewhere (row_refs.composed_loss itself, nothing applied)
closed_form_f32  the kernel's closed form (the two row maxima taken out of every term) in float32 with torch on the CPU: its error
                 against the composed reference is what the kernel's bounds are derived from (4x, as tests/test_row_kernels_gpu.py).
"""
from collections import namedtuple

import torch
import torch.nn.functional as F

from tests import row_refs as rr

# teach: indices of the segments that have a teacher.  form: what the teacher rows hold
#   logp   log-probabilities (log_softmax of N(0, 1) logits)
#   off+ / off-   raw logits with a common offset of +-50
#   x8     logits scaled by 8 (a peaked teacher)
#   inf    N(0, 1) logits with -inf in a fifth of the columns (never a whole row)
DistCase = namedtuple("DistCase", "V segs teach ldz_pad ldq_pad ldd_pad pads smoothing T alpha form pad scale offset")
FORMS = ("logp", "off+", "off-", "x8", "inf")
LAYOUTS = (((1,), (0,)), ((5,), (0,)), ((18, 15), (0,)), ((3, 1, 1, 2), (0, 2)))
VS = (8, 104, 256, 260, 1024, 3000, 3004)
PADDINGS = ((0, 0, 0), (12, 60, 0), (60, 12, 12), (0, 12, 60), (12, 0, 60), (60, 60, 12), (0, 60, 0))      # (ldz, ldq, ldd)
TEMPS = (0.5, 1.0, 2.0)
ALPHAS = (0.3, 1.0, 0.3, 0.0)
SMOOTHINGS = (0.1, 0.0, 0.1)
DIST_SEED = 3000


def loss_case(c):
    """The row_refs.LossCase of the hard part."""
    return rr.LossCase(c.V, c.segs, c.ldz_pad, c.ldd_pad, c.pads, c.smoothing, c.scale, c.offset, c.pad)


def dist_cases():
    """A covering list: every V meets every <pad> placement; layouts, strides, T, alpha, smoothing, teacher forms and student logit
    statistics are rotated over them with strides coprime to their counts, so that every value of the issue's lists appears with small,
    single-sweep and multi-sweep V.  Then the cases the rotation cannot hold: -inf teacher columns at the sweep boundaries."""
    cases, k = [], 0
    stats = ((1.0, 0.0), (1.0, 0.0), (8.0, 0.0), (1.0, 50.0), (1.0, -50.0))
    for V in VS:
        for kind in rr.PAD_KINDS:
            segs, teach = LAYOUTS[k % 4]
            if kind == "lone0_late" and len(segs) < 2:
                segs, teach = LAYOUTS[2 + k % 2]
            zp, qp, dp = PADDINGS[(3 * k) % 7]
            pad = (1, 0, V - 1)[(k // 2) % 3]
            sc, of = stats[(2 * k + k // 5) % 5]
            cases.append(DistCase(V, segs, teach, zp, qp, dp, kind, SMOOTHINGS[k % 3], TEMPS[(k + k // 3) % 3], ALPHAS[(k + k // 4) % 4],
                                  FORMS[(k + k // 5) % 4], pad, sc, of))
            k += 1
    cases += [DistCase(260, (5,), (0,), 0, 12, 0, "tail", 0.1, 2.0, 0.3, "inf", 1, 1.0, 0.0),
              DistCase(3000, (18, 15), (0,), 12, 0, 60, "none", 0.1, 0.5, 1.0, "inf", 1, 1.0, 0.0),
              DistCase(8, (3, 1, 1, 2), (0, 2), 0, 60, 12, "lone0_late", 0.0, 1.0, 0.3, "inf", 0, 1.0, 0.0)]
    return cases


def dist_case_id(c):
    return (f"V{c.V}-{'x'.join(map(str, c.segs))}-t{''.join(map(str, c.teach))}-ld{c.ldz_pad}.{c.ldq_pad}.{c.ldd_pad}-{c.pads}-sm{c.smoothing:g}"
            f"-T{c.T:g}-a{c.alpha:g}-{c.form}-pad{c.pad}-s{c.scale:g}o{c.offset:g}")


def dist_inputs(case, seed):
    """(logits float32 [rows, V], [target int64 per segment], [teacher float32 [rows_s, V] or None per segment])"""
    z, targets = rr.loss_inputs(loss_case(case), seed)
    g = torch.Generator().manual_seed(seed + 7919)
    teachers = []
    for s, n in enumerate(case.segs):
        if s not in case.teach:
            teachers.append(None)
            continue
        q = torch.randn(n, case.V, generator=g)
        if case.form == "logp":
            q = torch.log_softmax(q.double(), dim=1).float()
        elif case.form == "off+":
            q = q + 50.0
        elif case.form == "off-":
            q = q - 50.0
        elif case.form == "x8":
            q = q * 8.0
        elif case.form == "inf":
            q[:, 2::5] = float("-inf")
        teachers.append(q.float())
    return z, targets, teachers


def seg_scale(case, dtype=torch.float64):
    return torch.cat([torch.full((n,), rr.COEF[s], dtype=dtype) / torch.tensor(rr.NORM[s], dtype=dtype) for s, n in enumerate(case.segs)])


def kd_rows_mask(case, targets):
    """rows that carry a soft term: the segment has a teacher, alpha > 0, the target is not <pad>"""
    m = [(t != case.pad) & (s in case.teach and case.alpha > 0) for s, t in enumerate(targets)]
    return torch.cat(m)


def seg_distilled(case):
    """per row: the segment's hard part carries (1 - alpha)"""
    return torch.cat([torch.full((n,), s in case.teach and case.alpha > 0, dtype=torch.bool) for s, n in enumerate(case.segs)])


def _teacher_matrix(case, teachers, dtype):
    """[rows, V]: the teacher rows, zeros where a segment has none (those rows are masked out)"""
    return torch.cat([q.to(dtype) if q is not None else torch.zeros(n, case.V, dtype=dtype) for q, n in zip(teachers, case.segs)])


def composed_distill(logits, targets, teachers, case, gloss=rr.GLOSS):
    """float64: dict(lse, rowloss, rowkd, total, dlogits = gloss * d total / d logits, zero, hard = row_refs.composed_loss's dict)."""
    hard = rr.composed_loss(logits, targets, loss_case(case), gloss=gloss)
    dist, mask = seg_distilled(case), kd_rows_mask(case, targets)
    n = logits.size(0)
    if not bool(dist.any()):
        return dict(lse=hard["lse"], rowloss=hard["rowloss"], rowkd=torch.zeros(n, dtype=torch.float64), total=hard["total"],
                    dlogits=hard["dlogits"], zero=hard["zero"], hard=hard)
    T, alpha = float(case.T), float(case.alpha)
    z = logits.double().clone().requires_grad_()
    q = _teacher_matrix(case, teachers, torch.float64)
    kd = F.kl_div(torch.log_softmax(z / T, dim=1), torch.softmax(q / T, dim=1), reduction="none").sum(1)
    kd = torch.where(mask, kd, torch.zeros_like(kd))
    scale = seg_scale(case)
    soft = scale * alpha * T * T * kd
    (gsoft,) = torch.autograd.grad(soft.sum(), z)
    w = torch.where(dist, torch.full((n,), 1.0 - alpha, dtype=torch.float64), torch.ones(n, dtype=torch.float64))
    rowloss = w * hard["rowloss"] + soft.detach()
    return dict(lse=hard["lse"], rowloss=rowloss, rowkd=kd.detach(), total=float(rowloss.sum()),
                dlogits=w.unsqueeze(1) * hard["dlogits"] + gloss * gsoft, zero=hard["zero"], hard=hard)


def closed_form_f32(logits, targets, teachers, case, gloss=rr.GLOSS):
    """The closed form of csrc/losshead.hip in float32 with torch on the CPU: (lse, rowloss, rowkd, dlogits).  Not a reference."""
    f = torch.float32
    lse, row_h, dz_h = rr.closed_form_f32(logits, targets, loss_case(case), gloss=gloss)
    dist, mask = seg_distilled(case), kd_rows_mask(case, targets)
    n = logits.size(0)
    if not bool(dist.any()):
        return lse, row_h, torch.zeros(n, dtype=f), dz_h
    T, alpha = torch.tensor(case.T, dtype=f), torch.tensor(case.alpha, dtype=f)
    z = logits.to(f)
    q = _teacher_matrix(case, teachers, f)
    a, b = z / T, q / T
    da = a - a.max(1, keepdim=True).values
    db = b - b.max(1, keepdim=True).values
    e = torch.exp(db)
    term = torch.where(torch.isinf(db), torch.zeros((), dtype=f), e * (db - da))
    kd = term.sum(1) / e.sum(1) - torch.log(e.sum(1)) + torch.log(torch.exp(da).sum(1))
    kd = torch.where(mask, kd, torch.zeros((), dtype=f))
    scale = seg_scale(case, f)
    w = torch.where(dist, 1.0 - alpha, torch.ones((), dtype=f))
    rowloss = w * row_h + scale * (alpha * T * T) * kd
    pS = torch.exp(a - torch.logsumexp(a, dim=1, keepdim=True))
    pT = torch.exp(b - torch.logsumexp(b, dim=1, keepdim=True))
    soft = torch.where(mask.unsqueeze(1), (alpha * T) * (pS - pT), torch.zeros((), dtype=f))
    dz = w.unsqueeze(1) * dz_h + (torch.tensor(gloss, dtype=f) * scale).unsqueeze(1) * soft
    return lse, rowloss, kd, dz


def dist_errors(got_lse, got_rowloss, got_rowkd, got_dz, ref):
    """(lse absolute | rowloss relative to the case's largest |rowloss| | rowkd relative to max(1, the case's largest kd) | dlogits
    relative to max |ref|).  kd is a difference of log-sum-exps and a mean of log-ratios, each O(1..100): its error is absolute in
    nature, and scales with the magnitude of those terms, which the largest kd of the case tracks."""
    e_lse = float((got_lse.double() - ref["lse"]).abs().max())
    e_row = float((got_rowloss.double() - ref["rowloss"]).abs().max() / max(1e-30, float(ref["rowloss"].abs().max())))
    e_kd = float((got_rowkd.double() - ref["rowkd"]).abs().max() / max(1.0, float(ref["rowkd"].abs().max())))
    e_dz = float((got_dz.double() - ref["dlogits"]).abs().max() / max(1e-30, float(ref["dlogits"].abs().max())))
    return e_lse, e_row, e_kd, e_dz


# What float32 delivers on the closed form: the worst error of closed_form_f32 against composed_distill over dist_cases() (seeds
# DIST_SEED + index), measured with torch on a CPU in the units of dist_errors.  tests/test_distill_refs.py re-measures them (within a
# factor 2: summation order differs between CPUs).  The kernel's bounds are 4x these (tests/test_distill_kernel_gpu.py).
CPU_F32_DISTILL_LSE = 2.16e-6
CPU_F32_DISTILL_ROWLOSS = 1.28e-6
CPU_F32_DISTILL_ROWKD = 4.71e-7
CPU_F32_DISTILL_DLOGITS = 1.34e-6
