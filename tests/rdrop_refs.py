"""float64 definition, float32 closed form, case list and bounds for the paired (R-Drop) loss head (csrc/losshead.hip; include/mtn_hip.h
mtn_rlosshead_args), validated without a GPU by tests/test_rdrop_refs.py and used on the device by tests/test_rdrop_kernel_gpu.py.  Plain
helpers, no fixtures.

composed_rd      the definition: the hard part is row_refs.composed_loss (float64 log_softmax -> oracle label_smoothing_kl -> coef / norm,
                 gradient by autograd).  The paired part is composed from torch.log_softmax: for a row i of a paired segment whose own
                 target is not <pad>, with partner j = i +- N,
                     J = sum_c (p_c - q_c)(log p_c - log q_c),  kl = sum_c p_c (log p_c - log q_c),  rd = J / 4,
                     rowloss = scale (KL_ls + rd_alpha rd).
                 Its gradient is autograd's of sum_i scale rd_alpha / 2 J(z_i, const z_j) over those rows: the header's backward, where
                 a row's logits enter its own rd and its partner's (2 * 1/4).  Where both rows of every pair are live (every case but the
                 lone <pad>) that is the gradient of sum_i scale rd_alpha rd_i itself; tests/test_rdrop_refs.py checks it.  Where a
                 row's partner has a <pad> target (the lone <pad> at row 0), the partner takes the plain path and receives no gradient
                 from the pair, as the header states.
closed_form_f32  the kernel restated operation for operation in float32 with numpy (the hard part with torch: row_refs.closed_form_f32):
                 forward  m = max_c z_c, lg = log sum_c exp(z_c - m), lse = m + lg, lp_c = (z_ic - m_i) - lg_i, lq_c = (z_jc - m_j) - lg_j,
                          p = exp(lp), q = exp(lq), d = lp - lq, J = sum_c (p_c - q_c) d_c, kl = sum_c p_c d_c, rd = 0.25 J
                 backward lp_k = z_ik - lse_i, lq_k = z_jk - lse_j, p = exp(lp), q = exp(lq),
                          dz_k = (g scale) [(p_k sum_td - td_k) + (0.5 rd_alpha) (p_k ((lp_k - lq_k) - kl) + (p_k - q_k))]
                 numpy sums in its own (pairwise) order where the kernel sums lane by lane; both orders are fixed, and (p - q) d and
                 (q - p)(-d) are the same products in either, so rd[i] == rd[i + N] bit for bit here as on the device.

Error units (rd_errors): lse absolute | rowloss relative to the case's largest |rowloss| | rowrd and rowkl relative to max(1, the case's
largest reference value of each) — both are sums of V log-ratio terms whose error is absolute in nature | dlogits: per row relative to
g scale_row max(1, B) with B the case's largest |bracket| = |ref dlogits| / (g scale_row): the error of the bracket [...] of the header's
backward, which is O(1) for the plain head and grows with rd_alpha |d| on rows that diverge.  With B <= 1 the gradient bound is
DLOGITS * g * scale.
"""
from collections import namedtuple

import numpy as np
import torch

from tests import row_refs as rr

# layout: per segment its pair distance N (the segment holds 2 N rows) or -n for an unpaired segment of n rows
# pads:   none | same (<pad> targets at the same local positions in both halves of every paired segment, and in the unpaired segments'
#         tails) | lone0 (a lone <pad> at row 0 of the paired segment, no other <pad> in it: the quirk row; its partner, row N, is live)
# form:   how the second half of a paired segment relates to the first
#   self   z_j = z_i                       off+ / off-   z_j = z_i +- 30 (the same distributions: the maxima must be taken out)
#   near   z_j = z_i + N(0, 0.1^2)         (the regime training lives in)
#   indep  independent rows                x8    independent rows, both scaled by 8 (peaked)
RDCase = namedtuple("RDCase", "V layout ldz_pad ldd_pad pads smoothing rd_alpha form pad")
FORMS = ("self", "off+", "off-", "near", "indep", "x8")
VS = (8, 104, 256, 260, 1024, 3000, 3004)
LAYOUTS = ((1,), (5,), (18,), (5, -3), (18, -15), (1, -1, -2), (-3, 5), (-2, 18))
PADDINGS = ((0, 0), (12, 60), (60, 12), (12, 12), (0, 60))          # (ldz, ldd)
PAD_KINDS = ("none", "same", "lone0")
ALPHAS = (0.3, 1.0, 5.0)
SMOOTHINGS = (0.1, 0.0, 0.1)
NEAR_NOISE = 0.1
OFFSET = 30.0
RD_SEED = 5000


def rd_cases():
    """Every V meets every <pad> placement; layouts (pair distances 1, 5, 18; the paired segment alone, before one and two unpaired
    segments, and at index 1 behind an unpaired one), strides, rd_alpha, smoothing, the <pad> index and the partner forms are rotated over
    them with strides coprime to their counts.  Then what the rotation leaves out: every form at the workload's V with partners in
    different workgroups (N = 18)."""
    cases, k = [], 0
    for V in VS:
        for kind in PAD_KINDS:
            zp, dp = PADDINGS[(3 * k) % 5]
            pad = (1, 0, V - 1)[(k // 2) % 3]
            lay = LAYOUTS[(3 * k) % 8]
            if kind == "same" and max(lay) == 1:             # (N = 1 with its only position <pad> would leave no live pair)
                lay = LAYOUTS[(3 * k + 1) % 8]
            cases.append(RDCase(V, lay, zp, dp, kind, SMOOTHINGS[k % 3], ALPHAS[(k + k // 3) % 3], FORMS[(5 * k + k // 6) % 6], pad))
            k += 1
    for j, form in enumerate(FORMS):
        cases.append(RDCase(3000, ((18,), (18, -15), (-2, 18))[j % 3], (0, 12)[j % 2], (0, 60)[j % 2], PAD_KINDS[j % 2], 0.1, ALPHAS[j % 3], form, 1))
    return cases


def rd_case_id(c):
    lay = "+".join(("p%d" % n) if n > 0 else ("u%d" % -n) for n in c.layout)
    return f"V{c.V}-{lay}-ld{c.ldz_pad}.{c.ldd_pad}-{c.pads}-sm{c.smoothing:g}-a{c.rd_alpha:g}-{c.form}-pad{c.pad}"


def seg_rows(case):
    return tuple(2 * n if n > 0 else -n for n in case.layout)


def pairs(case):
    return tuple(max(n, 0) for n in case.layout)


def loss_case(case):
    """The row_refs.LossCase of the hard part (its generator fields are not used here)."""
    return rr.LossCase(case.V, seg_rows(case), case.ldz_pad, case.ldd_pad, case.pads, case.smoothing, 1.0, 0.0, case.pad)


def seg_scale(case, dtype=torch.float64):
    return torch.cat([torch.full((n,), rr.COEF[s], dtype=dtype) / torch.tensor(rr.NORM[s], dtype=dtype) for s, n in enumerate(seg_rows(case))])


def rd_inputs(case, seed):
    """(logits float32 [rows, V], [target int64 per segment]) from a seeded CPU generator."""
    g = torch.Generator().manual_seed(seed)
    V, pad = case.V, case.pad
    zs, targets = [], []
    for n in case.layout:
        half = abs(n)
        t = torch.randint(0, V - 1, (half,), generator=g)
        t = t + (t >= pad).long()                            # uniform over the non-<pad> columns
        if half > 1:
            t[1] = V - 1 if pad != V - 1 else 0              # the edge columns as targets
        if half > 3:
            t[3] = 0 if pad != 0 else V - 1
        if case.pads == "same":
            t[half - 1] = pad
            if half > 4:
                t[2] = pad
        z = torch.randn(half, V, generator=g)
        if n < 0:
            zs.append(z); targets.append(t)
            continue
        if case.form == "self":
            zj = z.clone()
        elif case.form == "off+":
            zj = z + OFFSET
        elif case.form == "off-":
            zj = z - OFFSET
        elif case.form == "near":
            zj = z + NEAR_NOISE * torch.randn(half, V, generator=g)
        else:
            zj = torch.randn(half, V, generator=g)
            if case.form == "x8":
                z, zj = z * 8.0, zj * 8.0
        t2 = t.clone()
        if case.pads == "lone0":
            t[0] = pad
        zs += [z, zj]
        targets.append(torch.cat([t, t2]))
    return torch.cat(zs).float(), targets


def partner_index(case):
    """[rows] int64: the flat row of each row's partner; the row itself in unpaired segments"""
    idx, base = [], 0
    for n, r in zip(pairs(case), seg_rows(case)):
        loc = torch.arange(r)
        idx.append(base + (torch.where(loc < n, loc + n, loc - n) if n > 0 else loc))
        base += r
    return torch.cat(idx)


def rd_rows_mask(case, targets, rd_alpha=None):
    """rows that carry the paired term: the segment is paired, rd_alpha > 0, the row's own target is not <pad>"""
    alpha = case.rd_alpha if rd_alpha is None else rd_alpha
    return torch.cat([(t != case.pad) & (n > 0 and alpha > 0) for t, n in zip(targets, pairs(case))])


def rd_rows_of_logp(logp, y, pad):
    """(2 N,) rd of ``logp`` (2 N, V) log-probabilities whose rows i and i + N are the two passes of one position and ``y`` (2 N,)
    targets, by the definition, in logp's dtype and differentiable (nothing held constant): what SimpleLossCompute.loss(rdrop=...) and
    the training step are held to."""
    N = logp.size(0) // 2
    lq = torch.cat([logp[N:], logp[:N]])
    J = ((logp.exp() - lq.exp()) * (logp - lq)).sum(1)
    return torch.where(y.reshape(-1) != pad, J / 4, torch.zeros_like(J))


def composed_rd(logits, targets, case, gloss=rr.GLOSS, rd_alpha=None):
    """float64: dict(lse, rowloss, rowrd, rowkl, total, dlogits = gloss * gradient (see the module's header), full = gloss * d total / d
    logits by autograd with nothing held constant, zero, hard = row_refs.composed_loss's dict, mask, bracket)."""
    alpha = float(case.rd_alpha if rd_alpha is None else rd_alpha)
    hard = rr.composed_loss(logits, targets, loss_case(case), gloss=gloss)
    mask, j = rd_rows_mask(case, targets, alpha), partner_index(case)
    scale = seg_scale(case)
    z = logits.double().clone().requires_grad_()
    lp = torch.log_softmax(z, dim=1)

    def terms(lq):
        d = lp - lq
        J = ((lp.exp() - lq.exp()) * d).sum(1)
        kl = (lp.exp() * d).sum(1)
        zero = torch.zeros_like(J)
        return torch.where(mask, J, zero), torch.where(mask, kl, zero)

    J, kl = terms(lp[j])
    rd = J / 4
    soft = scale * alpha * rd
    Jc, _ = terms(lp[j].detach())
    if mask.any():
        (gsoft,) = torch.autograd.grad((scale * alpha / 2 * Jc).sum(), z, retain_graph=True)
        (gfull,) = torch.autograd.grad(soft.sum(), z)
    else:
        gsoft = gfull = torch.zeros_like(z)
    rowloss = hard["rowloss"] + soft.detach()
    dlogits = hard["dlogits"] + gloss * gsoft
    bracket = float((dlogits / (gloss * scale).unsqueeze(1)).abs().max())
    return dict(lse=hard["lse"], rowloss=rowloss, rowrd=rd.detach(), rowkl=kl.detach(), total=float(rowloss.sum()), dlogits=dlogits,
                full=hard["dlogits"] + gloss * gfull, zero=hard["zero"], hard=hard, mask=mask, bracket=bracket,
                terms=((lp.exp() - lp[j].exp()) * (lp - lp[j])).detach())


def closed_form_f32(logits, targets, case, gloss=rr.GLOSS, rd_alpha=None):
    """The kernel restated in float32 (numpy; the hard part with torch): (lse, rowloss, rowrd, rowkl, dlogits) as torch tensors.  Not a
    reference: the yardstick for what float32 can deliver on these formulas."""
    f = np.float32
    alpha = f(case.rd_alpha if rd_alpha is None else rd_alpha)
    lse_h, row_h, dz_h = rr.closed_form_f32(logits, targets, loss_case(case), gloss=gloss)
    mask = rd_rows_mask(case, targets, float(alpha)).numpy()
    n = logits.size(0)
    if not mask.any():
        return lse_h, row_h, torch.zeros(n), torch.zeros(n), dz_h
    j = partner_index(case).numpy()
    z = logits.numpy().astype(f)
    m = z.max(1, keepdims=True)
    lg = np.log(np.exp(z - m).sum(1, keepdims=True, dtype=f))
    lse = (m + lg)[:, 0]
    lp = (z - m) - lg
    lq = lp[j]                                               # the partner's wave computes (m_j, lg_j) as its own: the same bits
    p, q, d = np.exp(lp), np.exp(lq), lp - lq
    J = ((p - q) * d).sum(1, dtype=f)
    kl = (p * d).sum(1, dtype=f)
    rd = np.where(mask, f(0.25) * J, f(0))
    kl = np.where(mask, kl, f(0))
    scale = seg_scale(case, torch.float32).numpy()
    # rowloss = scale (KL_ls + rd_alpha rd): the hard part's scale KL_ls is row_refs', the paired part is added to it
    rowloss = row_h.numpy() + scale * (alpha * rd)
    lpb, lqb = z - lse[:, None], z[j] - lse[j][:, None]
    pb, qb = np.exp(lpb), np.exp(lqb)
    extra = (f(0.5) * alpha) * (pb * ((lpb - lqb) - kl[:, None]) + (pb - qb))
    dz = dz_h.numpy() + (f(gloss) * scale)[:, None] * np.where(mask[:, None], extra, f(0))
    assert rowloss.dtype == f and dz.dtype == f and rd.dtype == f and kl.dtype == f
    lse_out = np.where(mask, lse, lse_h.numpy())
    return torch.from_numpy(lse_out), torch.from_numpy(rowloss), torch.from_numpy(rd), torch.from_numpy(kl), torch.from_numpy(dz)


def dz_error(got_dz, ref, case, gloss=rr.GLOSS):
    """worst |got - ref| of a dlogits block in units of g scale_row max(1, the case's largest |bracket|)"""
    unit = (gloss * seg_scale(case)).unsqueeze(1) * max(1.0, ref["bracket"])
    return float(((got_dz.double() - ref["dlogits"]).abs() / unit).max())


def rd_errors(got_lse, got_rowloss, got_rowrd, got_rowkl, got_dz, ref, case):
    """(lse | rowloss | rowrd | rowkl | dlogits) in the units the module's header states"""
    e_lse = float((got_lse.double() - ref["lse"]).abs().max())
    e_row = float((got_rowloss.double() - ref["rowloss"]).abs().max() / max(1e-30, float(ref["rowloss"].abs().max())))
    e_rd = float((got_rowrd.double() - ref["rowrd"]).abs().max() / max(1.0, float(ref["rowrd"].abs().max())))
    e_kl = float((got_rowkl.double() - ref["rowkl"]).abs().max() / max(1.0, float(ref["rowkl"].abs().max())))
    return e_lse, e_row, e_rd, e_kl, dz_error(got_dz, ref, case)


# What float32 delivers on the closed form: the worst error of closed_form_f32 against composed_rd over rd_cases() (seeds RD_SEED + index),
# measured with numpy / torch on a CPU in the units of rd_errors.  tests/test_rdrop_refs.py re-measures them and asserts that these are no
# smaller and within a factor 2 (measured 2.03e-6 | 7.03e-7 | 1.51e-7 | 7.44e-7 | 1.66e-6; rounded up).  The kernel's bounds are 4x these
# (tests/test_rdrop_kernel_gpu.py): fast-math intrinsics and another summation order, the margin tests/test_row_kernels_gpu.py and
# tests/test_distill_kernel_gpu.py give.  None comes from running the kernel.
CPU_F32_RD_LSE = 2.1e-6
CPU_F32_RD_ROWLOSS = 7.1e-7
CPU_F32_RD_ROWRD = 1.6e-7
CPU_F32_RD_ROWKL = 7.5e-7
CPU_F32_RD_DLOGITS = 1.7e-6
# rd of a pair with identical distributions (self, off+-): at most the rowrd bound at its max(1, .) floor
RD_FLOOR = 4 * CPU_F32_RD_ROWRD
