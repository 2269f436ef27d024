"""float64 reference, float32 closed form, case list and input generators for the unlikelihood loss head (csrc/losshead.hip;
include/mtn_hip.h mtn_ulosshead_args), validated without a GPU by tests/test_unlikelihood_refs.py and used on the device by
tests/test_unlikelihood_kernel_gpu.py.  Plain helpers, no fixtures.

composed_ul      the definition: the hard part is row_refs.composed_loss (float64 log_softmax -> oracle label_smoothing_kl -> coef / norm,
                 gradient by autograd); the unlikelihood part is, per row, a python set of the sequence's earlier targets without the
                 row's own target and <pad>, ul = sum_c -log(clamp(1 - p_c, min=MTN_UL_CLAMP)) with torch.clamp, gradient by autograd:
                     rowloss = scale (KL_ls + ul_alpha ul)
closed_form_f32  the kernel's closed form (r_c = p_c / (1 - p_c) on unclamped candidates, R their sum, d_j = [j live] r_j - p_j R) in
                 float32 with torch on the CPU: its error against composed_ul is what the kernel's bounds are derived from (4x, as
                 tests/test_row_kernels_gpu.py and tests/test_distill_kernel_gpu.py).
"""
from collections import namedtuple

import numpy as np
import torch

from tests import row_refs as rr

UL_CLAMP = float(np.float32(1e-5))          # MTN_UL_CLAMP is a float constant
UL_SEED = 4000
CLAMP_RAISE = 40.0                          # the logit of the candidate meant to be clamped is raised by this much

# layout: per segment (sequences, T); T = 0: a segment of `sequences` rows without unlikelihood (seq_len 0).
# pads:   none | inside (a <pad> in the middle of every sequence) | tail (every sequence ends in <pad>s, of different lengths) |
#         allpad (the last sequence is all <pad>, the others as tail) | quirk (a lone <pad> at the segment's row 0, no other)
# clamp:  one candidate of one row has its logit raised by CLAMP_RAISE
ULCase = namedtuple("ULCase", "V layout ldz_pad ldd_pad pads smoothing ul_alpha pad clamp")


def ul_cases():
    """V in {8, 260, 3000} (one partial sweep; one full sweep plus a 4-column tail; the workload's size), T in {1, 5, 70} (70 > 64: the
    lane loop over the prefix wraps), 1 and 3 sequences; <pad> placements, the clamped candidate, the segment layout, the strides,
    ul_alpha, smoothing and the <pad> index rotated over them.  The generator puts a repeated token, the row's own target, and the columns
    0 (or 1), V - 1 (or V - 2) and, for V = 260, 257 into the prefixes of every sequence with T >= 5."""
    c = ULCase
    return [
        c(8, ((1, 1),), 0, 0, "none", 0.1, 0.5, 1, False),
        c(8, ((3, 5),), 12, 12, "inside", 0.0, 2.0, 0, False),
        c(8, ((1, 70),), 0, 12, "tail", 0.1, 0.5, 7, True),
        c(8, ((3, 70),), 12, 0, "allpad", 0.0, 2.0, 1, False),
        c(260, ((1, 1),), 0, 0, "quirk", 0.1, 2.0, 1, False),
        c(260, ((3, 5),), 12, 12, "allpad", 0.1, 2.0, 259, True),
        c(260, ((1, 70),), 0, 0, "quirk", 0.0, 0.5, 0, False),
        c(260, ((2, 0), (3, 70)), 12, 12, "inside", 0.1, 2.0, 1, False),
        c(260, ((3, 5), (1, 70)), 0, 12, "tail", 0.0, 0.5, 1, True),
        c(3000, ((3, 1),), 12, 0, "tail", 0.1, 2.0, 0, False),
        c(3000, ((1, 5),), 12, 12, "none", 0.0, 2.0, 2999, False),
        c(3000, ((3, 70),), 0, 0, "tail", 0.1, 0.5, 1, True),
        c(3000, ((3, 0), (1, 70), (2, 0)), 0, 12, "quirk", 0.1, 0.5, 1, True),
        c(3000, ((3, 5),), 0, 0, "inside", 0.1, 2.0, 1, False),
    ]


def ul_case_id(c):
    lay = "+".join(f"{n}x{T}" for n, T in c.layout)
    return f"V{c.V}-{lay}-ld{c.ldz_pad}.{c.ldd_pad}-{c.pads}-sm{c.smoothing:g}-a{c.ul_alpha:g}-pad{c.pad}{'-clamp' if c.clamp else ''}"


def seg_rows(case):
    return tuple(n * max(T, 1) for n, T in case.layout)


def seq_lens(case):
    return tuple(T for _, T in case.layout)


def loss_case(case):
    """The row_refs.LossCase of the hard part (its generator fields are not used here)."""
    return rr.LossCase(case.V, seg_rows(case), case.ldz_pad, case.ldd_pad, case.pads, case.smoothing, 1.0, 0.0, case.pad)


def candidates(target, i, T, pad):
    """The sorted candidate list of local row i of a segment with sequence length T (0: none): the set of the sequence's earlier
    targets without the row's own target and <pad>; empty on <pad>-target rows."""
    if T <= 0:
        return []
    t = i % T
    y = int(target[i])
    if y == pad or t == 0:
        return []
    return sorted(set(int(v) for v in target[i - t:i]) - {y, pad})


def candidate_mask(case, targets, ul_alpha=None):
    """[rows, V] bool: column c is a candidate of the row"""
    alpha = case.ul_alpha if ul_alpha is None else ul_alpha
    m = torch.zeros(sum(seg_rows(case)), case.V, dtype=torch.bool)
    base = 0
    for s, t in enumerate(targets):
        for i in range(t.numel()):
            cand = candidates(t, i, seq_lens(case)[s] if alpha > 0 else 0, case.pad)
            if cand:
                m[base + i, cand] = True
        base += t.numel()
    return m


def _sequence(case, T, b, n_seq, g):
    V, pad = case.V, case.pad
    lo = 0 if pad != 0 else 1
    hi = V - 1 if pad != V - 1 else V - 2
    pool = torch.randperm(V, generator=g)[:max(3, min(V - 1, T // 2))]
    pool = pool[pool != pad]
    y = pool[torch.randint(0, pool.numel(), (T,), generator=g)]
    if T >= 5:
        y[0], y[1] = lo, hi
        y[2] = 257 if V == 260 else int(pool[0])
        y[3] = y[b % 3]                                     # the row's own target is in its prefix (excluded); a repeat for the rows after
        y[4] = int(pool[-1]) if int(pool[-1]) not in (lo, hi) else int(pool[0])
    kind = case.pads
    if kind == "allpad":
        kind = "all" if b == n_seq - 1 else "tail"
    if kind == "inside" and T > 1:
        y[T // 2] = pad
        if T >= 70:
            y[66] = pad
    elif kind == "tail":
        if T == 1:
            if b == n_seq - 1 and n_seq > 1:
                y[0] = pad
        else:
            y[T - 1 - (b % 3) * (T // 5):] = pad
    elif kind == "all":
        y[:] = pad
    return y


def ul_inputs(case, seed):
    """(logits float32 [rows, V], [target int64 per segment]) from a seeded CPU generator."""
    g = torch.Generator().manual_seed(seed)
    rows = seg_rows(case)
    z = torch.randn(sum(rows), case.V, generator=g)
    targets = []
    for (n, T), r in zip(case.layout, rows):
        if T == 0:
            t = torch.randint(0, case.V - 1, (r,), generator=g)
            t = t + (t >= case.pad).long()
        else:
            t = torch.cat([_sequence(case, T, b, n, g) for b in range(n)])
        if case.pads == "quirk":
            t = torch.where(t == case.pad, torch.tensor((case.pad + 2) % case.V), t)
            if T > 0:
                t[0] = case.pad
        targets.append(t)
    if case.clamp:
        row, col = clamped_candidate(case, targets)
        z[row, col] += CLAMP_RAISE
    return z, targets


def clamped_candidate(case, targets):
    """(flat row, column) of the candidate meant to be clamped: the last row of the first unlikelihood segment's first sequence that has
    candidates, and its smallest one."""
    base = 0
    for s, t in enumerate(targets):
        T = seq_lens(case)[s]
        if T > 0:
            for i in range(T - 1, 0, -1):
                cand = candidates(t, i, T, case.pad)
                if cand:
                    return base + i, cand[0]
        base += t.numel()
    raise AssertionError("the case has no row with candidates")


def seg_scale(case, dtype=torch.float64):
    return torch.cat([torch.full((n,), rr.COEF[s], dtype=dtype) / torch.tensor(rr.NORM[s], dtype=dtype) for s, n in enumerate(seg_rows(case))])


def ul_rows_of_logp(logp, y, pad):
    """(B, T) ul of ``logp`` (B, T, V) log-probabilities and ``y`` (B, T) targets by the definition (python sets, torch.clamp), in logp's
    dtype and differentiable: what SimpleLossCompute.loss(unlikelihood=...) and the training step are held to."""
    B, T, _ = logp.shape
    flat = y.reshape(-1)
    rows = []
    for i in range(B * T):
        cand = candidates(flat, i, T, pad)
        if cand:
            rows.append(-torch.log(torch.clamp(1.0 - logp[i // T, i % T, cand].exp(), min=UL_CLAMP)).sum())
        else:
            rows.append(logp.new_zeros(()))
    return torch.stack(rows).view(B, T)


def composed_ul(logits, targets, case, gloss=rr.GLOSS, ul_alpha=None):
    """float64: dict(lse, rowloss, rowul, total, dlogits = gloss * d total / d logits, zero, hard = row_refs.composed_loss's dict)."""
    alpha = float(case.ul_alpha if ul_alpha is None else ul_alpha)
    hard = rr.composed_loss(logits, targets, loss_case(case), gloss=gloss)
    z = logits.double().clone().requires_grad_()
    p = torch.log_softmax(z, dim=1).exp()
    rowul, base = [], 0
    for s, t in enumerate(targets):
        for i in range(t.numel()):
            cand = candidates(t, i, seq_lens(case)[s] if alpha > 0 else 0, case.pad)
            if cand:
                rowul.append(-torch.log(torch.clamp(1.0 - p[base + i, cand], min=UL_CLAMP)).sum())
            else:
                rowul.append(torch.zeros((), dtype=torch.float64))
        base += t.numel()
    rowul = torch.stack(rowul)
    soft = seg_scale(case) * alpha * rowul
    if soft.requires_grad:
        (gsoft,) = torch.autograd.grad(soft.sum(), z)
    else:
        gsoft = torch.zeros_like(z)
    rowloss = hard["rowloss"] + soft.detach()
    return dict(lse=hard["lse"], rowloss=rowloss, rowul=rowul.detach(), total=float(rowloss.sum()), dlogits=hard["dlogits"] + gloss * gsoft,
                zero=hard["zero"], hard=hard, softmax=p.detach())


def closed_form(logits, targets, case, gloss=rr.GLOSS, dtype=torch.float32):
    """The closed form of csrc/losshead.hip with torch on the CPU in ``dtype``: (lse, rowloss, rowul, dlogits).  In float32 not a
    reference: the yardstick for what float32 can deliver on this formula.  In float64 the hard part is the composed reference's."""
    f = dtype
    if f == torch.float32:
        lse, row_h, dz_h = rr.closed_form_f32(logits, targets, loss_case(case), gloss=gloss)
    else:
        hard = rr.composed_loss(logits, targets, loss_case(case), gloss=gloss)
        lse, row_h, dz_h = hard["lse"], hard["rowloss"], hard["dlogits"]
    z = logits.to(f)
    M = candidate_mask(case, targets)
    clamp = torch.tensor(UL_CLAMP, dtype=f)
    zero, one = torch.zeros((), dtype=f), torch.ones((), dtype=f)
    p = torch.exp(z - lse.unsqueeze(1))
    u = one - p
    rowul = torch.where(M, -torch.log(torch.maximum(u, clamp)), zero).sum(1)
    live = M & (u >= clamp)
    r = torch.where(live, p / torch.where(live, u, one), zero)
    R = r.sum(1)
    alpha, scale = torch.tensor(case.ul_alpha, dtype=f), seg_scale(case, f)
    rowloss = row_h + scale * (alpha * rowul)
    dz = dz_h + (torch.tensor(gloss, dtype=f) * scale).unsqueeze(1) * (alpha * (r - p * R.unsqueeze(1)))
    return lse, rowloss, rowul, dz


def closed_form_f32(logits, targets, case, gloss=rr.GLOSS):
    return closed_form(logits, targets, case, gloss=gloss, dtype=torch.float32)


def ul_errors(got_lse, got_rowloss, got_rowul, got_dz, ref):
    """(lse absolute | rowloss relative to the case's largest |rowloss| | rowul relative to max(1, the case's largest ul) | dlogits relative
    to max |ref|).  ul is a sum of up to T logarithms, each O(0.001..12): its error is absolute in nature and scales with the sum."""
    e_lse = float((got_lse.double() - ref["lse"]).abs().max())
    e_row = float((got_rowloss.double() - ref["rowloss"]).abs().max() / max(1e-30, float(ref["rowloss"].abs().max())))
    e_ul = float((got_rowul.double() - ref["rowul"]).abs().max() / max(1.0, float(ref["rowul"].abs().max())))
    e_dz = float((got_dz.double() - ref["dlogits"]).abs().max() / max(1e-30, float(ref["dlogits"].abs().max())))
    return e_lse, e_row, e_ul, e_dz


# What float32 delivers on the closed form: the worst error of closed_form_f32 against composed_ul over ul_cases() (seeds UL_SEED + index),
# measured with torch on a CPU in the units of ul_errors.  tests/test_unlikelihood_refs.py re-measures them and asserts that these are no
# smaller (measured 7.79e-7 | 2.36e-7 | 3.12e-7 | 3.27e-7; rounded up).  The kernel's bounds are 4x these (tests/test_unlikelihood_kernel_gpu.py).
CPU_F32_UL_LSE = 8.0e-7
CPU_F32_UL_ROWLOSS = 2.5e-7
CPU_F32_UL_ROWUL = 3.3e-7
CPU_F32_UL_DLOGITS = 3.5e-7
