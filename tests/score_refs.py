"""mtn_score_rows' definitions (include/mtn_hip.h) restated in float64, the same closed form in float32 with torch on the CPU, and the
case list of tests/test_score_kernel_gpu.py; validated without a GPU by tests/test_score_refs.py.  Plain helpers, no fixtures.

    tok_logp  z[t] - logsumexp(z[0..V-1])                          0 where t is <pad> or outside [0, V)
    tok_rank  #{c : z[c] > z[t]} + #{c < t : z[c] == z[t]}         -1 there
    seq_logp  sum of the sequence's tok_logp, ascending position   seq_len: its counted positions
"""
from collections import namedtuple

import torch

PAD = 1
ScoreCase = namedtuple("ScoreCase", "n_seq L V ldz offset")
SHAPES = [(1, 1, 7, 8), (3, 5, 64, 64), (2, 20, 257, 264), (2, 9, 3004, 3008), (1, 3, 4099, 4100), (1, 2, 40000, 40000)]
OFFSETS = (0.0, 50.0, -50.0)
SCORE_SEED = 3000


def score_cases():
    """Every shape under N(0, 8^2) logits without and with a common offset of +-50 (as row_refs.loss_cases has)."""
    return [ScoreCase(*s, o) for s in SHAPES for o in OFFSETS]


def score_case_id(c):
    return f"n{c.n_seq}-L{c.L}-V{c.V}-ldz{c.ldz}-o{c.offset:g}"


def score_inputs(case, seed):
    """(logits float32 [n_seq * L, ldz], target int64 [n_seq, L], planted) from a seeded CPU generator.  Columns V..ldz-1 hold NaN (never
    read).  Sequence 0 carries, as far as L allows: column 0, column V - 1, an interior <pad>, an id past the vocabulary, a negative id,
    an id past 2^31, a trailing <pad>; the last of several sequences is all <pad>.  Exact ties are planted in the float32 logits: the
    target equal to a column on either side of it, a duplicated row maximum, and a lower column equal to the target V - 1.
    planted: names of what this case could hold."""
    n, L, V, ldz, off = case
    g = torch.Generator().manual_seed(seed)
    z = (torch.randn(n * L, ldz, generator=g) * 8.0 + off).float()
    z[:, V:] = float("nan")
    t = torch.randint(0, V - 1, (n, L), generator=g)
    t = t + (t >= PAD).long()                                   # uniform over the non-<pad> columns
    special, planted = set(), []
    if L >= 2:
        t[0, 0], t[0, 1] = 0, V - 1
        special |= {(0, 0), (0, 1)}
        z[1, 3] = z[1, V - 1]                                   # a lower column equal to the target: it ranks first
        planted.append("edge columns")
    if L >= 5:
        t[0, 2], t[0, 3], t[0, L - 1] = PAD, V + 5, PAD
        special |= {(0, 2), (0, 3), (0, L - 1)}
        planted.append("pads")
    if L >= 9:
        t[0, 5], t[0, 6] = -1, 2 ** 40
        special |= {(0, 5), (0, 6)}
    if n >= 2:
        t[n - 1, :] = PAD
        planted.append("all-pad sequence")
    free = [(s, l) for s in range(max(1, n - 1)) for l in range(L) if (s, l) not in special]
    if free:                                                    # the target between two columns that equal it
        s, l = free[0]
        tt = V // 2
        t[s, l] = tt
        r = s * L + l
        z[r, tt - 2] = z[r, tt]
        z[r, tt + 2] = z[r, tt]
        planted.append("two-sided tie")
    if len(free) >= 2 or L >= 2:                                # a duplicated maximum (the target is one of the two where it is column 0)
        s, l = free[1] if len(free) >= 2 else (0, 0)
        r = s * L + l
        top = z[r, :V].max() + 1.0
        z[r, 0] = top
        z[r, V - 1] = top
        planted.append("duplicated maximum")
    return z, t, planted


def valid_targets(target, V, pad=PAD):
    return (target != pad) & (target >= 0) & (target < V)


def _score(zz, target, V, pad):
    n, L = target.shape
    t = target.reshape(-1)
    ok = valid_targets(t, V, pad)
    ts = torch.where(ok, t, torch.zeros_like(t))
    zt = zz.gather(1, ts.unsqueeze(1)).squeeze(1)
    mx = zz.max(1).values
    lse = mx + (zz - mx.unsqueeze(1)).exp().sum(1).log()
    logp = torch.where(ok, zt - lse, torch.zeros_like(zt))
    cols = torch.arange(V).unsqueeze(0)
    before = (zz > zt.unsqueeze(1)) | ((zz == zt.unsqueeze(1)) & (cols < ts.unsqueeze(1)))
    rank = torch.where(ok, before.sum(1), torch.full_like(t, -1)).to(torch.int32)
    return logp.view(n, L), rank.view(n, L), ok.view(n, L)


def score_ref64(logits, target, V, pad=PAD):
    """float64: (tok_logp [n_seq, L], tok_rank int32 [n_seq, L], seq_logp [n_seq], seq_len int32 [n_seq])."""
    logp, rank, ok = _score(logits[:, :V].double(), target, V, pad)
    return logp, rank, seq_sum64(logp), ok.sum(1).to(torch.int32)


def seq_sum64(tok_logp):
    """Per sequence the float64 sum of tok_logp in ascending position, one addition at a time (the kernel's order)."""
    out = torch.zeros(tok_logp.size(0), dtype=torch.float64)
    for l in range(tok_logp.size(1)):
        out = out + tok_logp[:, l].double()
    return out


def closed_form_f32(logits, target, V, pad=PAD):
    """The same closed form (max-shifted logsumexp, z[t] - lse) in float32 with torch on the CPU: tok_logp.  Not a reference: the
    yardstick for what float32 delivers on this formula."""
    return _score(logits[:, :V].float(), target, V, pad)[0]


# What float32 delivers: the worst |closed_form_f32 - score_ref64| of tok_logp over score_cases() (seeds SCORE_SEED + index), measured
# with torch on a CPU.  The logits with a common offset of +50 set it: half an ulp of lse ~ 80 is 3.8e-6, and z[t] - lse rounds once
# more.  tests/test_score_refs.py re-measures it (within a factor 2: summation order differs between CPUs); the GPU test holds the
# kernel to 4 x this.
CPU_F32_TOK_LOGP_ABS = 3.55e-6
