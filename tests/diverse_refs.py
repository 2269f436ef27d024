"""numpy form of diverse (group) beam search as include/mtn_hip.h mtn_diverse_advance defines it: a beam of B hypotheses per dialogue
split into G groups of B' = B / G, processed in order within a step; group g reads its rows lowered by lambda x (how many hypotheses of
the final new beams of groups 0..g-1 at this step end in that token) — fl32(r - fl32(fl32(lambda) * count)) — and then takes exactly the
reference's step (data_utils.py:209-240) with beam B'.

`State` + `advance` are one step in the device layout (what csrc/diverse.hip writes: D * G pseudo-dialogues of width B'), from the rows'
heads (as mtn_topk_rows packs them) or from full rows; `search` is a whole search on python lists driven by a ``rows(prefix_lists)``
callable, with the pooled n-best of the definition; `seeded_rows` / `tie_rows` are the inputs of tests/test_diverse_kernel_gpu.py."""
import numpy as np

F32, F64 = np.float32, np.float64


def penalise(values, tokens, chosen, lam):
    """fl32(values - fl32(fl32(lam) * count(token in chosen))) — one fp32 multiply, one fp32 subtract."""
    c = np.array([chosen.count(int(t)) for t in tokens], dtype=F32)
    return (np.asarray(values, dtype=F32) - (F32(lam) * c).astype(F32)).astype(F32)


def heads_of(rows, k_top, eos):
    """What mtn_topk_rows leaves per row: [k_top values, descending, equal values by ascending column | their columns | row[eos]]."""
    rows = np.asarray(rows, dtype=F32)
    out = np.zeros((rows.shape[0], 2 * k_top + 1), dtype=F32)
    for i, r in enumerate(rows):
        order = np.argsort(-r.astype(F64), kind="stable")[:k_top]
        out[i, :k_top], out[i, k_top:2 * k_top], out[i, 2 * k_top] = r[order], order.astype(F32), r[eos]
    return out


def group_step(hyp_lp, cands, eos_vals, l, beam, unk, eos, penalty, min_len):
    """The reference's step for one group.  hyp_lp: score per live hypothesis; cands[h]: (token, fp32 penalised value) in visiting order;
    eos_vals[h]: r[eos].  -> (new beam [(parent, token, score)], finished scores per hypothesis or None)."""
    new, argmin, done = [], 0, None
    if l >= min_len:
        done = [float(F32(F64(e) + F64(lp))) + penalty * (l + 1) for e, lp in zip(eos_vals, hyp_lp)]
    for h, lp in enumerate(hyp_lp):
        for o, v in cands[h]:
            if o == unk or o == eos:
                continue
            s = float(F32(F64(v) + F64(lp)))
            if len(new) == beam:
                if new[argmin][2] < s:
                    new[argmin] = (h, int(o), s)
                    argmin = min(range(len(new)), key=lambda i: new[i][2])
                else:
                    break
            else:
                new.append((h, int(o), s))
                if len(new) == beam:
                    argmin = min(range(len(new)), key=lambda i: new[i][2])
    return new, done


def head_candidates(head, k_top, k, chosen, lam):
    """Head path: penalise the k_top entries, re-sort stable descending, visit the first k.  -> (candidates, tie?)"""
    v, o = head[:k_top].astype(F32), head[k_top:2 * k_top].astype(np.int64)
    tie = bool((v[1:] == v[:-1]).any())
    pv = penalise(v, o, chosen, lam)
    order = sorted(range(k_top), key=lambda j: -float(pv[j]))               # (sorted() is stable; -inf stays last)
    sv = pv[order]
    tie = tie or bool((sv[1:] == sv[:-1]).any())
    return [(int(o[j]), pv[j]) for j in order[:k]], tie


def row_candidates(row, lp, chosen, lam):
    """Full-row path: the reference's argsort (data_utils.py:219) of the penalised row plus the hypothesis' score, rounded to float32."""
    pv = np.asarray(row, dtype=F32).copy()
    for t in set(chosen):
        pv[t] = penalise(pv[t:t + 1], [t], chosen, lam)[0]
    lp_vec = (pv.astype(F64) + lp).astype(F32)
    return [(int(o), pv[o]) for o in np.argsort(lp_vec)[::-1]]


class State:
    """Device state and step log of a search, in mtn_beam_advance's layout for D * G pseudo-dialogues of width B'."""

    def __init__(self, D, B, G, L, start, pad):
        assert B % G == 0
        self.D, self.B, self.G, self.Bp, self.L, self.pad = D, B, G, B // G, L, pad
        W, DG = D * B, D * G
        self.tokens = np.full(W, pad, dtype=np.int64)
        self.tokens[::self.Bp] = start
        self.pos = 0
        self.anc = np.tile(np.arange(W, dtype=np.int32)[:, None], (1, L))
        self.lp = np.zeros(W, dtype=F64)
        self.n_live, self.step = np.ones(DG, dtype=np.int32), np.zeros(DG, dtype=np.int32)
        self.log_parent, self.log_tok = np.zeros((L, W), dtype=np.int32), np.zeros((L, W), dtype=np.int32)
        self.log_score, self.log_done = np.zeros((L, W), dtype=F64), np.zeros((L, W), dtype=F64)
        self.log_n_old, self.log_n_new = np.zeros((L, DG), dtype=np.int32), np.zeros((L, DG), dtype=np.int32)
        self.flag = 0


def advance(st, k_top, k, unk, eos, penalty, min_len, lam, heads=None, rows=None):
    """One step for every dialogue of ``st``: heads (W, 2 k_top + 1) — the device path — or full rows (W, V)."""
    Bp, G = st.Bp, st.G
    anc_old = st.anc.copy()
    for d in range(st.D):
        chosen = []
        for g in range(G):
            p, base = d * G + g, d * st.B + g * Bp
            n, l = int(st.n_live[p]), int(st.step[p])
            lps = [float(st.lp[base + h]) for h in range(n)]
            if heads is not None:
                cands = []
                for h in range(n):
                    c, tie = head_candidates(heads[base + h], k_top, k, chosen, lam)
                    cands.append(c)
                    st.flag |= int(tie)
                eos_vals = [heads[base + h, 2 * k_top] for h in range(n)]
            else:
                cands = [row_candidates(rows[base + h], lps[h], chosen, lam) for h in range(n)]
                eos_vals = [rows[base + h][eos] for h in range(n)]
            new, done = group_step(lps, cands, eos_vals, l, Bp, unk, eos, penalty, min_len)
            st.log_n_old[l, p] = n
            if done is not None:
                st.log_done[l, base:base + n] = done
            st.tokens[base:base + Bp] = st.pad
            for i, (par, tok, s) in enumerate(new):
                st.tokens[base + i], st.lp[base + i] = tok, s
                st.log_parent[l, base + i], st.log_tok[l, base + i], st.log_score[l, base + i] = par, tok, s
                st.anc[base + i, :l + 1] = anc_old[base + par, :l + 1]
                if l + 1 < st.L:
                    st.anc[base + i, l + 1] = base + i
            st.log_n_new[l, p] = st.n_live[p] = len(new)
            st.step[p] = l + 1
            st.pos = l + 1
            chosen += [tok for _, tok, _ in new]


def pool(done, nbest):
    """Finished hypotheses in append order -> identical token lists once (highest score, first on equal), sorted by score, stable."""
    best = {}
    for i, (toks, s) in enumerate(done):
        j = best.get(tuple(toks))
        if j is None or done[j][1] < s:
            best[tuple(toks)] = i
    kept = [done[i] for i in sorted(best.values())]
    if not kept:
        return [([], 0)], None
    return sorted(kept, key=lambda h: -h[1])[:nbest], max(h[1] for h in kept)


def search(rows, D, B, G, lam, max_len, start, unk, eos, penalty, min_len, nbest, trace=None):
    """A whole search.  ``rows(prefix_lists)``: prefix_lists[d] = the live prefixes (with <sos>) of dialogue d in (group, hypothesis) order
    -> per dialogue an (n_d, V) array of log-probabilities.  Full-row path.  trace (a list) receives per step, dialogue and group the
    tokens placed."""
    Bp = B // G
    hyps = [[[([], 0.0)] for _ in range(G)] for _ in range(D)]              # [d][g] -> [(generated tokens, score)]
    done = [[] for _ in range(D)]
    for l in range(max_len):
        out = rows([[[start] + t for grp in hyps[d] for t, _ in grp] for d in range(D)])
        for d in range(D):
            r, chosen, o = np.asarray(out[d], dtype=F32), [], 0
            for g in range(G):
                grp = hyps[d][g]
                lps = [s for _, s in grp]
                cands = [row_candidates(r[o + h], lps[h], chosen, lam) for h in range(len(grp))]
                new, fin = group_step(lps, cands, [r[o + h][eos] for h in range(len(grp))], l, Bp, unk, eos, penalty, min_len)
                if fin is not None:
                    done[d] += [(grp[h][0], fin[h]) for h in range(len(grp))]
                o += len(grp)
                hyps[d][g] = [(grp[par][0] + [tok], s) for par, tok, s in new]
                chosen += [tok for _, tok, _ in new]
                if trace is not None:
                    trace.append((l, d, g, [tok for _, tok, _ in new]))
    return [pool(done[d], nbest) for d in range(D)]


# ---------------------------------------------------------------- inputs of the kernel test
KERNEL_V = (300, 3004)
KERNEL_SHAPES = ((1, 4, 2), (2, 4, 4), (2, 6, 3), (1, 6, 2), (1, 12, 4), (3, 4, 2))      # (D, B, G)
KERNEL_LAMBDAS = (0.0, 0.5, 64.0)
KERNEL_STEPS, KERNEL_L = 6, 8
START, UNK, EOS, PAD = 2, 0, 3, 1
MIN_LEN, PENALTY = 2, 1.0


def seeded_rows(V, D, B, G, step, seed=0):
    """(D * B, V) fp32 log-softmaxed rows of one step: a function of the arguments alone.  The rows of a dialogue share most of their
    logits, as the rows of one dialogue's hypotheses do, so its groups want the same tokens and the penalty decides."""
    rng = np.random.default_rng([seed, V, D, B, G, step])
    z = np.repeat(rng.standard_normal((D, V)) * 3.0, B, axis=0) + rng.standard_normal((D * B, V)) * 0.3
    z -= z.max(axis=1, keepdims=True)
    return (z - np.log(np.exp(z).sum(axis=1, keepdims=True))).astype(F32)


def tie_rows(V, W):
    """Rows of multiples of 0.5, all different within a row: with lambda = 0.5 a penalised entry meets the next one."""
    perm = np.random.default_rng(7).permutation(V)
    row = np.empty(V, dtype=F32)
    row[perm] = -0.5 * np.arange(V, dtype=F32)
    return np.tile(row, (W, 1))
