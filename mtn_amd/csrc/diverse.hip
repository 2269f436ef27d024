// diverse.hip — diverse (group) beam search, Hamming diversity (Vijayakumar et al. 2016): the hypothesis bookkeeping of one step for a
// dialogue whose beam of B hypotheses is split into G groups of B' = B / G.  include/mtn_hip.h mtn_diverse_advance holds the definition;
// this launch stands where mtn_beam_advance (select.hip) stands in the captured search, one for one.
//
// The groups of a dialogue depend on each other within a step — group g is penalised by the tokens the FINAL new beams of groups 0..g-1
// hold — so one workgroup (one wave) owns a real dialogue and walks its groups in order.  Per group the wave penalises the heads of the
// live rows and rank-sorts them (one lane per head entry, <= 16 x 16 of them), then lane 0 walks the candidates exactly as
// beam_advance_kernel does; the tokens chosen so far at this step (<= 16) sit in LDS.  After the last group the ancestor table of all
// B rows is updated in beam_advance_kernel's chunks: parents never cross groups.  The state and the step log are written in
// mtn_beam_advance's layout for D * G pseudo-dialogues of width B', so the host rebuild and mtn_constrain_rows' log walk read them as
// they are.  No atomics; every store is a vector store.
#include "common.h"
#include <cmath>

static constexpr int DIV_MAX = 16;                              // rows of a real dialogue, and entries of a row's head

struct DiverseArgs { mtn_diverse_args a; };
__global__ __launch_bounds__(64) void diverse_advance_kernel(const DiverseArgs DA) {
    const mtn_beam_args& A = DA.a.beam;
    __shared__ int s_anc[DIV_MAX * 64];                          // the parents' ancestor rows, in chunks of 64 positions
    __shared__ float s_pv[DIV_MAX][DIV_MAX], s_sv[DIV_MAX][DIV_MAX];   // a group's penalised heads: in head order, then sorted
    __shared__ int s_po[DIV_MAX][DIV_MAX], s_so[DIV_MAX][DIV_MAX];     // ... and their columns
    __shared__ int s_chosen[DIV_MAX], s_nch;                     // newest tokens of the final new beams of the groups before this one
    __shared__ int s_parent[DIV_MAX];                            // row of the dialogue -> its parent's row of the dialogue, -1: not live
    __shared__ int s_tie;
    const int G = DA.a.groups, Bp = A.width, B = Bp * G, DG = A.dialogues, W = DG * Bp;
    const int d = blockIdx.x, tid = threadIdx.x, dbase = d * B, k1 = A.k_top, cols = 2 * k1 + 1;
    const float lam = DA.a.diversity;
    const int l = A.step[d * G];                                 // the groups of a dialogue step together
    if (l < 0 || l >= A.L) return;                               // (a search issues exactly L steps: nothing to log beyond them)
    if (tid < DIV_MAX) s_parent[tid] = -1;
    if (tid == 0) { s_nch = 0; s_tie = 0; }
    for (int g = 0; g < G; ++g) {
        const int p = d * G + g, base = dbase + g * Bp;
        const int n = min(max(A.n_live[p], 0), Bp);
        __syncthreads();                                         // s_chosen / s_nch of the groups before
        const int nch = s_nch;
        // 1. penalise: r' = fl32(r - fl32(lambda * count)), one multiply and one subtract (never an fma)
        for (int e = tid; e < n * k1; e += 64) {
            const int h = e / k1, i = e - h * k1;
            const float* row = A.top + (size_t)(base + h) * cols;
            const float v = row[i];
            const int o = (int)row[k1 + i];
            int c = 0;
            for (int q = 0; q < nch; ++q) c += s_chosen[q] == o;
            s_pv[h][i] = __fsub_rn(v, __fmul_rn(lam, (float)c));
            s_po[h][i] = o;
            if (i + 1 < k1 && v == row[i + 1]) s_tie = 1;        // equal values before the penalty
        }
        __syncthreads();
        // 2. + 3. stable descending rank sort; any equal pair after the penalty is a tie
        for (int e = tid; e < n * k1; e += 64) {
            const int h = e / k1, i = e - h * k1;
            const float v = s_pv[h][i];
            int rank = 0, eq = 0;
            for (int j = 0; j < k1; ++j) {
                const float u = s_pv[h][j];
                rank += (u > v) || (u == v && j < i);
                eq |= (u == v) && j != i;
            }
            s_sv[h][rank] = v;
            s_so[h][rank] = s_po[h][i];
            if (eq) s_tie = 1;
        }
        __syncthreads();
        // 4. the walk of beam_advance_kernel on this group's hypotheses, beam B'
        if (tid == 0) {
            int np[DIV_MAX], nt[DIV_MAX]; double ns[DIV_MAX];
            int cnt = 0, argmin = 0;
            A.log_n_old[l * DG + p] = n;
            for (int h = 0; h < n; ++h) {
                const double lp = A.lp[base + h];
                const float eosv = A.top[(size_t)(base + h) * cols + 2 * k1];            // r[eos]: <eos> is never chosen, its count is 0
                if (l >= A.min_len) A.log_done[(size_t)l * W + base + h] = (double)(float)((double)eosv + lp) + A.penalty * (double)(l + 1);
                for (int i = 0; i < A.k; ++i) {
                    const int o = s_so[h][i];
                    if (o == A.unk || o == A.eos) continue;
                    const double sc = (double)(float)((double)s_sv[h][i] + lp);
                    if (cnt == A.beam) {
                        if (ns[argmin] < sc) {
                            np[argmin] = h; nt[argmin] = o; ns[argmin] = sc;
                            argmin = 0;
                            for (int q = 1; q < cnt; ++q) if (ns[q] < ns[argmin]) argmin = q;
                        } else break;
                    } else {
                        np[cnt] = h; nt[cnt] = o; ns[cnt] = sc; ++cnt;
                        if (cnt == A.beam) { argmin = 0; for (int q = 1; q < cnt; ++q) if (ns[q] < ns[argmin]) argmin = q; }
                    }
                }
            }
            int nc = s_nch;
            for (int i = 0; i < Bp; ++i) {
                const size_t at = (size_t)l * W + base + i;
                A.tokens[base + i] = i < cnt ? (long)nt[i] : (long)A.pad;
                if (i < cnt) {
                    A.lp[base + i] = ns[i]; A.log_parent[at] = np[i]; A.log_tok[at] = nt[i]; A.log_score[at] = ns[i];
                    s_parent[g * Bp + i] = g * Bp + np[i];
                    s_chosen[nc++] = nt[i];                       // (nc <= B <= 16)
                }
            }
            s_nch = nc;
            A.log_n_new[l * DG + p] = cnt;
            A.n_live[p] = cnt;
            A.step[p] = l + 1;
        }
    }
    __syncthreads();
    if (tid == 0) {
        if (s_tie) A.flags[0] = 1;
        if (d == 0) *A.pos = l + 1;                              // (read by the NEXT decode step only)
    }
    // ancestor table of the dialogue's B rows: row i takes its parent's slots for positions 0..l and its own slot for position l + 1
    // (all reads before any write)
    const int npos = l + 1;
    for (int c0 = 0; c0 < npos; c0 += 64) {
        const int t = c0 + tid;
        for (int i = 0; i < B; ++i) if (t < npos && s_parent[i] >= 0) s_anc[i * 64 + tid] = A.anc[(size_t)(dbase + s_parent[i]) * A.L + t];
        __syncthreads();
        for (int i = 0; i < B; ++i) if (t < npos && s_parent[i] >= 0) A.anc[(size_t)(dbase + i) * A.L + t] = s_anc[i * 64 + tid];
        __syncthreads();
    }
    if (tid < B && s_parent[tid] >= 0 && npos < A.L) A.anc[(size_t)(dbase + tid) * A.L + npos] = dbase + tid;
}

extern "C" int mtn_diverse_advance(const mtn_diverse_args* da, void* stream) {
    MTN_CHECK_ARG(da, "null arguments");
    const mtn_beam_args* a = &da->beam;
    MTN_CHECK_ARG(a->top && a->tokens && a->pos && a->anc && a->lp && a->n_live && a->step && a->flags, "null buffer");
    MTN_CHECK_ARG(a->log_parent && a->log_tok && a->log_score && a->log_done && a->log_n_old && a->log_n_new, "null log buffer");
    MTN_CHECK_ARG(da->groups >= 1 && a->dialogues >= 1 && a->dialogues % da->groups == 0, "groups >= 1 and dialogues = real dialogues x groups");
    MTN_CHECK_ARG(a->width >= 1 && a->width <= DIV_MAX && a->width * da->groups <= DIV_MAX && a->beam >= 1 && a->beam <= a->width, "1 <= beam <= width, width x groups <= 16");
    MTN_CHECK_ARG(a->k_top <= DIV_MAX && a->k_top >= a->width * da->groups + 3, "width x groups + 3 <= k_top <= 16 (beam + 2 entries and the tie sentinel)");
    MTN_CHECK_ARG(a->k >= 1 && a->k <= a->k_top && a->L >= 1, "1 <= k <= k_top");
    MTN_CHECK_ARG(std::isfinite(da->diversity) && da->diversity >= 0.f, "the diversity penalty is finite and >= 0");
    DiverseArgs DA; DA.a = *da;
    hipLaunchKernelGGL(diverse_advance_kernel, dim3(a->dialogues / da->groups), dim3(64), 0, (hipStream_t)stream, DA);
    MTN_CHECK_LAUNCH();
    return MTN_OK;
}
