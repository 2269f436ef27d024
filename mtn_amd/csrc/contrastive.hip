// contrastive.hip — contrastive search (Su et al. 2022): the selection and bookkeeping of one generated token for dialogues that each own
// k consecutive session rows, one candidate per row.  include/mtn_hip.h mtn_contrastive_advance holds the definition; this launch stands
// where mtn_beam_advance (select.hip) stands in a captured search, after the decoder's final norm, the generator and mtn_topk_rows.
//
// One workgroup of 16 waves per dialogue.  A row's degeneration penalty is the largest cosine between its candidate state h[r][l] and its
// prefix states h[r][0..l): row r is served by 16 / k waves, each holds the candidate state in registers (element 4 * (lane + 64 t) + c in
// lane `lane`, chunk t, component c — on the 16-byte path one load, on the scalar path four) and walks its share of the prefix positions
// two at a time, so the loads of one pair fly while the other is reduced.  Every sum runs chunk by chunk, component by component, then
// through a wave-64 butterfly: its order is a function of d alone, on either path.  The per-wave maxima, the k scores and the winner go
// through LDS; wave 0 then stores the chosen token into the k rows and deals the winner's head to them by a ballot over the head's
// entries.  The workgroup reads and writes only its own dialogue's words (workgroup 0 also stores *pos, which no launch of this kernel
// reads).  No atomics; every store is a vector store.
#include "common.h"
#include <cmath>

static constexpr int CS_MAX_K = 16;                              // rows of a dialogue, and entries of a row's head
static constexpr int CS_WAVES = 16, CS_THREADS = 64 * CS_WAVES;
static constexpr int CS_CHUNKS = 4, CS_MAX_D = 256 * CS_CHUNKS;  // a lane holds CS_CHUNKS x 4 elements of the candidate state
static constexpr int CS_MAX_L = 1 << 20;

struct ContrastiveArgs { mtn_contrastive_args a; };

// elements e .. e + 3 of a state (e < d; past d: 0)
template <bool VEC> __device__ __forceinline__ float4 cs_load4(const float* __restrict__ p, int e, int d) {
    if (VEC) return *(const float4*)(p + e);
    float4 v;
    v.x = p[e];
    v.y = e + 1 < d ? p[e + 1] : 0.f;
    v.z = e + 2 < d ? p[e + 2] : 0.f;
    v.w = e + 3 < d ? p[e + 3] : 0.f;
    return v;
}
__device__ __forceinline__ float cs_dot4(const float4& a, const float4& b, float acc) {
    acc = fmaf(a.x, b.x, acc);
    acc = fmaf(a.y, b.y, acc);
    acc = fmaf(a.z, b.z, acc);
    return fmaf(a.w, b.w, acc);
}
// max that keeps a NaN: a row with a NaN cosine has a NaN penalty
__device__ __forceinline__ float cs_max(float a, float b) { return a != a ? a : (b != b ? b : fmaxf(a, b)); }
__device__ __forceinline__ float cs_cos(float dot, float cn, float hn) { return (cn == 0.f || hn == 0.f) ? 0.f : dot / (sqrtf(cn) * sqrtf(hn)); }

template <bool VEC> __global__ __launch_bounds__(CS_THREADS) void contrastive_advance_kernel(const ContrastiveArgs CA) {
    const mtn_contrastive_args& A = CA.a;
    __shared__ float s_pen[CS_MAX_K][CS_WAVES];                  // per row: the maxima of the waves that serve it
    __shared__ float s_score[CS_MAX_K], s_penr[CS_MAX_K], s_lp[CS_MAX_K];
    __shared__ int s_ok[CS_MAX_K];
    __shared__ int s_win, s_deal;
    __shared__ long s_y;
    const int dlg = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int k = A.k, L = A.L, d = A.d, D = gridDim.x, base = dlg * k;
    const int l = A.step[dlg];
    const int next = l < 0x7fffffff ? l + 1 : l;
    const bool live = !A.done[dlg] && l >= 0 && l < L;
    __syncthreads();                                             // every thread holds the step before thread 0 advances it
    if (tid == 0) {
        A.step[dlg] = next;
        if (dlg == 0) *A.pos = (long)min(max(next, 0), L - 1);   // (read by the NEXT decoder pass only)
    }
    if (!live) return;

    if (l >= 1) {
        // 1. the rows' penalties: wave -> (row, its share of the prefix positions)
        const int nw = CS_WAVES / k, r = wave % k, s = wave / k;
        if (s < nw) {
            const float* hr = A.hidden + (size_t)(base + r) * A.row_stride;
            const float* hc = hr + (size_t)l * A.pos_stride;
            float4 c[CS_CHUNKS];
            float cn = 0.f;
#pragma unroll
            for (int t = 0; t < CS_CHUNKS; ++t) {
                const int e = 4 * (lane + 64 * t);
                c[t] = e < d ? cs_load4<VEC>(hc, e, d) : make_float4(0.f, 0.f, 0.f, 0.f);
                cn = cs_dot4(c[t], c[t], cn);
            }
            cn = wave_sum(cn);
            float pen = -INFINITY;
            for (int j = s; j < l; j += 2 * nw) {
                const bool two = j + nw < l;
                const float* ha = hr + (size_t)j * A.pos_stride;
                const float* hb = hr + (size_t)(two ? j + nw : j) * A.pos_stride;
                float da = 0.f, na = 0.f, db = 0.f, nb = 0.f;
#pragma unroll
                for (int t = 0; t < CS_CHUNKS; ++t) {
                    const int e = 4 * (lane + 64 * t);
                    if (e < d) {
                        const float4 a = cs_load4<VEC>(ha, e, d), b = cs_load4<VEC>(hb, e, d);
                        da = cs_dot4(c[t], a, da); na = cs_dot4(a, a, na);
                        db = cs_dot4(c[t], b, db); nb = cs_dot4(b, b, nb);
                    }
                }
                da = wave_sum(da); na = wave_sum(na);
                db = wave_sum(db); nb = wave_sum(nb);
                pen = cs_max(pen, cs_cos(da, cn, na));
                if (two) pen = cs_max(pen, cs_cos(db, cn, nb));
            }
            if (lane == 0) s_pen[r][s] = pen;
        }
        __syncthreads();
        // 2. the k scores: s_r = fl32(fl32((1 - alpha) * expf(cand_logp[r])) - fl32(alpha * pen_r)), two multiplies and a subtract
        if (tid < k) {
            float pen = s_pen[tid][0];
            for (int q = 1; q < nw; ++q) pen = cs_max(pen, s_pen[tid][q]);
            const float lp = A.cand_logp[base + tid];
            const float sc = __fsub_rn(__fmul_rn(__fsub_rn(1.f, A.alpha), expf(lp)), __fmul_rn(A.alpha, pen));
            s_penr[tid] = pen; s_lp[tid] = lp; s_score[tid] = sc;
            s_ok[tid] = (sc == sc) && !(lp == -INFINITY);
        }
        __syncthreads();
    }
    // 3. the winner (ties to the lowest row; nobody can win: row 0), the step log, done
    if (tid == 0) {
        int win = 0, deal = next < L;
        if (l >= 1) {
            win = -1;
            for (int r = 0; r < k; ++r)
                if (s_ok[r] && (win < 0 || s_score[r] > s_score[win])) win = r;
            if (win < 0) win = 0;
            const long y = A.tokens[(size_t)(base + win) * L + l];
            const size_t at = (size_t)l * D + dlg;
            A.log_tok[at] = (int)y; A.log_logp[at] = s_lp[win]; A.log_pen[at] = s_penr[win]; A.log_rank[at] = win;
            if (y == (long)A.eos) { A.done[dlg] = 1; deal = 0; }
            s_y = y;
        }
        s_win = win; s_deal = deal;
    }
    __syncthreads();
    if (wave != 0) return;
    // 4. the chosen token into the k rows; the winner's head dealt to them as the candidates of position l + 1
    if (l >= 1 && lane < k) A.tokens[(size_t)(base + lane) * L + l] = s_y;
    if (!s_deal) return;
    const int k1 = A.k_top;
    const float* row = A.top + (size_t)(base + s_win) * (2 * k1 + 1);
    float v = -INFINITY;
    int col = 0;
    bool adm = false;
    if (lane < k1) {
        v = row[lane];
        col = (int)row[k1 + lane];
        adm = !(col == A.eos && l < A.min_len);
        for (int q = 0; q < A.n_banned; ++q) adm = adm && col != A.banned[q];
    }
    const unsigned long long m = __ballot(adm);
    const int n_adm = __popcll(m), rank = __popcll(m & ((1ull << lane) - 1ull));
    if (adm && rank < k) {
        A.tokens[(size_t)(base + rank) * L + l + 1] = (long)col;
        A.cand_logp[base + rank] = v;
    }
    // fewer than k admitted entries: the other rows repeat the last admitted column (nothing admitted: the head's first column) and never win
    const int lastcol = __shfl(col, n_adm > 0 ? 63 - __clzll(m) : 0, 64);
    if (lane >= n_adm && lane < k) {
        A.tokens[(size_t)(base + lane) * L + l + 1] = (long)lastcol;
        A.cand_logp[base + lane] = -INFINITY;
    }
}

static bool cs_aligned(const void* p, uintptr_t a) { return (((uintptr_t)p) & (a - 1)) == 0; }

extern "C" int mtn_contrastive_advance(const mtn_contrastive_args* a, void* stream) {
    MTN_CHECK_ARG(a, "null arguments");
    MTN_CHECK_ARG(a->hidden && a->top && a->tokens && a->pos && a->cand_logp && a->step && a->done, "null buffer");
    MTN_CHECK_ARG(a->log_tok && a->log_logp && a->log_pen && a->log_rank, "null log buffer");
    MTN_CHECK_ARG(cs_aligned(a->hidden, 4) && cs_aligned(a->top, 4) && cs_aligned(a->cand_logp, 4) && cs_aligned(a->step, 4) && cs_aligned(a->done, 4)
                  && cs_aligned(a->log_tok, 4) && cs_aligned(a->log_logp, 4) && cs_aligned(a->log_pen, 4) && cs_aligned(a->log_rank, 4),
                  "hidden, top, cand_logp, step, done and the logs must be 4-byte aligned");
    MTN_CHECK_ARG(cs_aligned(a->tokens, 8) && cs_aligned(a->pos, 8), "tokens and pos must be 8-byte aligned");
    MTN_CHECK_ARG(a->dialogues >= 0 && a->k >= 1 && a->k <= CS_MAX_K, "dialogues >= 0, 1 <= k <= 16");
    MTN_CHECK_ARG(a->L >= 1 && a->L <= CS_MAX_L && a->d >= 1 && a->d <= CS_MAX_D, "1 <= L <= 2^20, 1 <= d <= 1024");
    MTN_CHECK_ARG(a->n_banned >= 0 && a->n_banned <= 4, "at most 4 banned tokens");
    MTN_CHECK_ARG(a->k_top >= 1 && a->k_top <= CS_MAX_K && a->k_top >= (a->k + a->n_banned + 1 < CS_MAX_K ? a->k + a->n_banned + 1 : CS_MAX_K),
                  "min(16, k + n_banned + 1) <= k_top <= 16 (k candidates behind every entry that may be barred)");
    MTN_CHECK_ARG(a->alpha >= 0.0f && a->alpha <= 1.0f, "alpha must be finite and in [0, 1]");
    MTN_CHECK_ARG(a->pos_stride >= a->d && a->row_stride >= (long)(a->L - 1) * a->pos_stride + a->d,
                  "pos_stride >= d and row_stride >= (L - 1) * pos_stride + d (the dense strides at least)");
    MTN_CHECK_ARG((long)a->dialogues * a->k <= 0x7fffffffL, "dialogues * k must fit an int");
    if (a->dialogues == 0) return MTN_OK;
    ContrastiveArgs CA; CA.a = *a;
    const bool vec = (a->d & 3) == 0 && (a->row_stride & 3) == 0 && (a->pos_stride & 3) == 0 && cs_aligned(a->hidden, 16);
    if (vec)
        hipLaunchKernelGGL(contrastive_advance_kernel<true>, dim3(a->dialogues), dim3(CS_THREADS), 0, (hipStream_t)stream, CA);
    else
        hipLaunchKernelGGL(contrastive_advance_kernel<false>, dim3(a->dialogues), dim3(CS_THREADS), 0, (hipStream_t)stream, CA);
    MTN_CHECK_LAUNCH();
    return MTN_OK;
}
