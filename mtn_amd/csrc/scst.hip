// scst.hip — what self-critical sequence training (Rennie et al. 2017; the leave-one-out baseline of Luo 2020) needs on the device between
// the sampling search (sample.hip) and the optimiser: include/mtn_hip.h states every formula.
//   mtn_scst_assemble         the sample log -> teacher-forcing targets and the int32 rows the reward launch reads (a wave per row)
//   mtn_eval_table_build      the document-frequency table of a fixed reference corpus, once (eval_common.h's clear and table bodies)
//   mtn_eval_score_rows       N hypotheses, each against the references of the corpus item it names (eval_common.h's item body: the
//                             launch reads the table and never writes it, no atomics, double with fixed-order sums)
//   mtn_scst_advantage        rewards -> signed row weights -(r - b), b a given baseline or the leave-one-out mean
//   mtn_wlosshead_fwd / _bwd  the loss head with a signed weight per row and a smoothing per segment.  A segment without weights at the
//                             loss head's smoothing runs losshead.hip's arithmetic, statement for statement (the weight is applied by
//                             a multiplication of its own, which cannot be contracted into anything), so its bits are the loss head's.
// One 64-lane wave per loss-head row, float4 loads, wave-shuffle reductions in a fixed order, no atomics; HBM/L2-bound as losshead.hip.
#include "eval_common.h"

#include <math.h>

// ------------------------------------------------------------------------------------------ weighted loss head
struct WRow {
    int seg, local;      // segment (stream) and row inside it
    long t;
    float scale;         // coef / norm
    float eps, conf;     // the segment's smoothing
    bool zero_row, t_is_pad;
    bool weighted;       // the segment has weights
    float w;
};

__device__ __forceinline__ WRow wrow_info(const mtn_wlosshead_args& A, int row, int lane) {
    WRow r;
    int base = 0;
    r.seg = 0;
    for (int s = 0; s < A.n_seg; ++s) {
        if (row >= base && row < base + A.rows[s]) { r.seg = s; break; }
        base += A.rows[s];
    }
    r.local = row - base;
    r.t = A.target[r.seg][r.local];
    r.scale = A.coef[r.seg] / *A.norm[r.seg];
    r.t_is_pad = (r.t == A.pad);
    r.zero_row = false;
    if (r.t_is_pad) {
        if (r.local > 0) r.zero_row = true;                 // its own index makes the index sum positive
        else {                                              // flat row 0: zeroed only if another <pad> row exists
            int any = 0;
            for (int i = 1 + lane; i < A.rows[r.seg]; i += 64) any |= (A.target[r.seg][i] == A.pad);
            r.zero_row = __any(any);
        }
    }
    const float sm = A.smoothing_seg[r.seg] >= 0.f ? A.smoothing_seg[r.seg] : A.smoothing;
    r.eps = sm / (float)(A.V - 2);
    r.conf = 1.0f - sm;
    r.weighted = A.roww[r.seg] != nullptr;
    r.w = r.weighted ? A.roww[r.seg][r.local] : 1.0f;
    if (r.w == 0.f) r.zero_row = true;                      // +0.0 everywhere, whatever the row holds
    return r;
}

__global__ __launch_bounds__(256) void wlosshead_fwd_kernel(const mtn_wlosshead_args A, int total_rows) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= total_rows) return;
    const WRow r = wrow_info(A, row, lane);
    const float* z = A.logits + (size_t)row * A.ldz;
    const int V = A.V;
    float mx = -INFINITY, S = 0.f;
    for (int c = lane * 4; c < V; c += 256) {
        float4 v = *(const float4*)(z + c);                 // V % 4 == 0 (checked on the host)
        mx = fmaxf(fmaxf(mx, fmaxf(v.x, v.y)), fmaxf(v.z, v.w));
        S += (v.x + v.y) + (v.z + v.w);
    }
    mx = wave_max(mx);
    S = wave_sum(S);
    float se = 0.f;
    for (int c = lane * 4; c < V; c += 256) {
        float4 v = *(const float4*)(z + c);
        se += (__expf(v.x - mx) + __expf(v.y - mx)) + (__expf(v.z - mx) + __expf(v.w - mx));
    }
    const float lse = mx + __logf(wave_sum(se));
    if (lane == 0) {
        A.lse[row] = lse;
        float loss = 0.f;
        if (!r.zero_row) {
            const float eps = r.eps, conf = r.conf;
            const float zt = z[r.t], zp = z[A.pad];
            float n_eps, sum_tdz, sum_td, sum_tdlog;
            if (!r.t_is_pad) {
                n_eps = (float)(V - 2);
                sum_tdz = eps * (S - zt - zp) + conf * zt;
                sum_td = n_eps * eps + conf;
                sum_tdlog = (eps > 0.f ? n_eps * eps * __logf(eps) : 0.f) + (conf > 0.f ? conf * __logf(conf) : 0.f);
            } else {
                n_eps = (float)(V - 1);
                sum_tdz = eps * (S - zp);
                sum_td = n_eps * eps;
                sum_tdlog = eps > 0.f ? n_eps * eps * __logf(eps) : 0.f;
            }
            const float sw = r.weighted ? r.scale * r.w : r.scale;
            loss = (sum_tdlog - sum_tdz + lse * sum_td) * sw;
        }
        A.rowloss[row] = loss;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void wlosshead_bwd_kernel(const mtn_wlosshead_args A, int total_rows) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= total_rows) return;
    const WRow r = wrow_info(A, row, lane);
    const float* z = A.logits + (size_t)row * A.ldz;
    T* dz = (T*)A.dlogits + (size_t)row * A.ldd;
    const int V = A.V;
    float g = (*A.gloss) * r.scale;
    if (r.weighted) g = g * r.w;
    const float eps = r.eps, conf = r.conf;
    const float sum_td = r.zero_row ? 0.f : (r.t_is_pad ? (float)(V - 1) * eps : (float)(V - 2) * eps + conf);
    const float lse = A.lse[row];
    for (int c = lane * 4; c < A.ldd; c += 256) {
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c < V && !r.zero_row) {
            float4 v = *(const float4*)(z + c);
            float* ov = &o.x;
            const float* vv = &v.x;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int j = c + k;
                float td = eps;
                if (j == A.pad) td = 0.f;
                else if (j == r.t) td = conf;
                ov[k] = g * (__expf(vv[k] - lse) * sum_td - td);
            }
        }
        store_lp4<T>(dz + c, o);
    }
}

// everything mtn_losshead_fwd / _bwd refuse, then the weights and the smoothings
static int wlosshead_check(const char* fn, const mtn_wlosshead_args* A, bool bwd, int dtype, int* total) {
#define WL_CHECK(cond, msg) do { if (!(cond)) { mtn_set_error("%s: %s", fn, msg); return MTN_ERR_ARG; } } while (0)
    WL_CHECK(!bwd || dtype == MTN_F32 || dtype == MTN_BF16, "bad dtype");
    WL_CHECK(A && A->n_seg >= 1 && A->n_seg <= MTN_LOSSHEAD_MAX_SEG, "bad segment count");
    WL_CHECK(A->V >= 4 && A->V % 4 == 0 && A->ldz % 4 == 0 && A->ldz >= A->V, "V and ldz must be multiples of 4, ldz >= V >= 4");
    WL_CHECK(!bwd || (A->ldd % 4 == 0 && A->ldd >= A->V), "ldd must be a multiple of 4, ldd >= V");
    WL_CHECK(A->pad >= 0 && A->pad < A->V, "pad outside [0, V)");
    WL_CHECK(A->logits && A->lse && (bwd ? (A->gloss && A->dlogits) : A->rowloss != nullptr), "null buffer");
    *total = 0;
    for (int s = 0; s < A->n_seg; ++s) {
        WL_CHECK(A->rows[s] > 0 && A->target[s] && A->norm[s], "bad segment");
        WL_CHECK(((uintptr_t)A->roww[s] & 3) == 0, "row weights must be 4-byte aligned");
        WL_CHECK(!isnan(A->smoothing_seg[s]), "smoothing_seg is NaN");
        *total += A->rows[s];
    }
#undef WL_CHECK
    return MTN_OK;
}

extern "C" int mtn_wlosshead_fwd(const mtn_wlosshead_args* A, void* stream) {
    int total = 0;
    const int rc = wlosshead_check(__func__, A, false, 0, &total);
    if (rc != MTN_OK) return rc;
    hipLaunchKernelGGL(wlosshead_fwd_kernel, dim3((total + 3) / 4), dim3(256), 0, (hipStream_t)stream, *A, total);
    MTN_CHECK_LAUNCH();
    return MTN_OK;
}

extern "C" int mtn_wlosshead_bwd(int dtype, const mtn_wlosshead_args* A, void* stream) {
    int total = 0;
    const int rc = wlosshead_check(__func__, A, true, dtype, &total);
    if (rc != MTN_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (dtype == MTN_BF16) hipLaunchKernelGGL((wlosshead_bwd_kernel<bf16_t>), dim3((total + 3) / 4), dim3(256), 0, st, *A, total);
    else hipLaunchKernelGGL((wlosshead_bwd_kernel<float>), dim3((total + 3) / 4), dim3(256), 0, st, *A, total);
    MTN_CHECK_LAUNCH();
    return MTN_OK;
}

// ------------------------------------------------------------------------------------------ rewards against a fixed corpus
struct RowsArgs { EvalArgs e; const int* item; };

__global__ __launch_bounds__(256) void scst_table_clear_kernel(uint4* w, size_t n16) { ev_clear_body(w, n16); }
__global__ __launch_bounds__(EV_THREADS) void scst_table_df_kernel(const EvalArgs E) { ev_df_body(E); }
__global__ __launch_bounds__(EV_THREADS) void scst_score_rows_kernel(const RowsArgs X) {
    const int n = blockIdx.x;
    const int q = min(max(X.item[n], 0), X.e.a.Q - 1);      // device data: clamped, never an index outside the corpus
    ev_item_body(X.e, q, n);
}

// the corpus and its table as the EvalArgs the shared bodies read (Q = Qc); `rows`: the hypothesis side too
static int rows_check(const char* fn, const mtn_eval_rows_args* a, bool rows, EvalArgs* E) {
#define RW_CHECK(cond, msg) do { if (!(cond)) { mtn_set_error("%s: %s", fn, msg); return MTN_ERR_ARG; } } while (0)
    RW_CHECK(a, "null arguments");
    RW_CHECK(a->ref && a->ref_len && a->n_ref, "null corpus buffer");
    RW_CHECK(a->Qc >= 1 && a->R >= 1 && a->R <= EV_R && a->L >= 1 && a->L <= EV_L, "Qc >= 1, 1 <= R <= 8, 1 <= L <= 128");
    RW_CHECK(a->ldl >= a->L, "ldl >= L");
    RW_CHECK((unsigned long long)a->Qc * a->R * a->L <= EV_MAX_TOKENS, "Qc R L <= 2^28");
    const unsigned long long cap = ev_capacity(a->Qc, a->R, a->L);
    RW_CHECK(a->workspace && a->workspace_bytes >= (long)(cap * 8ull) && ((uintptr_t)a->workspace & 15u) == 0,
             "workspace: 16-byte aligned, at least mtn_eval_workspace_bytes(Qc, R, L)");
    if (rows) {
        RW_CHECK(a->N >= 1, "N >= 1");
        RW_CHECK(a->hyp && a->hyp_len && a->item, "null input buffer");
        RW_CHECK(a->stats && a->rouge && a->cider, "null output buffer");
    }
#undef RW_CHECK
    memset(E, 0, sizeof *E);
    E->a.Q = a->Qc; E->a.R = a->R; E->a.L = a->L; E->a.ldl = a->ldl;
    E->a.ref = a->ref; E->a.ref_len = a->ref_len; E->a.n_ref = a->n_ref;
    E->a.workspace = a->workspace; E->a.workspace_bytes = a->workspace_bytes;
    if (rows) {
        E->a.hyp = a->hyp; E->a.hyp_len = a->hyp_len;
        E->a.stats = a->stats; E->a.rouge = a->rouge; E->a.cider = a->cider;
    }
    E->key = (unsigned*)a->workspace;
    E->cnt = (int*)a->workspace + cap;
    E->mask = (unsigned)(cap - 1ull);
    return MTN_OK;
}

extern "C" int mtn_eval_table_build(const mtn_eval_rows_args* a, void* stream) {
    EvalArgs E;
    const int rc = rows_check(__func__, a, false, &E);
    if (rc != MTN_OK) return rc;
    const size_t n16 = (size_t)(((unsigned long long)E.mask + 1ull) * 8ull / 16ull);
    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(scst_table_clear_kernel, dim3((unsigned)((n16 + 255) / 256 < 4096 ? (n16 + 255) / 256 : 4096)), dim3(256), 0, st,
                       (uint4*)a->workspace, n16);
    MTN_CHECK_LAUNCH();
    hipLaunchKernelGGL(scst_table_df_kernel, dim3(a->Qc), dim3(EV_THREADS), 0, st, E);
    MTN_CHECK_LAUNCH();
    return MTN_OK;
}

extern "C" int mtn_eval_score_rows(const mtn_eval_rows_args* a, void* stream) {
    RowsArgs X;
    const int rc = rows_check(__func__, a, true, &X.e);
    if (rc != MTN_OK) return rc;
    X.item = a->item;
    hipLaunchKernelGGL(scst_score_rows_kernel, dim3(a->N), dim3(EV_THREADS), 0, (hipStream_t)stream, X);
    MTN_CHECK_LAUNCH();
    return MTN_OK;
}

// ------------------------------------------------------------------------------------------ sample log -> targets
__global__ __launch_bounds__(256) void scst_assemble_kernel(const mtn_scst_assemble_args A) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= A.rows) return;
    int first = A.L;                                         // the smallest l that holds <eos>
    for (int l = lane; l < A.L; l += 64)
        if (A.log_tok[(size_t)l * A.rows + row] == A.eos) first = min(first, l);
    for (int o = 32; o > 0; o >>= 1) first = min(first, __shfl_xor(first, o, 64));
    const int n = first < A.L ? first : A.L - 1;
    long* trg = A.trg + (size_t)row * A.T;
    long* trg_y = A.trg_y + (size_t)row * A.T;
    int* hyp = A.hyp + (size_t)row * (size_t)A.ldh;
    for (int t = lane; t < A.T; t += 64) {                   // n <= L - 1 <= T - 1: position n of both rows exists
        const long y = t < n ? (long)A.log_tok[(size_t)t * A.rows + row] : (long)A.pad;
        const long yb = (t >= 1 && t <= n) ? (long)A.log_tok[(size_t)(t - 1) * A.rows + row] : (long)A.pad;
        trg[t] = t == 0 ? (long)A.sos : yb;
        trg_y[t] = t == n ? (long)A.eos : y;
        if (t < A.L) hyp[t] = (int)y;
    }
    if (lane == 0) A.hyp_len[row] = n;
}

extern "C" int mtn_scst_assemble(const mtn_scst_assemble_args* a, void* stream) {
    MTN_CHECK_ARG(a, "null arguments");
    MTN_CHECK_ARG(a->log_tok && a->trg && a->trg_y && a->hyp && a->hyp_len, "null buffer");
    MTN_CHECK_ARG(a->rows >= 1 && a->L >= 1, "rows >= 1, L >= 1");
    MTN_CHECK_ARG(a->T >= a->L && a->ldh >= a->L, "T >= L, ldh >= L");
    hipLaunchKernelGGL(scst_assemble_kernel, dim3((a->rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, *a);
    MTN_CHECK_LAUNCH();
    return MTN_OK;
}

// ------------------------------------------------------------------------------------------ rewards -> row weights
static constexpr int ADV_MAX_D = 1024, ADV_MAX_S = 64;

__device__ __forceinline__ double adv_baseline(const mtn_scst_advantage_args& A, int d, int s) {
    if (A.baseline) return A.baseline[d];
    double sum = 0.0;
    for (int k = 0; k < A.S; ++k) if (k != s) sum += A.reward[(size_t)d * A.S + k];
    return sum / (double)(A.S - 1);
}

// block b < D S: the weights of sample b; the last block: the two means (a thread per dialogue, then one thread over the dialogues)
__global__ __launch_bounds__(256) void scst_advantage_kernel(const mtn_scst_advantage_args A) {
    __shared__ double s_r[ADV_MAX_D], s_b[ADV_MAX_D];
    const int n = A.D * A.S, b = blockIdx.x;
    if (b < n) {
        const int d = b / A.S, s = b - d * A.S;
        const double a = A.reward[b] - adv_baseline(A, d, s);
        const float w = (float)(-a);
        for (int t = threadIdx.x; t < A.T; t += 256) A.roww[(size_t)b * A.T + t] = w;
        if (threadIdx.x == 0 && A.adv) A.adv[b] = a;
        return;
    }
    for (int d = threadIdx.x; d < A.D; d += 256) {
        double sr = 0.0, sb = 0.0;
        for (int s = 0; s < A.S; ++s) {
            sr += A.reward[(size_t)d * A.S + s];
            sb += adv_baseline(A, d, s);
        }
        s_r[d] = sr;
        s_b[d] = sb;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double sr = 0.0, sb = 0.0;
        for (int d = 0; d < A.D; ++d) { sr += s_r[d]; sb += s_b[d]; }
        *A.mean_reward = sr / (double)n;
        *A.mean_baseline = sb / (double)n;
    }
}

extern "C" int mtn_scst_advantage(const mtn_scst_advantage_args* a, void* stream) {
    MTN_CHECK_ARG(a, "null arguments");
    MTN_CHECK_ARG(a->reward && a->roww && a->mean_reward && a->mean_baseline, "null buffer");
    MTN_CHECK_ARG(a->D >= 1 && a->D <= ADV_MAX_D && a->S >= 1 && a->S <= ADV_MAX_S && a->T >= 1, "1 <= D <= 1024, 1 <= S <= 64, T >= 1");
    MTN_CHECK_ARG(a->baseline || a->S >= 2, "the leave-one-out baseline needs S >= 2");
    hipLaunchKernelGGL(scst_advantage_kernel, dim3(a->D * a->S + 1), dim3(256), 0, (hipStream_t)stream, *a);
    MTN_CHECK_LAUNCH();
    return MTN_OK;
}
