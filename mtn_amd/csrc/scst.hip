// scst.hip — what self-critical sequence training (Rennie et al. 2017; the leave-one-out baseline of Luo 2020) needs on the device between
// the sampling search (sample.hip) and the optimiser: include/mtn_hip.h states every formula.
//   mtn_scst_assemble         the sample log -> teacher-forcing targets and the int32 rows the reward launch reads (a wave per row)
//   mtn_eval_table_build      the document-frequency table of a fixed reference corpus, once (eval_common.h's clear and table bodies)
//   mtn_eval_score_rows       N hypotheses, each against the references of the corpus item it names (eval_common.h's item body: the
//                             launch reads the table and never writes it, no atomics, double with fixed-order sums)
//   mtn_scst_advantage        rewards -> signed row weights -(r - b), b a given baseline or the leave-one-out mean
// The loss head that reads those weights (mtn_wlosshead_fwd / _bwd) is an instantiation of losshead.hip.
#include "eval_common.h"

#include <math.h>

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
