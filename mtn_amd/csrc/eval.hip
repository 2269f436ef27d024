// eval.hip — corpus metrics of generated responses on the device: BLEU-1..4, ROUGE-L and CIDEr (the clipped, length-penalised form) of Q
// items, each one hypothesis against up to 8 references of at most 128 tokens.  include/mtn_hip.h mtn_eval_metrics holds the definition
// (tests/eval_refs.py is its Python form).  The reference scores with coco-caption on the host (utils/evaluate.py); nothing of that runs here.
// Four launches on the caller's stream, no grid barrier, no workgroup ever waits for another:
//   1  eval_clear_kernel   zeroes the workspace (the table's keys and counts).
//   2  eval_df_kernel      the document-frequency table, one workgroup per item (csrc/eval_common.h: open addressing, one
//                          compare-and-swap per claimed slot, integer atomic counts — exact in any arrival order).
//   3  eval_item_kernel    one workgroup per item, all its tokens in LDS: table lookups, sliding-window n-gram counts, clipped matches,
//                          the bit-parallel LCS, then the item's ten integers, ROUGE-L and CIDEr (csrc/eval_common.h, phases 1-4).
//   4  eval_reduce_kernel  one workgroup: int64 sums of the BLEU statistics, means of the doubles, the eight corpus values.
// All floating point is double.  A sum across lanes is a fixed butterfly inside a wave, then the waves' partials in ascending order in one
// thread: two launches give the same bytes.  Tokens are compared and hashed, never used as indices.  Every store is a vector store.
#include "common.h"
#include "eval_common.h"

// the bodies are eval_common.h's (csrc/scst.hip scores sampled rows against a fixed corpus with the same ones)
__global__ __launch_bounds__(256) void eval_clear_kernel(uint4* w, size_t n16) { ev_clear_body(w, n16); }
__global__ __launch_bounds__(EV_THREADS) void eval_df_kernel(const EvalArgs E) { ev_df_body(E); }
__global__ __launch_bounds__(EV_THREADS) void eval_item_kernel(const EvalArgs E) { ev_item_body(E, blockIdx.x, blockIdx.x); }

__global__ __launch_bounds__(EV_RED) void eval_reduce_kernel(const EvalArgs E) {
    const mtn_eval_args& A = E.a;
    __shared__ long long s_i[EV_RED / 64][10];
    __shared__ double s_d[EV_RED / 64][2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    long long si[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    double sd[2] = {0.0, 0.0};
    for (int q = tid; q < A.Q; q += EV_RED) {                // a thread's items in ascending order
        for (int k = 0; k < 10; ++k) si[k] += A.stats[(size_t)q * 10 + k];
        sd[0] += A.rouge[q];
        sd[1] += A.cider[q];
    }
    for (int k = 0; k < 10; ++k) {
        const long long v = ev_wave_sum(si[k]);
        if (lane == 0) s_i[wave][k] = v;
    }
    for (int k = 0; k < 2; ++k) {
        const double v = ev_wave_sum(sd[k]);
        if (lane == 0) s_d[wave][k] = v;
    }
    __syncthreads();
    if (tid != 0) return;
    long long t[10];
    for (int k = 0; k < 10; ++k) { t[k] = 0; for (int w = 0; w < EV_RED / 64; ++w) t[k] += s_i[w][k]; }
    double rl = 0.0, cd = 0.0;
    for (int w = 0; w < EV_RED / 64; ++w) { rl += s_d[w][0]; cd += s_d[w][1]; }
    const double T = (double)t[8], C = (double)t[9];
    const double ratio = (T + 1e-15) / (C + 1e-9);
    const double bp = ratio < 1.0 ? exp(1.0 - 1.0 / ratio) : 1.0;
    double p = 1.0;
    for (int n = 1; n <= 4; ++n) {
        p = p * (((double)t[3 + n] + 1e-15) / ((double)t[n - 1] + 1e-9));
        const double b = pow(p, 1.0 / (double)n);
        A.corpus[n - 1] = ratio < 1.0 ? b * bp : b;
    }
    A.corpus[4] = rl / (double)A.Q;
    A.corpus[5] = cd / (double)A.Q;
    A.corpus[6] = T;
    A.corpus[7] = C;
}

extern "C" long mtn_eval_workspace_bytes(int Q, int R, int L) {
    if (Q < 1 || R < 1 || R > EV_R || L < 1 || L > EV_L || (unsigned long long)Q * R * L > EV_MAX_TOKENS) return 0;
    return (long)(ev_capacity(Q, R, L) * 8ull);
}

extern "C" int mtn_eval_metrics(const mtn_eval_args* a, void* stream) {
    MTN_CHECK_ARG(a, "null arguments");
    MTN_CHECK_ARG(a->hyp && a->hyp_len && a->ref && a->ref_len && a->n_ref, "null input buffer");
    MTN_CHECK_ARG(a->stats && a->rouge && a->cider && a->corpus, "null output buffer");
    MTN_CHECK_ARG(a->Q >= 1 && a->R >= 1 && a->R <= EV_R && a->L >= 1 && a->L <= EV_L, "Q >= 1, 1 <= R <= 8, 1 <= L <= 128");
    MTN_CHECK_ARG(a->ldl >= a->L, "ldl >= L");
    MTN_CHECK_ARG((unsigned long long)a->Q * a->R * a->L <= EV_MAX_TOKENS, "Q R L <= 2^28");
    const unsigned long long cap = ev_capacity(a->Q, a->R, a->L);
    MTN_CHECK_ARG(a->workspace && a->workspace_bytes >= (long)(cap * 8ull) && ((uintptr_t)a->workspace & 15u) == 0,
                  "workspace: 16-byte aligned, at least mtn_eval_workspace_bytes(Q, R, L)");
    EvalArgs E;
    E.a = *a;
    E.key = (unsigned*)a->workspace;
    E.cnt = (int*)a->workspace + cap;
    E.mask = (unsigned)(cap - 1ull);
    const size_t n16 = (size_t)(cap * 8ull / 16ull);
    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(eval_clear_kernel, dim3((unsigned)((n16 + 255) / 256 < 4096 ? (n16 + 255) / 256 : 4096)), dim3(256), 0, st, (uint4*)a->workspace, n16);
    MTN_CHECK_LAUNCH();
    hipLaunchKernelGGL(eval_df_kernel, dim3(a->Q), dim3(EV_THREADS), 0, st, E);
    MTN_CHECK_LAUNCH();
    hipLaunchKernelGGL(eval_item_kernel, dim3(a->Q), dim3(EV_THREADS), 0, st, E);
    MTN_CHECK_LAUNCH();
    hipLaunchKernelGGL(eval_reduce_kernel, dim3(1), dim3(EV_RED), 0, st, E);
    MTN_CHECK_LAUNCH();
    return MTN_OK;
}
