// ensemble.hip — ensemble decoding on the device: M <= 8 rows of logits (or log-probabilities), one per checkpoint, become ONE row of
// log-probabilities that everything behind it (constrain.hip, select.hip topk_rows, sample.hip, score.hip) reads as it reads a single
// model's row — so an ensemble search stays one captured graph.  Definitions (include/mtn_hip.h restates them; tests/ensemble_refs.py is
// their float64 form), with x_m the row of member m, w_m >= 0 its weight (sum 1) and lse_m = logsumexp_c x_m[c]:
//   prob     out[c] = log sum_m w_m exp(x_m[c] - lse_m)          arithmetic mean of the probabilities; a_m = log w_m + x_m[c] - lse_m,
//            (mode 0) evaluated as max_m a_m + log sum_m exp(a_m - max): already normalised, no second pass
//   logprob  s[c] = sum_{m: w_m > 0} w_m (x_m[c] - lse_m),  out[c] = s[c] - logsumexp_c s[c]      weighted geometric mean, renormalised
//            (mode 1)
//   w_m = 0  the member is dropped on the host before the launch: it contributes nothing, whatever its entries (no 0 * inf)
//   -inf     prob: the entry contributes 0, a column that is -inf in every weighted member is -inf; logprob: -inf in any weighted
//            member gives -inf.  Every weighted member row must hold a finite entry (not checked).
// Every member row is normalised HERE (lse_m), so the generator's logits come in as they are: no mtn_log_softmax_rows launch per member.
// One workgroup per row.  Pass 1: per member a running (max, sum-exp) per thread, lanes combined by wave shuffles, the four waves
// through LDS in wave order — one barrier for all members.  Pass 2: every thread combines the columns it owns.  logprob: the same
// reduction once more over s (which the thread wrote to `out` and reads back itself), then the subtraction.  Fixed column -> thread map,
// fixed combination order, no atomics: two launches give the same bits.  16-byte loads and stores when every member's row and the out row
// are 16-byte aligned (columns past the last whole float4 one by one), otherwise the whole row one column at a time: any V / ld works.
#include "common.h"

#include <math.h>

static constexpr int ENS_THREADS = 256;
static constexpr int ENS_WAVES = ENS_THREADS / 64;
static constexpr int ENS_MAX_M = 8;

struct EnsArgs {                                              // the weighted members only, with log w
    int rows, V, M, mode;
    const float* x[ENS_MAX_M]; long ld[ENS_MAX_M];
    float w[ENS_MAX_M], logw[ENS_MAX_M];
    float* out; long ldo;
};

// a thread's (max, sum-exp) -> its wave's, left in LDS by lane 0
__device__ __forceinline__ void ens_wave_put(float m, float s, float (*red)[ENS_WAVES], int lane, int wave) {
    online_wave(m, s);
    if (lane == 0) { red[0][wave] = m; red[1][wave] = s; }
}
// ... and, after a barrier, the row's logsumexp from the waves' pairs in wave order (every thread computes the same bits)
__device__ __forceinline__ float ens_row_lse(const float (*red)[ENS_WAVES]) {
    float Mx = red[0][0];
#pragma unroll
    for (int w = 1; w < ENS_WAVES; ++w) Mx = fmaxf(Mx, red[0][w]);
    float S = 0.f;
#pragma unroll
    for (int w = 0; w < ENS_WAVES; ++w) S += red[0][w] > -INFINITY ? red[1][w] * __expf(red[0][w] - Mx) : 0.f;
    return Mx + logf(S);
}

// one column: prob -> its final value, logprob -> s[c]
__device__ __forceinline__ float ens_combine(const EnsArgs& A, const float (&v)[ENS_MAX_M], const float (&lse)[ENS_MAX_M]) {
    if (A.mode == 0) {
        float a[ENS_MAX_M], mx = -INFINITY;
#pragma unroll
        for (int m = 0; m < ENS_MAX_M; ++m)
            if (m < A.M) { a[m] = (v[m] - lse[m]) + A.logw[m]; mx = fmaxf(mx, a[m]); }
        if (!(mx > -INFINITY)) return -INFINITY;
        float acc = 0.f;
#pragma unroll
        for (int m = 0; m < ENS_MAX_M; ++m)
            if (m < A.M) acc += __expf(a[m] - mx);
        return mx + logf(acc);
    }
    float s = 0.f;
#pragma unroll
    for (int m = 0; m < ENS_MAX_M; ++m)
        if (m < A.M) s += A.w[m] * (v[m] - lse[m]);
    return s;
}

__global__ __launch_bounds__(ENS_THREADS) void ensemble_rows_kernel(const EnsArgs A) {
    __shared__ float s_red[ENS_MAX_M + 1][2][ENS_WAVES];
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, V = A.V, M = A.M;
    float* orow = A.out + (size_t)row * A.ldo;
    uintptr_t bits = (uintptr_t)orow;
#pragma unroll
    for (int m = 0; m < ENS_MAX_M; ++m)
        if (m < M) bits |= (uintptr_t)(A.x[m] + (size_t)row * A.ld[m]);
    const int V4 = (bits & 15) == 0 ? V / 4 : 0;              // whole float4s of the row; columns 4 * V4 .. V-1 go one by one

    // ---- pass 1: lse_m of every member row
#pragma unroll
    for (int m = 0; m < ENS_MAX_M; ++m) {
        if (m < M) {
            const float* x = A.x[m] + (size_t)row * A.ld[m];
            float mx = -INFINITY, s = 0.f;
            for (int i = tid; i < V4; i += ENS_THREADS) online4(mx, s, ((const float4*)x)[i]);
            for (int c = V4 * 4 + tid; c < V; c += ENS_THREADS) online1(mx, s, x[c]);
            ens_wave_put(mx, s, s_red[m], lane, wave);
        }
    }
    __syncthreads();
    float lse[ENS_MAX_M];
#pragma unroll
    for (int m = 0; m < ENS_MAX_M; ++m) lse[m] = m < M ? ens_row_lse(s_red[m]) : 0.f;

    // ---- pass 2: the columns this thread owns (the same ones in both halves of logprob)
    float smx = -INFINITY, ssum = 0.f;                        // (logprob: running logsumexp of s)
    for (int i = tid; i < V4; i += ENS_THREADS) {
        float4 xv[ENS_MAX_M];
#pragma unroll
        for (int m = 0; m < ENS_MAX_M; ++m)
            if (m < M) xv[m] = ((const float4*)(A.x[m] + (size_t)row * A.ld[m]))[i];
        float v[ENS_MAX_M];
        float4 o;
#pragma unroll
        for (int m = 0; m < ENS_MAX_M; ++m) v[m] = m < M ? xv[m].x : 0.f;
        o.x = ens_combine(A, v, lse);
#pragma unroll
        for (int m = 0; m < ENS_MAX_M; ++m) v[m] = m < M ? xv[m].y : 0.f;
        o.y = ens_combine(A, v, lse);
#pragma unroll
        for (int m = 0; m < ENS_MAX_M; ++m) v[m] = m < M ? xv[m].z : 0.f;
        o.z = ens_combine(A, v, lse);
#pragma unroll
        for (int m = 0; m < ENS_MAX_M; ++m) v[m] = m < M ? xv[m].w : 0.f;
        o.w = ens_combine(A, v, lse);
        ((float4*)orow)[i] = o;
        if (A.mode == 1) online4(smx, ssum, o);
    }
    for (int c = V4 * 4 + tid; c < V; c += ENS_THREADS) {
        float v[ENS_MAX_M];
#pragma unroll
        for (int m = 0; m < ENS_MAX_M; ++m) v[m] = m < M ? A.x[m][(size_t)row * A.ld[m] + c] : 0.f;
        const float o = ens_combine(A, v, lse);
        orow[c] = o;
        if (A.mode == 1) online1(smx, ssum, o);
    }
    if (A.mode == 0) return;                                  // (uniform: a kernel argument)

    ens_wave_put(smx, ssum, s_red[ENS_MAX_M], lane, wave);
    __syncthreads();
    const float Ls = ens_row_lse(s_red[ENS_MAX_M]);
    auto norm = [&](float s) { return s > -INFINITY ? s - Ls : -INFINITY; };
    for (int i = tid; i < V4; i += ENS_THREADS) {             // (a thread reads back what it wrote itself)
        float4 o = ((float4*)orow)[i];
        o.x = norm(o.x); o.y = norm(o.y); o.z = norm(o.z); o.w = norm(o.w);
        ((float4*)orow)[i] = o;
    }
    for (int c = V4 * 4 + tid; c < V; c += ENS_THREADS) orow[c] = norm(orow[c]);
}

extern "C" int mtn_ensemble_rows(const mtn_ensemble_args* a, void* stream) {
    MTN_CHECK_ARG(a && a->out, "null buffer");
    MTN_CHECK_ARG(a->M >= 1 && a->M <= ENS_MAX_M, "1 <= M <= 8");
    MTN_CHECK_ARG(a->rows > 0 && a->V > 0 && a->V < (1 << 24) && a->ldo >= a->V, "bad row matrix (rows, V >= 1, V < 2^24, ldo >= V)");
    MTN_CHECK_ARG(a->mode == 0 || a->mode == 1, "mode is 0 (prob) or 1 (logprob)");
    EnsArgs E;
    memset(&E, 0, sizeof(E));
    E.rows = a->rows; E.V = a->V; E.mode = a->mode; E.out = a->out; E.ldo = a->ldo;
    for (int m = 0; m < a->M; ++m) {
        MTN_CHECK_ARG(a->x[m], "null member");
        MTN_CHECK_ARG(a->ld[m] >= a->V, "ld >= V");
        MTN_CHECK_ARG(isfinite(a->w[m]) && a->w[m] >= 0.f, "weights are finite and >= 0");
        if (a->w[m] == 0.f) continue;                         // contributes nothing: never read
        E.x[E.M] = a->x[m]; E.ld[E.M] = a->ld[m]; E.w[E.M] = a->w[m]; E.logw[E.M] = (float)log((double)a->w[m]);
        ++E.M;
    }
    MTN_CHECK_ARG(E.M >= 1, "every weight is 0");
    hipLaunchKernelGGL(ensemble_rows_kernel, dim3(a->rows), dim3(ENS_THREADS), 0, (hipStream_t)stream, E);
    MTN_CHECK_LAUNCH();
    return MTN_OK;
}
