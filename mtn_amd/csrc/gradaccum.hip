// gradaccum.hip — gradient accumulation over a window of micro-batches: acc collects w_k * g_k, the closing pass writes the window's
// gradient (sum_k w_k g_k) / (sum_k w_k) over g in place and, when asked, the partials mtn_grad_sumsq would compute from it
// (mtn_grad_accum).  One HBM-bound streaming pass shaped like average.hip's and gradnorm.hip's: 16-byte accesses, grid-stride over
// gradnorm's capped grid (a pure function of n), a scalar tail for n % 4 in workgroup 0.  No atomics, nothing allocated, no host read.
#include "gradnorm_common.h"

// w * g, acc + (w * g) and (...) * inv are separately rounded fp32 operations: numpy float32 reproduces the bytes.  No contraction
// into an fma anywhere in this file (gn_sq's double chain is rounded once either way).
#pragma clang fp contract(off)

template <int MODE>
__device__ __forceinline__ float accum1(float a, float x, float w, float inv) {
    const float p = w * x;
    if (MODE == MTN_ACCUM_FIRST) return p;
    const float s = a + p;
    if (MODE == MTN_ACCUM_ADD) return s;
    return s * inv;
}

// FIRST / ADD write acc and only read g; LAST writes g and only reads acc.  SUMSQ (LAST only): every thread also keeps
// grad_sumsq_kernel's chain over the values it writes, in that kernel's order, and the workgroup writes that kernel's partial.
template <int MODE, bool SUMSQ>
__global__ __launch_bounds__(GN_THREADS) void grad_accum_kernel(long n, float* __restrict__ acc, float* __restrict__ g, const float* w_p,
                                                                const float* total_in, float* total_out,
                                                                double* __restrict__ partial) {  // acc != g (checked)
    __shared__ double lds[GN_THREADS / 64];
    const float w = *w_p;
    const float t = MODE == MTN_ACCUM_FIRST ? w : *total_in + w;
    const float inv = MODE == MTN_ACCUM_LAST ? (float)(1.0 / (double)t) : 0.0f;  // every thread computes it: no second launch
    const long n4 = n >> 2;
    double sq = 0.0;
#pragma unroll 4
    for (long i = (long)blockIdx.x * GN_THREADS + threadIdx.x; i < n4; i += (long)gridDim.x * GN_THREADS) {
        float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (MODE != MTN_ACCUM_FIRST) a = *(const float4*)(acc + i * 4);
        const float4 v = *(const float4*)(g + i * 4);
        a.x = accum1<MODE>(a.x, v.x, w, inv); a.y = accum1<MODE>(a.y, v.y, w, inv);
        a.z = accum1<MODE>(a.z, v.z, w, inv); a.w = accum1<MODE>(a.w, v.w, w, inv);
        *(float4*)((MODE == MTN_ACCUM_LAST ? g : acc) + i * 4) = a;
        if (SUMSQ) sq = gn_sq(gn_sq(gn_sq(gn_sq(sq, a.x), a.y), a.z), a.w);
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {  // tail
        const long i = (n4 << 2) + threadIdx.x;
        const float r = accum1<MODE>(MODE == MTN_ACCUM_FIRST ? 0.0f : acc[i], g[i], w, inv);
        (MODE == MTN_ACCUM_LAST ? g : acc)[i] = r;
        if (SUMSQ) sq = gn_sq(sq, r);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *total_out = t;  // one thread, a plain store; total_in is another float (checked)
    if (SUMSQ) {
        const double s = gn_block_sum(sq, lds);
        if (threadIdx.x == 0) partial[blockIdx.x] = s;
    }
}

extern "C" int mtn_grad_accum(int mode, long n, float* acc, float* g, const float* w, const float* total_in, float* total_out,
                              double* partial, void* stream) {
    MTN_CHECK_ARG(mode == MTN_ACCUM_FIRST || mode == MTN_ACCUM_ADD || mode == MTN_ACCUM_LAST, "mode is MTN_ACCUM_FIRST, _ADD or _LAST");
    MTN_CHECK_ARG(n >= 0, "n must not be negative");
    MTN_CHECK_ARG(acc && g && gn_aligned(acc, 16) && gn_aligned(g, 16), "acc and g must be non-null and 16-byte aligned");
    MTN_CHECK_ARG(acc != g, "acc and g must be different buffers");
    MTN_CHECK_ARG(w && gn_aligned(w, 4), "w must be non-null and 4-byte aligned");
    MTN_CHECK_ARG(total_out && gn_aligned(total_out, 4) && gn_aligned(total_in, 4), "total_out must be non-null; the totals 4-byte aligned");
    MTN_CHECK_ARG(mode == MTN_ACCUM_FIRST || total_in, "total_in must be non-null outside MTN_ACCUM_FIRST");
    MTN_CHECK_ARG(total_in != total_out && w != total_out, "total_out must be a float of its own (all threads read total_in and w)");
    MTN_CHECK_ARG(gn_aligned(partial, 8), "partial must be 8-byte aligned");
    MTN_CHECK_ARG(mode == MTN_ACCUM_LAST || !partial, "partial must be null outside MTN_ACCUM_LAST");
    if (n == 0) return MTN_OK;
    const dim3 grid(gn_grid_for(n)), block(GN_THREADS);
    hipStream_t st = (hipStream_t)stream;
    if (mode == MTN_ACCUM_FIRST)
        hipLaunchKernelGGL((grad_accum_kernel<MTN_ACCUM_FIRST, false>), grid, block, 0, st, n, acc, g, w, total_in, total_out, partial);
    else if (mode == MTN_ACCUM_ADD)
        hipLaunchKernelGGL((grad_accum_kernel<MTN_ACCUM_ADD, false>), grid, block, 0, st, n, acc, g, w, total_in, total_out, partial);
    else if (partial)
        hipLaunchKernelGGL((grad_accum_kernel<MTN_ACCUM_LAST, true>), grid, block, 0, st, n, acc, g, w, total_in, total_out, partial);
    else
        hipLaunchKernelGGL((grad_accum_kernel<MTN_ACCUM_LAST, false>), grid, block, 0, st, n, acc, g, w, total_in, total_out, partial);
    MTN_CHECK_LAUNCH();
    return MTN_OK;
}
