// gradnorm.hip — gradient clipping by global norm: the sum of squares of an fp32 buffer in double (mtn_grad_sumsq, one partial per
// workgroup) and the one-workgroup pass that turns the partials into the norm and the clip coefficient Adam reads as its grad_scale
// (mtn_clip_scale).  The first is an HBM-bound streaming pass shaped like average.hip's: 16-byte loads, grid-stride over a capped grid
// that is a pure function of n, a scalar tail for n % 4.  No atomics anywhere: every sum is taken in an order fixed by n alone, so two
// launches over the same bytes give the same bytes, on any device.
#include <math.h>

#include "gradnorm_common.h"  // the grid, the chain step and the reduction tree, shared with gradaccum.hip

__global__ __launch_bounds__(GN_THREADS) void grad_sumsq_kernel(long n, const float* __restrict__ g, double* __restrict__ partial) {
    __shared__ double lds[GN_THREADS / 64];
    const long n4 = n >> 2;
    double acc = 0.0;
#pragma unroll 4  // four loads in flight per thread; the additions keep their order (one chain)
    for (long i = (long)blockIdx.x * GN_THREADS + threadIdx.x; i < n4; i += (long)gridDim.x * GN_THREADS) {
        const float4 v = *(const float4*)(g + i * 4);
        acc = gn_sq(gn_sq(gn_sq(gn_sq(acc, v.x), v.y), v.z), v.w);
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) acc = gn_sq(acc, g[(n4 << 2) + threadIdx.x]);  // tail
    const double t = gn_block_sum(acc, lds);
    if (threadIdx.x == 0) partial[blockIdx.x] = t;
}

__global__ __launch_bounds__(GN_THREADS) void clip_scale_kernel(int n_partial, const double* __restrict__ partial, float max_norm,
                                                                const float* base_scale, float* scale_out, double* norm_out, double* stats) {
    __shared__ double lds[GN_THREADS / 64];
    double acc = 0.0;
    for (int i = threadIdx.x; i < n_partial; i += GN_THREADS) acc += partial[i];
    const double sum = gn_block_sum(acc, lds);
    if (threadIdx.x != 0) return;
    const float base = base_scale ? *base_scale : 1.0f;  // read before scale_out is written: they may be one float
    const double norm = sqrt(sum) * fabs((double)base);
    const bool finite = isfinite(norm);
    const double coef = finite ? fmin(1.0, (double)max_norm / (norm + 1e-6)) : (double)NAN;
    *scale_out = coef == 1.0 ? base : (float)((double)base * coef);  // not clipping: the base's own bits
    if (norm_out) *norm_out = norm;
    if (stats) {  // one thread, plain loads and stores: stream order keeps calls apart
        if (finite) {
            stats[0] += norm;
            stats[1] = fmax(stats[1], norm);
        }
        stats[2] += 1.0;
        if (coef < 1.0) stats[3] += 1.0;
        if (!finite) stats[4] += 1.0;
    }
}

extern "C" int mtn_grad_sumsq_partials(long n) { return n <= 0 ? 0 : gn_grid_for(n); }

extern "C" int mtn_grad_sumsq(long n, const float* g, double* partial, void* stream) {
    MTN_CHECK_ARG(n > 0, "n must be positive");
    MTN_CHECK_ARG(g && gn_aligned(g, 16), "g must be non-null and 16-byte aligned");
    MTN_CHECK_ARG(partial && gn_aligned(partial, 8), "partial must be non-null and 8-byte aligned");
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3(gn_grid_for(n)), dim3(GN_THREADS), 0, (hipStream_t)stream, n, g, partial);
    MTN_CHECK_LAUNCH();
    return MTN_OK;
}

extern "C" int mtn_clip_scale(int n_partial, const double* partial, float max_norm, const float* base_scale, float* scale_out,
                              double* norm_out, double* stats, void* stream) {
    MTN_CHECK_ARG(n_partial >= 1 && n_partial <= GN_MAX_PARTIALS, "n_partial must lie in 1..2048 (mtn_grad_sumsq_partials)");
    MTN_CHECK_ARG(partial && gn_aligned(partial, 8), "partial must be non-null and 8-byte aligned");
    MTN_CHECK_ARG(max_norm > 0.0f, "max_norm must be > 0 (+inf measures without clipping) and not NaN");
    MTN_CHECK_ARG(gn_aligned(base_scale, 4), "base_scale must be 4-byte aligned");
    MTN_CHECK_ARG(scale_out && gn_aligned(scale_out, 4), "scale_out must be non-null and 4-byte aligned");
    MTN_CHECK_ARG(gn_aligned(norm_out, 8) && gn_aligned(stats, 8), "norm_out and stats must be 8-byte aligned");
    hipLaunchKernelGGL(clip_scale_kernel, dim3(1), dim3(GN_THREADS), 0, (hipStream_t)stream, n_partial, partial, max_norm, base_scale,
                       scale_out, norm_out, stats);
    MTN_CHECK_LAUNCH();
    return MTN_OK;
}
