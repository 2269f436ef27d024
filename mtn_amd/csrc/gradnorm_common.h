// gradnorm_common.h — what gradnorm.hip's sum of squares and gradaccum.hip's closing pass share: the capped grid (a pure function of n),
// one thread's chain step and the workgroup's reduction tree.  A kernel that walks the 16-byte vectors j = b * 256 + t, j + 256 G, ...
// with gn_sq in x, y, z, w order, adds workgroup 0's tail and reduces with gn_block_sum writes mtn_grad_sumsq's partials, bit for bit.
#pragma once

#include "common.h"

#define GN_THREADS 256
#define GN_MAX_PARTIALS 2048  // 256 CUs x 8 blocks, as average.hip's avg_grid_for

static inline int gn_grid_for(long n) {
    long b = ((n >> 2) + GN_THREADS - 1) / GN_THREADS;
    if (b > GN_MAX_PARTIALS) b = GN_MAX_PARTIALS;
    if (b < 1) b = 1;
    return (int)b;
}

static inline bool gn_aligned(const void* p, uintptr_t a) { return (((uintptr_t)p) & (a - 1)) == 0; }

__device__ __forceinline__ double gn_sq(double acc, float x) {
    const double d = (double)x;  // the product of two floats is exact in double: acc + d * d is rounded once, fused or not
    return acc + d * d;
}

// The workgroup's total in thread 0, in a fixed order: xor butterfly inside each wave (every lane adds the same pairs), then the
// waves' totals from LDS, wave 0 first.
__device__ __forceinline__ double gn_block_sum(double v, double* lds) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = 0.0;
    if (threadIdx.x == 0) {
        t = lds[0];
#pragma unroll
        for (int w = 1; w < GN_THREADS / 64; ++w) t += lds[w];
    }
    return t;
}
