// average.hip — averaging in weight space over fp32 buffers: the running mean of checkpoints (mtn_lerp_f32), the exponential moving
// average the optimiser keeps inside the step (mtn_ema_step) and the exchange that puts the average under the model (mtn_swap_f32).
// HBM-bound streaming passes: 16-byte vector accesses, grid-stride over a capped grid, a scalar tail for n % 4.
#include <math.h>

#include "common.h"

// acc + c * (x - acc) is THREE separately rounded fp32 operations (subtract, multiply, add): numpy float32 reproduces it bit for bit,
// and so does every kernel here.  No contraction into an fma anywhere in this file.
#pragma clang fp contract(off)

static inline int avg_grid_for(long n_vec) {
    long b = (n_vec + 255) / 256;
    if (b > 2048) b = 2048;  // 256 CUs x 8 blocks, grid-stride the rest
    if (b < 1) b = 1;
    return (int)b;
}

__device__ __forceinline__ float lerp1(float a, float x, float c) {
    const float d = x - a;
    const float s = c * d;
    return a + s;
}

// c = max(1 - decay, 9 / (10 + t)), t = the step number after the tick (state[0])
__device__ __forceinline__ float ema_coef(const float* state, float decay) {
    const float t = state[0];
    return fmaxf(1.0f - decay, 9.0f / (10.0f + t));
}

// FROM_STATE: the coefficient comes from the optimiser state (every thread computes it: no second launch); otherwise it is `coef`.
template <bool FROM_STATE>
__global__ __launch_bounds__(256) void lerp_kernel(long n, float* __restrict__ acc, const float* __restrict__ x, const float* __restrict__ state,
                                                   float coef, float* __restrict__ coef_out) {
    const float c = FROM_STATE ? ema_coef(state, coef) : coef;
    if (FROM_STATE && coef_out && blockIdx.x == 0 && threadIdx.x == 0) *coef_out = c;
    const long n4 = n >> 2;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        float4 a = *(const float4*)(acc + i * 4);
        const float4 v = *(const float4*)(x + i * 4);
        a.x = lerp1(a.x, v.x, c); a.y = lerp1(a.y, v.y, c); a.z = lerp1(a.z, v.z, c); a.w = lerp1(a.w, v.w, c);
        *(float4*)(acc + i * 4) = a;
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {  // tail
        const long i = (n4 << 2) + threadIdx.x;
        acc[i] = lerp1(acc[i], x[i], c);
    }
}

__global__ __launch_bounds__(256) void swap_kernel(long n, float* __restrict__ a, float* __restrict__ b) {
    const long n4 = n >> 2;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        const float4 u = *(const float4*)(a + i * 4);
        const float4 v = *(const float4*)(b + i * 4);
        *(float4*)(a + i * 4) = v;
        *(float4*)(b + i * 4) = u;
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {  // tail
        const long i = (n4 << 2) + threadIdx.x;
        const float u = a[i];
        a[i] = b[i];
        b[i] = u;
    }
}

static inline bool aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

extern "C" int mtn_lerp_f32(long n, float* acc, const float* x, float coef, void* stream) {
    MTN_CHECK_ARG(n >= 0, "n must not be negative");
    MTN_CHECK_ARG(acc && x && aligned16(acc) && aligned16(x), "acc and x must be non-null and 16-byte aligned");
    MTN_CHECK_ARG(acc != x, "acc and x must be different buffers");
    MTN_CHECK_ARG(isfinite(coef) && coef >= 0.0f && coef <= 1.0f, "coef must be in [0, 1]");
    if (n == 0) return MTN_OK;
    hipLaunchKernelGGL((lerp_kernel<false>), dim3(avg_grid_for(n >> 2)), dim3(256), 0, (hipStream_t)stream, n, acc, x, (const float*)nullptr, coef,
                       (float*)nullptr);
    MTN_CHECK_LAUNCH();
    return MTN_OK;
}

extern "C" int mtn_ema_step(long n, float* ema, const float* p, const float* state, float decay, float* coef_out, void* stream) {
    MTN_CHECK_ARG(n >= 0, "n must not be negative");
    MTN_CHECK_ARG(ema && p && aligned16(ema) && aligned16(p), "ema and p must be non-null and 16-byte aligned");
    MTN_CHECK_ARG(ema != p, "ema and p must be different buffers");
    MTN_CHECK_ARG(state && (((uintptr_t)state) & 3) == 0 && (((uintptr_t)coef_out) & 3) == 0, "state must be non-null; state and coef_out 4-byte aligned");
    MTN_CHECK_ARG(isfinite(decay) && decay >= 0.0f && decay < 1.0f, "decay must be in [0, 1)");
    if (n == 0) return MTN_OK;
    hipLaunchKernelGGL((lerp_kernel<true>), dim3(avg_grid_for(n >> 2)), dim3(256), 0, (hipStream_t)stream, n, ema, p, state, decay, coef_out);
    MTN_CHECK_LAUNCH();
    return MTN_OK;
}

extern "C" int mtn_swap_f32(long n, float* a, float* b, void* stream) {
    MTN_CHECK_ARG(n >= 0, "n must not be negative");
    MTN_CHECK_ARG(a && b && aligned16(a) && aligned16(b), "a and b must be non-null and 16-byte aligned");
    MTN_CHECK_ARG(a != b, "a and b must be different buffers");
    if (n == 0) return MTN_OK;
    hipLaunchKernelGGL(swap_kernel, dim3(avg_grid_for(n >> 2)), dim3(256), 0, (hipStream_t)stream, n, a, b);
    MTN_CHECK_LAUNCH();
    return MTN_OK;
}
