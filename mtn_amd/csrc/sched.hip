// sched.hip — scheduled sampling's token mix (mtn_sched_mix): the decoder inputs of the training pass, a fraction p of them replaced by
// what a first, teacher-forced pass of the model predicted for them (the two-pass, parallel form: Mihaylova & Martins 2019; Duckworth et
// al. 2019).  include/mtn_hip.h states every formula; tests/sched_refs.py is their numpy form.
// One workgroup of 256 threads per (b, t).  The coin comes first and is uniform over the workgroup (one hash of values every thread
// holds), so a kept position stores its gold token and returns without touching its logits row: at p = 0.25 three quarters of the grid
// move 8 bytes each.  That is why pick and mix are one kernel: a separate pick would read every row.  A replaced row is read once, each
// thread a lexicographic (score, column) maximum over its strided columns, then a butterfly over the 64 lanes and four LDS slots.
#include <math.h>

#include "common.h"

// p, z * inv_temperature and (...) + g are separately rounded fp32 operations (numpy float32 reproduces p bit for bit; the Gumbel scores
// are held to float64 within a bound that counts these roundings).  No contraction into an fma anywhere in this file.
#pragma clang fp contract(off)

static constexpr int SCH_THREADS = 256;
static constexpr int SCH_NONE = 0x7fffffff;                   // "no column yet": above every column, so any admitted column beats it

struct SchedArgs { mtn_sched_args a; };

struct SchBest { float s; int c; bool nan; };

__device__ __forceinline__ bool sch_excluded(const mtn_sched_args& A, int c) {
    bool x = (long)c == A.pad;
    for (int i = 0; i < A.n_banned; ++i) x = x || (c == A.banned[i]);
    return x;
}

// g = -log(-log(u)), u = (k + 0.5) * 2^-24 with k the hash's top 24 bits.  Below one half u is an fp32 number; above, 1 - u is
// (k + 0.5 would round there, and reach u = 1 at the top), so -log(u) = -log1p(-(1 - u)) from an exact argument.
__device__ __forceinline__ float sch_gumbel(uint32_t k) {
    float w;
    if (k < (1u << 23)) w = -logf(((float)k + 0.5f) * (1.0f / 16777216.0f));
    else w = -log1pf(-(((float)(16777215u - k) + 0.5f) * (1.0f / 16777216.0f)));
    return -logf(w);
}

template <int PICK>
__device__ __forceinline__ void sch_take(const mtn_sched_args& A, SchBest& b, float z, int c, uint64_t seed, uint64_t key) {
    if (sch_excluded(A, c)) return;
    float s = z;
    if (PICK == MTN_SCHED_SAMPLE) {
        const float zt = z * A.inv_temperature;
        s = zt + sch_gumbel(sample_hash(seed, key, (uint32_t)c) >> 8);
    }
    if (s != s) { b.nan = true; return; }
    if (s > b.s || (s == b.s && c < b.c)) { b.s = s; b.c = c; }
}

__device__ __forceinline__ void sch_merge(SchBest& b, float s, int c) {
    if (s > b.s || (s == b.s && c < b.c)) { b.s = s; b.c = c; }
}

template <int PICK>
__global__ __launch_bounds__(SCH_THREADS) void sched_mix_kernel(const SchedArgs SA) {
    const mtn_sched_args& A = SA.a;
    __shared__ float s_val[SCH_THREADS / 64];
    __shared__ int s_col[SCH_THREADS / 64];
    __shared__ int s_nan[SCH_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, V = A.V;
    const int b = blockIdx.x / A.T, t = blockIdx.x - b * A.T;
    const size_t at = (size_t)blockIdx.x;
    const long gold = A.trg[at];
    const bool eligible = t >= 1 && gold != A.pad;

    // the schedule and the coin: every thread computes the same values from the same (uniform) loads
    const float step = A.state[0];
    const float start = (float)A.start, ramp = (float)A.ramp;
    float p;
    if (A.ramp == 0) p = step >= start ? A.p_max : 0.0f;
    else {
        const float d = fmaxf(0.0f, step - start);
        const float q = d / ramp;
        p = A.p_max * fminf(1.0f, q);
    }
    const uint64_t seed = (uint64_t)A.seed + (uint64_t)step;
    const uint64_t key = ((uint64_t)A.key[b] << 12) | (uint64_t)t;
    const float u = (float)(sample_hash(seed, key, 0xFFFFFFFFu) >> 8) * (1.0f / 16777216.0f);
    if (!(eligible && u < p)) {                               // kept: the logits row is never touched
        if (tid == 0) {
            A.mixed[at] = gold;
            if (A.pick_score) A.pick_score[at] = __uint_as_float(0x7fc00000u);
            if (eligible) atomicAdd(&A.stats[0], 1ull);
        }
        return;
    }

    const float* xr = A.logits + (at - 1) * (size_t)A.ldx;    // row (b, t - 1): t >= 1 here
    SchBest best = {-INFINITY, SCH_NONE, false};
    if ((((uintptr_t)xr) & 15) == 0) {                        // 16-byte loads; the V % 4 tail by the first threads
        const int n4 = V >> 2;
        for (int i = tid; i < n4; i += SCH_THREADS) {
            const float4 v = *(const float4*)(xr + 4 * i);
            sch_take<PICK>(A, best, v.x, 4 * i, seed, key);
            sch_take<PICK>(A, best, v.y, 4 * i + 1, seed, key);
            sch_take<PICK>(A, best, v.z, 4 * i + 2, seed, key);
            sch_take<PICK>(A, best, v.w, 4 * i + 3, seed, key);
        }
        const int c = (n4 << 2) + tid;
        if (tid < (V & 3)) sch_take<PICK>(A, best, xr[c], c, seed, key);
    } else {
        for (int c = tid; c < V; c += SCH_THREADS) sch_take<PICK>(A, best, xr[c], c, seed, key);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float os = __shfl_xor(best.s, o, 64);
        const int oc = __shfl_xor(best.c, o, 64);
        sch_merge(best, os, oc);
    }
    const bool wave_nan = __any(best.nan);
    if (lane == 0) { s_val[wave] = best.s; s_col[wave] = best.c; s_nan[wave] = wave_nan ? 1 : 0; }
    __syncthreads();
    if (tid == 0) {
        SchBest r = {s_val[0], s_col[0], (s_nan[0] | s_nan[1] | s_nan[2] | s_nan[3]) != 0};
        sch_merge(r, s_val[1], s_col[1]);
        sch_merge(r, s_val[2], s_col[2]);
        sch_merge(r, s_val[3], s_col[3]);
        const bool picked = !r.nan && r.c != SCH_NONE;
        A.mixed[at] = picked ? (long)r.c : gold;
        if (A.pick_score) A.pick_score[at] = picked ? r.s : __uint_as_float(0x7fc00000u);
        atomicAdd(&A.stats[0], 1ull);
        if (picked) {
            atomicAdd(&A.stats[1], 1ull);
            if ((long)r.c != gold) atomicAdd(&A.stats[2], 1ull);
        }
    }
}

static bool sch_aligned(const void* p, uintptr_t a) { return (((uintptr_t)p) & (a - 1)) == 0; }

extern "C" int mtn_sched_mix(const mtn_sched_args* a, void* stream) {
    MTN_CHECK_ARG(a, "null args");
    MTN_CHECK_ARG(a->logits && a->trg && a->key && a->state && a->mixed && a->stats, "null buffer");
    MTN_CHECK_ARG(sch_aligned(a->logits, 4) && sch_aligned(a->state, 4) && sch_aligned(a->pick_score, 4),
                  "logits, state and pick_score must be 4-byte aligned");
    MTN_CHECK_ARG(sch_aligned(a->trg, 8) && sch_aligned(a->key, 8) && sch_aligned(a->mixed, 8) && sch_aligned(a->stats, 8),
                  "trg, key, mixed and stats must be 8-byte aligned");
    MTN_CHECK_ARG(a->mixed != a->trg, "mixed must be a buffer of its own (the gold ids must survive graph replays)");
    MTN_CHECK_ARG(a->B >= 0 && a->T >= 0 && a->T < 4096, "B >= 0, 0 <= T < 4096 (the position shares the hash key with key[b] << 12)");
    MTN_CHECK_ARG(a->V >= 1 && a->V < (1 << 24) && a->ldx >= a->V, "1 <= V < 2^24, ldx >= V");
    MTN_CHECK_ARG(a->pick == MTN_SCHED_ARGMAX || a->pick == MTN_SCHED_SAMPLE, "pick is MTN_SCHED_ARGMAX or MTN_SCHED_SAMPLE");
    MTN_CHECK_ARG(a->p_max >= 0.0f && a->p_max <= 1.0f && a->start >= 0 && a->ramp >= 0, "0 <= p_max <= 1, start >= 0, ramp >= 0");
    MTN_CHECK_ARG(a->n_banned >= 0 && a->n_banned <= 4, "at most 4 banned tokens");
    MTN_CHECK_ARG(a->inv_temperature > 0.0f && a->inv_temperature <= 3.4028234e38f, "inv_temperature must be finite and > 0");
    if (a->B == 0 || a->T == 0) return MTN_OK;
    MTN_CHECK_ARG((long)a->B * a->T <= 0x7fffffffL, "B * T must fit the grid");
    SchedArgs SA; SA.a = *a;
    const dim3 grid((unsigned)((long)a->B * a->T)), block(SCH_THREADS);
    if (a->pick == MTN_SCHED_ARGMAX)
        hipLaunchKernelGGL(sched_mix_kernel<MTN_SCHED_ARGMAX>, grid, block, 0, (hipStream_t)stream, SA);
    else
        hipLaunchKernelGGL(sched_mix_kernel<MTN_SCHED_SAMPLE>, grid, block, 0, (hipStream_t)stream, SA);
    MTN_CHECK_LAUNCH();
    return MTN_OK;
}
