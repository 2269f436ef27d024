// sample.hip — stochastic decoding on the device: one workgroup turns a row of log-probabilities into ONE drawn token (temperature,
// top-k, nucleus), so that a sampling search runs as one captured graph like the beam search does (select.hip), without parents, ancestor
// re-ordering or a tie fallback.  Definitions (include/mtn_hip.h restates them; tests/sample_refs.py is their float64 form):
//   ban      up to 4 token ids, and <eos> while the row's position is below min_len, get probability 0;
//   T        e_i = exp((x_i - max) / T) over the rest;
//   top-k    keep x_i >= the k-th largest x (ties at the threshold all kept): a bitwise bisection over the monotone integer key of the
//            float with workgroup-wide counts — 32 counts whatever k is, no sort;
//   top-p    over what top-k kept, keep e_i >= t*, t* the largest threshold whose kept mass is >= top_p x mass (ties all kept): the same
//            bisection over the bits of e (non-negative floats order like their bits) with workgroup-wide sums;
//   draw     u = 24 bits of a counter hash of (seed, key[row], position) / 2^24; the token is the first kept index in vocabulary order
//            whose running kept mass exceeds u x kept mass.
// Thread t owns the CONTIGUOUS columns [t * C, (t + 1) * C), C = ceil(V / 256): the running mass of the draw is then a per-thread
// sequential sum behind an exclusive scan of the 256 chunk sums, and every workgroup-wide sum is 256 chunk sums plus a tree — the same
// order in every pass, so a sum is monotone in the set it runs over and the bisections are exact on the kernel's own arithmetic.
// Rows of up to 4096 columns live in registers (16 per thread); longer rows are re-read (L2) in every pass.
#include "common.h"

static constexpr int SMP_THREADS = 256;
static constexpr int SMP_PER = 16;                            // columns per thread on the register path

// sample_hash(seed, key, position), the counter hash of the draw, lives in common.h (sched.hip draws from it too).

// monotone integer key of a float: a < b  <=>  key(a) < key(b)  (-0 below +0)
__device__ __forceinline__ uint32_t float_key(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u >> 31) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_float(uint32_t k) {
    return __uint_as_float((k >> 31) ? (k & 0x7fffffffu) : ~k);
}

// Workgroup-wide sum, the same value in every thread: wave butterflies, then the four wave sums in a fixed order.  Two LDS slots used
// alternately: one barrier per call (a thread can be at most one call ahead of another).
__device__ __forceinline__ float smp_block_sum(float v, float* s_red, int& phase) {
    v = wave_sum(v);
    float* s = s_red + (phase & 1) * 4;
    ++phase;
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
    __syncthreads();
    return (s[0] + s[1]) + (s[2] + s[3]);
}

struct SampleArgs { mtn_sample_args a; };

__device__ __forceinline__ bool smp_banned(const mtn_sample_args& A, int c, bool eos_off) {
    bool b = eos_off && c == A.eos;
    for (int i = 0; i < A.n_banned; ++i) b = b || (c == A.banned[i]);
    return b;
}

template <bool REGS>
__global__ __launch_bounds__(SMP_THREADS) void sample_rows_kernel(const SampleArgs SA) {
    const mtn_sample_args& A = SA.a;
    __shared__ float s_red[8];
    __shared__ float s_wave[SMP_THREADS / 64];
    __shared__ int s_first, s_last;
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, V = A.V;
    const int l = A.step[row];                                // tokens this row has drawn so far = the position being extended
    if (l < 0 || l >= A.L) return;                            // (the log has L entries per row)
    const float* xr = A.logp + (size_t)row * A.ldx;
    const int C = (V + SMP_THREADS - 1) / SMP_THREADS, c0 = tid * C, c1 = min(V, c0 + C);
    const bool eos_off = l < A.min_len;
    int phase = 0;
    if (tid == 0) { s_first = 0x7fffffff; s_last = -1; }

    // x of this thread's columns, banned columns at -inf
    float v[SMP_PER];
    auto x_at = [&](int c) { return smp_banned(A, c, eos_off) ? -INFINITY : xr[c]; };
    if (REGS) {
#pragma unroll
        for (int i = 0; i < SMP_PER; ++i) v[i] = (c0 + i < c1) ? x_at(c0 + i) : -INFINITY;
    }
    float mx = -INFINITY;
    if (REGS) {
#pragma unroll
        for (int i = 0; i < SMP_PER; ++i) mx = fmaxf(mx, v[i]);
    } else {
        for (int c = c0; c < c1; ++c) mx = fmaxf(mx, x_at(c));
    }
    mx = wave_max(mx);
    if (lane == 0) s_wave[wave] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(s_wave[0], s_wave[1]), fmaxf(s_wave[2], s_wave[3]));

    // top-k: the largest key with at least k columns at or above it is the key of the k-th largest x (counts below 2^24 are exact floats)
    float xk = -INFINITY;
    if (A.top_k > 0 && A.top_k < V) {
        const float need = (float)A.top_k;
        uint32_t t = 0;
        for (int bit = 31; bit >= 0; --bit) {
            const uint32_t cand = t | (1u << bit);
            float n = 0.f;
            if (REGS) {
#pragma unroll
                for (int i = 0; i < SMP_PER; ++i) n += (c0 + i < c1 && float_key(v[i]) >= cand) ? 1.f : 0.f;
            } else {
                for (int c = c0; c < c1; ++c) n += float_key(x_at(c)) >= cand ? 1.f : 0.f;
            }
            if (smp_block_sum(n, s_red, phase) >= need) t = cand;
        }
        xk = key_float(t);
    }

    // e_i = exp((x_i - max) / T) of what is left (0 elsewhere, and everywhere in a row with nothing left)
    const float T = A.temperature;
    auto e_of = [&](float x) { return (x >= xk && x > -INFINITY) ? expf((x - mx) / T) : 0.f; };
    if (REGS) {
#pragma unroll
        for (int i = 0; i < SMP_PER; ++i) v[i] = e_of(v[i]);
    }
    auto e_at = [&](int c) { return e_of(x_at(c)); };         // (the long-row path recomputes)

    // top-p: the largest threshold (as the bits of a non-negative float) whose kept mass reaches top_p x mass
    float tp = 0.f;
    if (A.top_p < 1.f) {
        float part = 0.f;
        if (REGS) {
#pragma unroll
            for (int i = 0; i < SMP_PER; ++i) part += v[i];
        } else {
            for (int c = c0; c < c1; ++c) part += e_at(c);
        }
        const float need = A.top_p * smp_block_sum(part, s_red, phase);
        uint32_t t = 0;
        for (int bit = 30; bit >= 0; --bit) {
            const uint32_t cand = t | (1u << bit);
            const float th = __uint_as_float(cand);
            part = 0.f;
            if (REGS) {
#pragma unroll
                for (int i = 0; i < SMP_PER; ++i) part += v[i] >= th ? v[i] : 0.f;
            } else {
                for (int c = c0; c < c1; ++c) { const float e = e_at(c); part += e >= th ? e : 0.f; }
            }
            if (smp_block_sum(part, s_red, phase) >= need) t = cand;
        }
        tp = __uint_as_float(t);
    }

    // draw: exclusive scan of the chunk masses, then each thread walks its chunk
    float mine = 0.f;
    if (REGS) {
#pragma unroll
        for (int i = 0; i < SMP_PER; ++i) mine += v[i] >= tp ? v[i] : 0.f;
    } else {
        for (int c = c0; c < c1; ++c) { const float e = e_at(c); mine += e >= tp ? e : 0.f; }
    }
    float incl = mine;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const float o = __shfl_up(incl, off, 64);
        if (lane >= off) incl += o;
    }
    __syncthreads();                                          // (s_wave held the maxima)
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    const float up = __shfl_up(incl, 1, 64);
    float before = 0.f;
    for (int w = 0; w < wave; ++w) before += s_wave[w];
    if (lane) before += up;
    const float mass = ((s_wave[0] + s_wave[1]) + s_wave[2]) + s_wave[3];
    const uint32_t hbits = sample_hash((uint64_t)A.seed[0], (uint64_t)A.key[row], (uint32_t)l) >> 8;
    const float u = (float)hbits * (1.0f / 16777216.0f);
    const float target = u * mass;
    float run = before;
    int first = 0x7fffffff, last = -1;
    if (REGS) {
#pragma unroll
        for (int i = 0; i < SMP_PER; ++i) {
            const float e = v[i];
            if (e >= tp && e > 0.f) {
                run += e;
                last = c0 + i;
                if (run > target && first == 0x7fffffff) first = c0 + i;
            }
        }
    } else {
        for (int c = c0; c < c1; ++c) {
            const float e = e_at(c);
            if (e >= tp && e > 0.f) {
                run += e;
                last = c;
                if (run > target && first == 0x7fffffff) first = c;
            }
        }
    }
    if (first != 0x7fffffff) atomicMin(&s_first, first);
    if (last >= 0) atomicMax(&s_last, last);
    __syncthreads();
    if (tid == 0) {
        // (rounding can leave the last running mass at or below u x mass: the last kept column then; 0 in a row with nothing to draw)
        int w = s_first != 0x7fffffff ? s_first : s_last;
        if (w < 0 || w >= V) w = 0;
        const size_t at = (size_t)l * gridDim.x + row;
        A.log_tok[at] = w;
        A.log_logp[at] = xr[w];
        A.log_u[at] = u;
        A.step[row] = l + 1;
        if (A.tokens) A.tokens[row] = (long)w;
        if (A.anc && l + 1 < A.L) A.anc[(size_t)row * A.L + l + 1] = row;
        if (A.pos && row == 0) *A.pos = l + 1;                  // (read by the NEXT decode step only)
    }
}

extern "C" int mtn_sample_rows(const mtn_sample_args* a, void* stream) {
    MTN_CHECK_ARG(a && a->logp && a->seed && a->key && a->step && a->log_tok && a->log_logp && a->log_u, "null buffer");
    MTN_CHECK_ARG(a->rows > 0 && a->V > 0 && a->V < (1 << 24) && (a->ldx == 0 || a->ldx >= a->V) && a->L >= 1, "bad row matrix");
    MTN_CHECK_ARG(a->temperature > 0.f && a->top_k >= 0 && a->top_p > 0.f && a->top_p <= 1.f, "temperature > 0, top_k >= 0, 0 < top_p <= 1");
    MTN_CHECK_ARG(a->n_banned >= 0 && a->n_banned <= 4 && a->min_len >= 0, "at most 4 banned tokens");
    SampleArgs SA; SA.a = *a;
    if (a->V <= SMP_PER * SMP_THREADS)
        hipLaunchKernelGGL(sample_rows_kernel<true>, dim3(a->rows), dim3(SMP_THREADS), 0, (hipStream_t)stream, SA);
    else
        hipLaunchKernelGGL(sample_rows_kernel<false>, dim3(a->rows), dim3(SMP_THREADS), 0, (hipStream_t)stream, SA);
    MTN_CHECK_LAUNCH();
    return MTN_OK;
}
