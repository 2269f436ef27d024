// mbr.hip — minimum-Bayes-risk selection over the hypotheses of a dialogue (samples or an n-best list) on the device: one workgroup owns a
// set of K <= 16 hypotheses of at most 128 tokens and answers with the one that agrees most, in n-grams, with the others.
// include/mtn_hip.h mtn_mbr_select holds the definition (tests/mbr_refs.py is its numpy form); not in the reference, like sampling.
//   U(h, r)   = (F_1 + .. + F_N) / N,  F_n = 2 m_n / (c_n(h) + c_n(r)),  m_n the clipped n-gram match count, c_n(h) = max(len(h) - n + 1, 0)
//   E_i       = sum_j w_j U(h_i, h_j) in ascending j, one multiply and one add per step (never an fma)
//   best      = the largest E, the lower index among equals; order = all indices by descending E, stable.
// Clipping without a table of grams: occurrence number k (0-based, by position) of a gram in h counts iff r holds more than k of it —
// summed over the occurrences that is min(count in h, count in r).  So
//   phase 1  every position p of every hypothesis: how many EARLIER positions of the same hypothesis start the same n-gram (n = 1..4),
//            four bytes in LDS (a count is < 128);
//   phase 2  pairs i <= j (U is symmetric), one wave per pair: a lane owns position p of h_i, walks the positions q of h_j with a sliding
//            window of four tokens (every lane reads the same LDS words: broadcasts) and takes the leading-match length of (p, q) once —
//            the n-gram at p equals the one at q iff that length is >= n, for all four orders; position p counts for order n iff its
//            occurrence number is below the number of matching q.  Integer sums over the lanes by shuffles;
//   phase 3  a thread per (i, j): the doubles F_n and U, in the stated order, from the integer counts;
//   phase 4  a thread per i: E_i, then its rank among the E (K^2 comparisons).
// Everything before phase 3 is integer, every double operation after it is a single IEEE operation in a fixed order in one thread: two
// launches give the same bits, and a set's results depend on nothing outside the set.  No atomics; every store is a vector store.
#include "common.h"

// E_i is one multiply then one add per step.  The compiler contracts a + b * c into an fma by default, and HIP's __dmul_rn / __dadd_rn
// are plain operators that inline into the same contraction: from here on no expression of this file may be contracted.
#pragma clang fp contract(off)

static constexpr int MBR_THREADS = 1024;                         // 16 waves: the pairs of a full set are 136 short serial walks, so more waves is less time
static constexpr int MBR_WAVES = MBR_THREADS / 64;
static constexpr int MBR_MAX_L = 128;                          // tokens of a hypothesis

struct MbrArgs { mtn_mbr_args a; };

// How many of the positions q in [0, q_end) of r (length nr) start the same n-gram as the window a[0..na-1] (na <= 4 tokens that exist
// at a position of h), for n = 1..4: cnt[n-1].  The leading-match length of (p, q) decides all four orders.
__device__ __forceinline__ void mbr_count(const int* r, int nr, int q_end, const int a[4], int na, int cnt[4]) {
    cnt[0] = cnt[1] = cnt[2] = cnt[3] = 0;
    int b0 = 0 < nr ? r[0] : 0, b1 = 1 < nr ? r[1] : 0, b2 = 2 < nr ? r[2] : 0;
    for (int q = 0; q < q_end; ++q) {
        const int b3 = q + 3 < nr ? r[q + 3] : 0;
        const int lim = min(na, nr - q);                          // tokens both windows hold
        int ml = 0;
        if (lim > 0 && a[0] == b0) {
            ml = 1;
            if (lim > 1 && a[1] == b1) {
                ml = 2;
                if (lim > 2 && a[2] == b2) ml = (lim > 3 && a[3] == b3) ? 4 : 3;
            }
        }
        cnt[0] += ml >= 1; cnt[1] += ml >= 2; cnt[2] += ml >= 3; cnt[3] += ml >= 4;
        b0 = b1; b1 = b2; b2 = b3;
    }
}

__global__ __launch_bounds__(MBR_THREADS) void mbr_select_kernel(const MbrArgs MA) {
    const mtn_mbr_args& A = MA.a;
    __shared__ int s_tok[MTN_MBR_MAX_HYP][MBR_MAX_L];
    __shared__ unsigned s_occ[MTN_MBR_MAX_HYP][MBR_MAX_L];     // byte n-1: earlier positions of the hypothesis with the same n-gram
    __shared__ int s_m[MTN_MBR_MAX_HYP][MTN_MBR_MAX_HYP][4];   // m_n of the pairs i <= j
    __shared__ double s_u[MTN_MBR_MAX_HYP][MTN_MBR_MAX_HYP], s_e[MTN_MBR_MAX_HYP], s_w[MTN_MBR_MAX_HYP];
    __shared__ int s_len[MTN_MBR_MAX_HYP];
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int K = A.K, L = A.L, N = A.N;
    const size_t sk = (size_t)s * K;

    // ---- phase 0: the set's tokens and lengths in LDS
    int n;
    if (A.tok) {
        n = min(max(A.n_hyp[s], 0), K);
        for (int e = tid; e < K * L; e += MBR_THREADS) {
            const int k = e / L, l = e - k * L;
            s_tok[k][l] = A.tok[(sk + k) * A.ldl + l];
        }
        if (tid < K) s_len[tid] = tid < n ? min(max(A.len[sk + tid], 0), L) : 0;
    } else {
        n = K;
        const size_t cols = (size_t)A.sets * K;
        for (int e = tid; e < K * L; e += MBR_THREADS) {
            const int l = e / K, k = e - l * K;
            s_tok[k][l] = A.log_tok[(size_t)l * cols + sk + k];
        }
        __syncthreads();
        if (tid < K) {                                          // the tokens before the first <eos>; L - 1 of them without one
            int len = L - 1;
            for (int l = L - 1; l >= 0; --l) if (s_tok[tid][l] == A.eos) len = l;
            s_len[tid] = len;
        }
    }
    if (tid < K) s_w[tid] = tid < n ? (A.w ? A.w[sk + tid] : 1.0 / (double)n) : 0.0;
    __syncthreads();

    // ---- phase 1: occurrence numbers
    for (int e = tid; e < n * L; e += MBR_THREADS) {
        const int k = e / L, p = e - k * L, len = s_len[k];
        if (p >= len) continue;
        const int na = min(4, len - p);
        int a[4], cnt[4];
        for (int t = 0; t < 4; ++t) a[t] = t < na ? s_tok[k][p + t] : 0;
        mbr_count(s_tok[k], len, p, a, na, cnt);
        s_occ[k][p] = (unsigned)cnt[0] | ((unsigned)cnt[1] << 8) | ((unsigned)cnt[2] << 16) | ((unsigned)cnt[3] << 24);
    }
    __syncthreads();

    // ---- phase 2: m_n of the pairs i <= j, a wave per pair (the pair index is the same in every lane of a wave: all 64 reach the shuffles)
    int c = 0;
    for (int i = 0; i < n; ++i) {
        for (int j = i; j < n; ++j, ++c) {
            if (c % MBR_WAVES != wave) continue;
            const int li = s_len[i], lj = s_len[j];
            int m[4] = {0, 0, 0, 0};
            for (int p = lane; p < li; p += 64) {
                const int na = min(4, li - p);
                int a[4], cnt[4];
                for (int t = 0; t < 4; ++t) a[t] = t < na ? s_tok[i][p + t] : 0;
                mbr_count(s_tok[j], lj, lj, a, na, cnt);
                const unsigned occ = s_occ[i][p];
                for (int t = 0; t < 4; ++t) m[t] += (int)((occ >> (8 * t)) & 255u) < cnt[t];
            }
            for (int t = 0; t < 4; ++t) {
                int v = m[t];
                for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
                if (lane == 0) s_m[i][j][t] = v;
            }
        }
    }
    __syncthreads();

    // ---- phase 3: U of every ordered pair from the counts of its unordered one (c_n(h_i) + c_n(h_j) is an integer: the same bits both ways)
    if (tid < K * K) {
        const int i = tid / K, j = tid - i * K;
        double u = 0.0;
        if (i < n && j < n) {
            const int lo = min(i, j), hi = max(i, j), li = s_len[i], lj = s_len[j];
            for (int t = 1; t <= N; ++t) {
                const int den = max(li - t + 1, 0) + max(lj - t + 1, 0);
                const double f = den > 0 ? (double)(2 * s_m[lo][hi][t - 1]) / (double)den : 0.0;
                u = u + f;
            }
            u = u / (double)N;
        }
        s_u[i][j] = u;
        if (A.util) A.util[(sk + i) * K + j] = u;
    }
    __syncthreads();

    // ---- phase 4: expected utilities, then their ranks
    if (tid < K) {
        double e = -1.0;
        if (tid < n) {
            e = 0.0;
            for (int j = 0; j < n; ++j) { const double t = s_w[j] * s_u[tid][j]; e = e + t; }   // (contraction is off in this file)
        }
        s_e[tid] = e;
        A.expected[sk + tid] = e;
    }
    __syncthreads();
    if (tid < K) {
        int rank = tid;                                        // entries past n_hyp follow the valid ones, by ascending index
        if (tid < n) {
            const double e = s_e[tid];
            rank = 0;
            for (int j = 0; j < n; ++j) rank += (s_e[j] > e) || (s_e[j] == e && j < tid);
            if (rank == 0) A.best[s] = tid;
        }
        A.order[sk + rank] = tid;
    }
    if (tid == 0 && n == 0) A.best[s] = -1;
}

extern "C" int mtn_mbr_select(const mtn_mbr_args* a, void* stream) {
    MTN_CHECK_ARG(a, "null arguments");
    MTN_CHECK_ARG(a->expected && a->best && a->order, "null output buffer");
    MTN_CHECK_ARG(a->sets >= 1 && a->K >= 1 && a->K <= MTN_MBR_MAX_HYP, "sets >= 1, 1 <= K <= 16");
    MTN_CHECK_ARG(a->L >= 1 && a->L <= MBR_MAX_L && a->N >= 1 && a->N <= 4, "1 <= L <= 128, 1 <= N <= 4");
    if (a->tok) {
        MTN_CHECK_ARG(a->len && a->n_hyp && a->ldl >= a->L, "explicit hypotheses: len, n_hyp, ldl >= L");
    } else {
        MTN_CHECK_ARG(a->log_tok, "a source of hypotheses: tok, or the sample log");
    }
    MbrArgs MA; MA.a = *a;
    hipLaunchKernelGGL(mbr_select_kernel, dim3(a->sets), dim3(MBR_THREADS), 0, (hipStream_t)stream, MA);
    MTN_CHECK_LAUNCH();
    return MTN_OK;
}
