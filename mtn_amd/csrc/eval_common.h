// eval_common.h — the device code of the corpus metrics (BLEU-1..4, ROUGE-L, CIDEr; include/mtn_hip.h mtn_eval_metrics holds the definition,
// tests/eval_refs.py is its Python form), shared by eval.hip (mtn_eval_metrics: table and items of one evaluated corpus) and scst.hip
// (mtn_eval_table_build / mtn_eval_score_rows: the table of a fixed reference corpus, then any hypothesis rows against its items).  Only
// __device__ bodies live here; each file wraps them in __global__ kernels of its own.
//   clear   ev_clear_body   zeroes the workspace (the table's keys and counts).
//   table   ev_df_body      the document-frequency table, one workgroup per item.  Open addressing with linear probing in device memory.  A
//                          slot's key is a 32-bit HANDLE, 1 + (((q R + r) L + p) << 2 | n - 1): where one occurrence of the n-gram lies in
//                          the immutable reference array.  An empty slot is claimed with one compare-and-swap; a probe that meets a taken
//                          slot compares the tokens behind its handle with its own.  A key goes from 0 to its final value once, so nothing
//                          is published in two steps and no thread spins.  Within an item an n-gram is inserted by its FIRST occurrence
//                          over the item's references alone (no earlier position of the item starts the same n-gram), so df counts items;
//                          the count is an integer atomic add (no float atomics anywhere; after the per-item test an n-gram is added
//                          once per item that holds it, and the adds spread over the whole table): exact in any arrival order.
//   item    ev_item_body    one workgroup per hypothesis, all the tokens of its item in LDS.
//                            phase 1  the df of every n-gram of the item by one table lookup per position and order; then per position of every
//                                     sentence how many positions of the sentence start the same n-gram (n = 1..4) and how many EARLIER ones
//                                     do, by the sliding-window walk of mbr.hip, and the squared CIDEr norms summed over first occurrences;
//                            phase 2  a thread per (reference r, hypothesis position p) walks r once: count_r of the four n-grams at p (for
//                                     the clipped matches and for CIDEr's min(v_h, v_r) v_r) and the 128-bit mask of the q with r[q] = h[p];
//                            phase 3  clipped matches: occurrence number k of a gram in h counts iff max_r count_r > k (the max over the
//                                     references comes before the clipping).  LCS: one thread per reference runs the bit-parallel row
//                                     recurrence V' = (V + (V & M)) | (V & ~M) over two 64-bit words, LCS = zero bits of V below len(r).
//                                     Chosen over an anti-diagonal sweep because the masks M fall out of the walk phase 2 makes anyway and
//                                     what is left is at most 128 steps of two-word arithmetic per reference, against 255 barriers;
//                            phase 4  one thread: the item's ten integers, ROUGE-L and CIDEr.
// All floating point is double.  A sum across lanes is a fixed butterfly inside a wave, then the waves' partials in ascending order in one
// thread: two launches give the same bytes.  Tokens are compared and hashed, never used as indices.  Every store is a vector store.
#pragma once
#include "common.h"

static constexpr int EV_THREADS = 1024;                          // 8 references x 128 positions: a thread per (reference, position)
static constexpr int EV_RED = 256;                                // threads of the reduction: room for its registers without spills
static constexpr int EV_L = 128;                                 // tokens of a sentence
static constexpr int EV_R = MTN_EVAL_MAX_REF;
static constexpr int EV_HYP = EV_R;                              // the hypothesis' row of the LDS token table
static constexpr unsigned long long EV_MAX_TOKENS = 1ull << 28;  // Q R L: handles and the table's capacity stay below 2^32

struct EvalArgs { mtn_eval_args a; unsigned* key; int* cnt; unsigned mask; };

static unsigned long long ev_capacity(int Q, int R, int L) {     // a power of two >= 2 x 4 x (the most reference tokens)
    const unsigned long long need = 8ull * (unsigned long long)Q * (unsigned long long)R * (unsigned long long)L;
    unsigned long long cap = 1024;
    while (cap < need) cap <<= 1;
    return cap;
}

__device__ __forceinline__ unsigned ev_hash(const int a[4], int n) {
    unsigned h = mix32((unsigned)a[0] ^ (0x9E3779B9u * (unsigned)n));
    for (int t = 1; t < n; ++t) h = mix32((h ^ ((unsigned)a[t] * 0x85EBCA6Bu)) + (unsigned)t);
    return h;
}

// Is the n-gram behind a slot's handle the n-gram a[0..n-1]?  (A handle names a position that holds n tokens: the read stays inside its row.)
__device__ __forceinline__ bool ev_same(const EvalArgs& E, unsigned handle, const int a[4], int n) {
    const unsigned v = handle - 1u;
    if ((int)(v & 3u) + 1 != n) return false;
    const unsigned pos = v >> 2, row = pos / (unsigned)E.a.L, p = pos - row * (unsigned)E.a.L;
    const int* t = E.a.ref + (size_t)row * (size_t)E.a.ldl + p;
    for (int i = 0; i < n; ++i) if (t[i] != a[i]) return false;
    return true;
}

__device__ __forceinline__ void ev_insert(const EvalArgs& E, unsigned handle, const int a[4], int n) {
    unsigned s = ev_hash(a, n) & E.mask;
    for (unsigned probe = 0; probe <= E.mask; ++probe, s = (s + 1u) & E.mask) {       // bounded by the capacity
        unsigned k = __hip_atomic_load(&E.key[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (k == 0u) {
            const unsigned old = atomicCAS(&E.key[s], 0u, handle);
            k = old == 0u ? handle : old;
        }
        if (k == handle || ev_same(E, k, a, n)) { atomicAdd(&E.cnt[s], 1); return; }
    }
}

__device__ __forceinline__ int ev_lookup(const EvalArgs& E, const int a[4], int n) {   // 0 for an n-gram no reference holds
    unsigned s = ev_hash(a, n) & E.mask;
    for (unsigned probe = 0; probe <= E.mask; ++probe, s = (s + 1u) & E.mask) {
        const unsigned k = E.key[s];
        if (k == 0u) return 0;
        if (ev_same(E, k, a, n)) return E.cnt[s];
    }
    return 0;
}

// One walk over the positions q of sentence r (nr tokens) with the window a[0..na-1] (the na <= 4 tokens that exist at a position of some
// sentence).  Byte n-1 of `tot`: how many q start the same n-gram (the leading-match length of the two windows decides all four orders; a
// count is <= 128, so the bytes never carry); of `early`: how many of them with q < q_snap; m: bit q set where r[q] = a[0].
__device__ __forceinline__ void ev_walk(const int* r, int nr, int q_snap, const int a[4], int na, unsigned& tot, unsigned& early, uint64_t m[2]) {
    unsigned t = 0, e = 0;
    uint64_t m0 = 0, m1 = 0;
    int b0 = 0 < nr ? r[0] : 0, b1 = 1 < nr ? r[1] : 0, b2 = 2 < nr ? r[2] : 0;
    for (int q = 0; q < nr; ++q) {
        if (q == q_snap) e = t;
        const int b3 = q + 3 < nr ? r[q + 3] : 0;
        const int lim = min(na, nr - q);
        int ml = 0;
        if (lim > 0 && a[0] == b0) {
            ml = 1;
            if (lim > 1 && a[1] == b1) {
                ml = 2;
                if (lim > 2 && a[2] == b2) ml = (lim > 3 && a[3] == b3) ? 4 : 3;
            }
        }
        if (ml > 0) {
            t += 0x01010101u >> (8 * (4 - ml));
            if (q < 64) m0 |= 1ull << q; else m1 |= 1ull << (q - 64);
        }
        b0 = b1; b1 = b2; b2 = b3;
    }
    if (q_snap >= nr) e = t;
    tot = t; early = e; m[0] = m0; m[1] = m1;
}

__device__ __forceinline__ double ev_wave_sum(double v) {        // the same butterfly for the same lanes: a fixed order
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ long long ev_wave_sum(long long v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ void ev_clear_body(uint4* w, size_t n16) {   // blocks of 256 threads
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (size_t)gridDim.x * 256) w[i] = make_uint4(0u, 0u, 0u, 0u);
}

// The item's references in LDS (rows past n_ref and tokens past a length are zero and never compared); returns n_ref clamped to [1, R].
__device__ __forceinline__ int ev_load_refs(const mtn_eval_args& A, int q, int (*s_tok)[EV_L], int* s_len) {
    const int tid = threadIdx.x, r = tid >> 7, p = tid & 127;
    const int nr = min(max(A.n_ref[q], 1), A.R);
    const size_t row = (size_t)q * A.R + r;
    int len = 0;
    if (r < nr) len = min(max(A.ref_len[row], 0), A.L);
    s_tok[r][p] = p < len ? A.ref[row * (size_t)A.ldl + p] : 0;
    if (p == 0) s_len[r] = len;
    return nr;
}

// One workgroup of EV_THREADS per item (blockIdx.x): the item's n-grams into the table.
__device__ __forceinline__ void ev_df_body(const EvalArgs& E) {
    const mtn_eval_args& A = E.a;
    __shared__ int s_tok[EV_R][EV_L];
    __shared__ int s_len[EV_R];
    const int q = blockIdx.x, tid = threadIdx.x, r = tid >> 7, p = tid & 127;
    const int nr = ev_load_refs(A, q, s_tok, s_len);
    __syncthreads();
    if (r >= nr || p >= s_len[r]) return;
    const int len = s_len[r], na = min(4, len - p);
    int a[4];
    for (int t = 0; t < 4; ++t) a[t] = t < na ? s_tok[r][p + t] : 0;
    unsigned seen = 0, tot, early;
    uint64_t m[2];
    for (int rr = 0; rr < r; ++rr) {                             // every position of the references before this one
        ev_walk(s_tok[rr], s_len[rr], 0, a, na, tot, early, m);
        seen |= tot;
    }
    ev_walk(s_tok[r], len, p, a, na, tot, early, m);             // the earlier positions of this one
    seen |= early;
    const unsigned pos = (unsigned)(((size_t)q * A.R + r) * A.L + p);
    for (int n = 1; n <= na; ++n)
        if (((seen >> (8 * (n - 1))) & 255u) == 0u) ev_insert(E, 1u + ((pos << 2) | (unsigned)(n - 1)), a, n);
}

// One workgroup of EV_THREADS: hypothesis row `o` of A.hyp / A.hyp_len against the references of item `q`, df from the table behind E,
// Q = A.Q; the numbers go to row `o` of A.stats / A.rouge / A.cider.  mtn_eval_metrics: o == q.  Reads the table, never writes it.
__device__ __forceinline__ void ev_item_body(const EvalArgs& E, const int q, const int o) {
    const mtn_eval_args& A = E.a;
    __shared__ int s_tok[EV_R + 1][EV_L];                        // row EV_HYP: the hypothesis
    __shared__ int s_len[EV_R + 1];
    __shared__ unsigned s_hc[EV_L], s_ho[EV_L];                  // hypothesis position: count of its n-grams in h, and its occurrence numbers
    __shared__ double s_idf[EV_L][4];                            // ... and their idf
    __shared__ int s_df[EV_R + 1][EV_L][4];                      // df of the n-gram at every position of every sentence (0 where there is none)
    __shared__ unsigned s_cr[EV_R][EV_L];                        // count in reference r of the n-grams at hypothesis position p
    __shared__ uint64_t s_mask[EV_R][EV_L][2];                   // bit j: r[j] == h[p]
    __shared__ double s_n2[(EV_R + 1) * 2][4];                   // squared norms, by wave (two waves per sentence)
    __shared__ double s_sim[EV_R * 2][4];                        // sim_n(h, r) before the norms, by wave
    __shared__ int s_match[2][4];
    __shared__ int s_lcs[EV_R];
    const int tid = threadIdx.x, lane = tid & 63;
    const int R = A.R, L = A.L;

    // ---- phase 0: tokens and lengths in LDS
    const int nr = ev_load_refs(A, q, s_tok, s_len);
    if (tid < EV_L) {
        const int len = min(max(A.hyp_len[o], 0), L);
        s_tok[EV_HYP][tid] = tid < len ? A.hyp[(size_t)o * (size_t)A.ldl + tid] : 0;
        if (tid == 0) s_len[EV_HYP] = len;
    }
    __syncthreads();
    const int lh = s_len[EV_HYP];
    const double log_q = log((double)A.Q);

    // ---- phase 1a: the df of every n-gram of the item, a thread per (sentence, position, order).  A lookup is a chain of dependent loads
    //      (the key, the tokens behind it, the count); one order per thread puts the chains of an item side by side, not behind each other:
    //      with the four orders of a position in one thread the launch took 161 us on 1 710 items of <= 16 tokens, mostly waiting; 64 us so.
    //      The hypothesis takes the place behind the launch's R references, so at R < 8 one sweep covers the item.
    for (int e = tid; e < (R + 1) * EV_L * 4; e += EV_THREADS) {
        const int si = e >> 9, p = (e >> 2) & 127, n = (e & 3) + 1, s = si < R ? si : EV_HYP;
        int df = 0;
        if (p + n <= s_len[s]) {
            int a[4];
            for (int t = 0; t < 4; ++t) a[t] = t < n ? s_tok[s][p + t] : 0;
            df = ev_lookup(E, a, n);
        }
        s_df[s][p][n - 1] = df;
        if (A.df_of_ref && si < R && p < L) A.df_of_ref[(((size_t)q * R + si) * L + p) * 4 + (n - 1)] = df;
    }
    __syncthreads();

    // ---- phase 1b: per position of every sentence the counts inside the sentence and the squared norms (a wave is 64 positions of one
    //      sentence: the bounds of this loop are the same in all its lanes, so all of them reach the shuffles)
    for (int e = tid; e < (R + 1) * EV_L; e += EV_THREADS) {
        const int si = e >> 7, p = e & 127, s = si < R ? si : EV_HYP, len = s_len[s];
        double n2[4] = {0.0, 0.0, 0.0, 0.0};
        if (p < len) {
            const int na = min(4, len - p);
            int a[4];
            for (int t = 0; t < 4; ++t) a[t] = t < na ? s_tok[s][p + t] : 0;
            unsigned tot, early;
            uint64_t m[2];
            ev_walk(s_tok[s], len, p, a, na, tot, early, m);
            for (int n = 1; n <= na; ++n) {
                const double idf = log_q - log((double)max(1, s_df[s][p][n - 1]));
                if (s == EV_HYP) s_idf[p][n - 1] = idf;
                if (((early >> (8 * (n - 1))) & 255u) == 0u) {   // the first occurrence stands for the distinct n-gram
                    const double v = (double)((tot >> (8 * (n - 1))) & 255u) * idf;
                    n2[n - 1] = v * v;
                }
            }
            if (s == EV_HYP) { s_hc[p] = tot; s_ho[p] = early; }
        }
        for (int n = 0; n < 4; ++n) {
            const double v = ev_wave_sum(n2[n]);
            if (lane == 0) s_n2[2 * s + (p >> 6)][n] = v;
        }
    }
    __syncthreads();

    // ---- phase 2: a thread per (reference, hypothesis position) — a wave is 64 positions against one reference
    {
        const int r = tid >> 7, p = tid & 127;
        if (r < nr) {
            double sp[4] = {0.0, 0.0, 0.0, 0.0};
            unsigned cr = 0, early;
            uint64_t m[2] = {0, 0};
            if (p < lh) {
                const int na = min(4, lh - p);
                int a[4];
                for (int t = 0; t < 4; ++t) a[t] = t < na ? s_tok[EV_HYP][p + t] : 0;
                ev_walk(s_tok[r], s_len[r], 0, a, na, cr, early, m);
                const unsigned hc = s_hc[p], ho = s_ho[p];
                for (int n = 1; n <= na; ++n) {
                    if (((ho >> (8 * (n - 1))) & 255u) != 0u) continue;
                    const double idf = s_idf[p][n - 1];
                    const double vh = (double)((hc >> (8 * (n - 1))) & 255u) * idf, vr = (double)((cr >> (8 * (n - 1))) & 255u) * idf;
                    sp[n - 1] = fmin(vh, vr) * vr;
                }
            }
            s_cr[r][p] = cr;
            s_mask[r][p][0] = m[0];
            s_mask[r][p][1] = m[1];
            for (int n = 0; n < 4; ++n) {
                const double v = ev_wave_sum(sp[n]);
                if (lane == 0) s_sim[tid >> 6][n] = v;
            }
        }
    }
    __syncthreads();

    // ---- phase 3: waves 0 and 1 clip the matches, the first threads of wave 2 run the LCS of a reference each
    if (tid < EV_L) {
        int mt[4] = {0, 0, 0, 0};
        if (tid < lh) {
            const unsigned ho = s_ho[tid];
            for (int n = 0; n < 4; ++n) {
                unsigned mx = 0;
                for (int r = 0; r < nr; ++r) mx = max(mx, (s_cr[r][tid] >> (8 * n)) & 255u);   // the max over the references, then the clip
                mt[n] = ((ho >> (8 * n)) & 255u) < mx;
            }
        }
        for (int n = 0; n < 4; ++n) {
            int v = mt[n];
            for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
            if (lane == 0) s_match[tid >> 6][n] = v;
        }
    } else if (tid < EV_L + nr) {
        const int r = tid - EV_L, lr = s_len[r];
        uint64_t v0 = ~0ull, v1 = ~0ull;
        for (int i = 0; i < lh; ++i) {
            const uint64_t u0 = v0 & s_mask[r][i][0], u1 = v1 & s_mask[r][i][1];
            const uint64_t a0 = v0 + u0, a1 = v1 + u1 + (a0 < v0 ? 1ull : 0ull);
            v0 = a0 | (v0 & ~u0);
            v1 = a1 | (v1 & ~u1);
        }
        const uint64_t lo = lr >= 64 ? ~0ull : ((1ull << lr) - 1ull);
        const uint64_t hi = lr <= 64 ? 0ull : (lr >= 128 ? ~0ull : ((1ull << (lr - 64)) - 1ull));
        s_lcs[r] = __popcll(~v0 & lo) + __popcll(~v1 & hi);
    }
    __syncthreads();

    // ---- phase 4: the item's numbers, one thread, the references in ascending order
    if (tid == 0) {
        int closest = s_len[0];
        for (int r = 1; r < nr; ++r) {
            const int l = s_len[r], d = abs(l - lh), dc = abs(closest - lh);
            if (d < dc || (d == dc && l < closest)) closest = l;
        }
        int* st = A.stats + (size_t)o * 10;
        for (int n = 0; n < 4; ++n) {
            st[n] = max(lh - n, 0);
            st[4 + n] = s_match[0][n] + s_match[1][n];
        }
        st[8] = lh;
        st[9] = closest;

        double prec = 0.0, rec = 0.0;
        for (int r = 0; r < nr; ++r) {
            const int lr = s_len[r];
            if (lh > 0) prec = fmax(prec, (double)s_lcs[r] / (double)lh);
            if (lr > 0) rec = fmax(rec, (double)s_lcs[r] / (double)lr);
        }
        const double beta2 = 1.2 * 1.2;
        A.rouge[o] = (prec > 0.0 && rec > 0.0) ? (1.0 + beta2) * prec * rec / (rec + beta2 * prec) : 0.0;

        double total = 0.0;
        for (int n = 0; n < 4; ++n) {
            const double nh = sqrt(s_n2[2 * EV_HYP][n] + s_n2[2 * EV_HYP + 1][n]);
            double acc = 0.0;
            for (int r = 0; r < nr; ++r) {
                const double nrm = sqrt(s_n2[2 * r][n] + s_n2[2 * r + 1][n]);
                double val = s_sim[2 * r][n] + s_sim[2 * r + 1][n];
                if (nh != 0.0 && nrm != 0.0) val = val / (nh * nrm);
                const double d = (double)(lh - s_len[r]);
                acc += val * exp(-(d * d) / 72.0);
            }
            total += acc / (double)nr;
        }
        A.cider[o] = 10.0 * (total / 4.0);
    }
}
