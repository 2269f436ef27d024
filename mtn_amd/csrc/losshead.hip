// losshead.hip — generator log-softmax + label-smoothed KL divergence, fused per row, in its five forms: plain, with teacher soft
// targets (word-level knowledge distillation, Hinton et al. 2015; Kim & Rush 2016), with a signed weight per row (the policy-gradient
// loss of self-critical sequence training), with token-level unlikelihood and with a paired consistency term (R-Drop, Liang et al. 2021).
// include/mtn_hip.h states the contracts of the ten entry points.
//   Generator.forward      : log_softmax(proj(x))                          (mtn.py:62-69)
//   LabelSmoothing.forward : KLDivLoss(sum)(logp, smoothed one-hot)        (label_smoothing.py:20-32)
//   SimpleLossCompute      : sum_i coef_i * KL_i / norm_i                  (data_utils.py:133-144)
// The (rows, vocab) log-probabilities and target distribution are never materialised: with z the logits, lse the row
// log-sum-exp, t the target, eps = smoothing/(V-2), conf = 1-smoothing, td the smoothed target row and scale = coef / norm,
//     KL_ls = sum_j td_j log td_j - sum_j td_j z_j + lse * sum_j td_j
// needs only lse, S = sum_j z_j, z_t and z_pad.
//   plain     rowloss = scale KL_ls                                    dz_j = g scale (softmax_j * sum(td) - td_j)
//   weighted  rowloss = scale w KL_ls at the segment's smoothing       dz_j = g scale w (softmax_j * sum(td) - td_j);  w == 0 zeroes the row
//   distill   rowloss = scale [(1 - alpha) KL_ls + alpha T^2 kd]       dz_j = g scale [(1 - alpha)(softmax_j * sum(td) - td_j) + alpha T (pS_j - pT_j)]
// The soft part needs the dense teacher row q next to z; with T the temperature, a = z / T, b = q / T, m_a / m_b the row maxima of a / b,
//     e_j  = exp(b_j - m_b)                                    (0 where q_j = -inf)
//     kd   = sum_j e_j ((b_j - m_b) - (a_j - m_a)) / sum_j e_j - log sum_j e_j + log sum_j exp(a_j - m_a)
// which is sum_j pT_j (log pT_j - log pS_j) with the two maxima taken out of every term (they cancel exactly; the unshifted sum
// loses log2(|m_b - m_a|) bits to teacher logits with a common offset).  kd = 0 on rows whose target is <pad>; those rows never read q.
// The reference's quirk is kept (label_smoothing.py:29): <pad> rows are zeroed only if the sum of their row indices is
// positive, i.e. a lone <pad> target at flat row 0 keeps td = eps everywhere but the <pad> column.
//   unlikely  rowloss = scale (KL_ls + ul_alpha ul)                    dz_j = g scale [(softmax_j * sum(td) - td_j) + ul_alpha ([j live] r_j - p_j R)]
// Unlikelihood (Welleck et al. 2019): the candidates C of a row are its sequence's earlier targets, as a set, without the row's own target
// and <pad>; ul = sum_C -log(max(1 - p_c, 1e-5)), r_c = p_c / (1 - p_c) on unclamped candidates, R their sum.  The set is a bitmap of V bits
// in the wave's LDS slice (lanes OR the earlier targets in); ul and R come from a walk over its words, the backward sweep tests its own
// columns' bits, so every dlogits element is written once.  Rows without candidates (<pad>, t = 0, seq_len 0) take the plain path.
//   paired    rowloss = scale (KL_ls + rd_alpha J / 4)                 dz_k = g scale [(softmax_k * sum(td) - td_k) + rd_alpha / 2 (p_k (d_k - kl) + p_k - q_k)]
// R-Drop: local rows i and i + N of a paired segment are two passes of one position; p / q their softmaxes, d = log p - log q,
// J = sum_c (p_c - q_c) d_c = KL(p||q) + KL(q||p) (termwise >= 0, no cancellation), kl = sum_c p_c d_c.  Both rows differentiate through their
// own softmax (the partner is no constant teacher).  A wave computes its partner's (max, log-sum-exp) itself with the code that wave runs
// on its own row, and both form the same products in the same column order: the two rowrd of a pair are equal bit for bit.  The forward
// is three sweeps over both rows (the partner's 12 KB are L2-resident), the backward one, with lse of both rows and kl from the forward.
// The forms are instantiations of the same code, so a segment without a teacher (or alpha == 0: the host drops the teacher
// pointers; no (1 - alpha) factor is applied there) and a segment without weights at the loss head's smoothing (the weight is applied by
// a multiplication of its own, which cannot be contracted into anything) give the plain head's lse, rowloss and dlogits bit for bit.
// One 64-lane wave per row, float4 loads (z and q of a sweep issued together), wave-shuffle reductions in a fixed order, no atomics.
// Forward: two sweeps (maxima and S; the sums).  Backward: one sweep; with a teacher one more before it (a running (max, sum-exp) pair
// per lane for lse(b) — and lse(a) when T != 1, else the forward's lse serves).  HBM/L2-bound: 12 KB per row at V = 3000, 24 KB with a teacher
// or a partner (the paired form: a third forward sweep for the divergence).
#include "common.h"

#include <math.h>
#include <type_traits>

template <typename Args> constexpr bool HEAD_DISTILL = std::is_same_v<Args, mtn_distill_args>;
template <typename Args> constexpr bool HEAD_WEIGHTED = std::is_same_v<Args, mtn_wlosshead_args>;
template <typename Args> constexpr bool HEAD_UL = std::is_same_v<Args, mtn_ulosshead_args>;
template <typename Args> constexpr bool HEAD_RD = std::is_same_v<Args, mtn_rlosshead_args>;

struct HeadRow {
    int seg, local;      // segment (stream) and row inside it
    long t;
    float scale;         // coef / norm
    float eps, conf;     // the segment's smoothing
    bool zero_row, t_is_pad;
    bool weighted = false;       // the segment has weights
    float w = 1.0f;
    const float* q = nullptr;    // teacher row; nullptr: this row takes the plain path
    bool kd_seg = false;         // the segment is distilled: its hard part carries (1 - alpha)
    int ul_t = 0;                // unlikelihood: position inside the sequence; 0: this row takes the plain path
    const long* ul_prev = nullptr;   // the sequence's targets y_0 .. y_{t-1}
    int rd_row = -1;             // R-Drop: the partner's flat row; -1: this row takes the plain path
};

template <typename Args>
__device__ __forceinline__ HeadRow head_row(const Args& A, int row, int lane) {
    HeadRow r;
    int base = 0;
    r.seg = 0;
    for (int s = 0; s < A.n_seg; ++s) {
        if (row >= base && row < base + A.rows[s]) { r.seg = s; break; }
        base += A.rows[s];
    }
    r.local = row - base;
    r.t = A.target[r.seg][r.local];
    r.scale = A.coef[r.seg] / *A.norm[r.seg];
    r.t_is_pad = (r.t == A.pad);
    r.zero_row = false;
    if (r.t_is_pad) {
        if (r.local > 0) r.zero_row = true;                 // its own index makes the index sum positive
        else {                                              // flat row 0: zeroed only if another <pad> row exists
            int any = 0;
            for (int i = 1 + lane; i < A.rows[r.seg]; i += 64) any |= (A.target[r.seg][i] == A.pad);
            r.zero_row = __any(any);
        }
    }
    float sm = A.smoothing;
    if constexpr (HEAD_WEIGHTED<Args>) {
        if (A.smoothing_seg[r.seg] >= 0.f) sm = A.smoothing_seg[r.seg];
        r.weighted = A.roww[r.seg] != nullptr;
        r.w = r.weighted ? A.roww[r.seg][r.local] : 1.0f;
        if (r.w == 0.f) r.zero_row = true;                  // +0.0 everywhere, whatever the row holds
    }
    r.eps = sm / (float)(A.V - 2);
    r.conf = 1.0f - sm;
    if constexpr (HEAD_DISTILL<Args>) {
        r.kd_seg = A.teacher[r.seg] != nullptr;
        r.q = (r.kd_seg && !r.t_is_pad) ? A.teacher[r.seg] + (size_t)r.local * A.ldq[r.seg] : nullptr;
    }
    if constexpr (HEAD_UL<Args>) {
        const int T = A.seq_len[r.seg];
        if (T > 0 && !r.t_is_pad) {                         // (<pad> rows, the quirk row included, and t = 0: no candidates)
            r.ul_t = r.local % T;
            r.ul_prev = A.target[r.seg] + (r.local - r.ul_t);
        }
    }
    if constexpr (HEAD_RD<Args>) {
        const int N = A.pair[r.seg];                        // rows[seg] == 2 N (checked on the host): the partner lies inside the segment
        if (N > 0 && !r.t_is_pad) r.rd_row = base + (r.local < N ? r.local + N : r.local - N);
    }
    return r;
}

__device__ __forceinline__ float head_max4(float m, const float4& v) { return fmaxf(fmaxf(m, fmaxf(v.x, v.y)), fmaxf(v.z, v.w)); }

// the two plain sweeps of a wave over its row: returns lse, leaves S = sum_j z_j
__device__ __forceinline__ float head_lse(const float* z, int V, int lane, float& S) {
    float mx = -INFINITY;
    S = 0.f;
    for (int c = lane * 4; c < V; c += 256) {
        float4 v = *(const float4*)(z + c);                 // V % 4 == 0 (checked on the host)
        mx = head_max4(mx, v);
        S += (v.x + v.y) + (v.z + v.w);
    }
    mx = wave_max(mx);
    S = wave_sum(S);
    float se = 0.f;
    for (int c = lane * 4; c < V; c += 256) {
        float4 v = *(const float4*)(z + c);
        se += (__expf(v.x - mx) + __expf(v.y - mx)) + (__expf(v.z - mx) + __expf(v.w - mx));
    }
    return mx + __logf(wave_sum(se));
}

// label-smoothed KL of one live row, unweighted (lane 0)
__device__ __forceinline__ float head_hard_kl(const HeadRow& r, const float* z, int V, int pad, float S, float lse) {
    const float eps = r.eps, conf = r.conf;
    const float zt = z[r.t], zp = z[pad];
    float n_eps, sum_tdz, sum_td, sum_tdlog;
    if (!r.t_is_pad) {
        n_eps = (float)(V - 2);
        sum_tdz = eps * (S - zt - zp) + conf * zt;
        sum_td = n_eps * eps + conf;
        sum_tdlog = (eps > 0.f ? n_eps * eps * __logf(eps) : 0.f) + (conf > 0.f ? conf * __logf(conf) : 0.f);
    } else {
        n_eps = (float)(V - 1);
        sum_tdz = eps * (S - zp);
        sum_td = n_eps * eps;
        sum_tdlog = eps > 0.f ? n_eps * eps * __logf(eps) : 0.f;
    }
    return sum_tdlog - sum_tdz + lse * sum_td;
}

// the backward sweep of a row without soft targets: dz_j = g (softmax_j sum(td) - td_j), columns V..ldd-1 zero-filled
template <typename T>
__device__ __forceinline__ void head_hard_bwd(const HeadRow& r, const float* z, T* dz, int V, int ldd, int pad, float g, float sum_td,
                                              float lse, int lane) {
    for (int c = lane * 4; c < ldd; c += 256) {
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c < V && !r.zero_row) {
            float4 v = *(const float4*)(z + c);
            float* ov = &o.x;
            const float* vv = &v.x;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int j = c + k;
                float td = r.eps;
                if (j == pad) td = 0.f;
                else if (j == r.t) td = r.conf;
                ov[k] = g * (__expf(vv[k] - lse) * sum_td - td);
            }
        }
        store_lp4<T>(dz + c, o);
    }
}

// online4 (common.h) over x * iT; the product stays inside the exponent's argument, where it may contract
__device__ __forceinline__ void head_online4_scaled(float& m, float& s, const float4& v, float iT) {
    const float mn = fmaxf(m, head_max4(-INFINITY, v) * iT);
    if (mn > -INFINITY) {
        s = s * __expf(m - mn) + ((__expf(v.x * iT - mn) + __expf(v.y * iT - mn)) + (__expf(v.z * iT - mn) + __expf(v.w * iT - mn)));
        m = mn;
    }
}
__device__ __forceinline__ float head_wave_lse(float m, float s) {
    online_wave(m, s);
    return m + __logf(s);
}

// Unlikelihood: the candidate set C = { y_0 .. y_{t-1} } \ { y_t, <pad> } of a row as a bitmap of V bits in the wave's own LDS slice.
// LDS operations of one wave complete in issue order; the fence and the wave barrier keep the compiler from moving them.
__device__ __forceinline__ void head_ul_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}
__device__ __forceinline__ unsigned* head_ul_bitmap(const HeadRow& r, int V, int pad, int lane) {
    extern __shared__ __attribute__((aligned(16))) unsigned head_ul_lds[];   // [4 waves][ceil(V / 32)]
    const int words = (V + 31) >> 5;
    unsigned* bits = head_ul_lds + (threadIdx.x >> 6) * words;
    for (int w = lane; w < words; w += 64) bits[w] = 0u;
    head_ul_sync();
    for (int i = lane; i < r.ul_t; i += 64) {
        const long y = r.ul_prev[i];
        if (y >= 0 && y < V && y != r.t && y != pad) atomicOr(&bits[y >> 5], 1u << (y & 31));   // (a set: the order of the ORs is immaterial)
    }
    head_ul_sync();
    return bits;
}
// sum over the candidates of -log(max(1 - p_c, clamp)) (forward) or of r_c = p_c / (1 - p_c) where unclamped (backward): a lane walks its
// words' bits in ascending order, the lanes combine in wave_sum's order — fixed by V and the set alone
template <bool BWD>
__device__ __forceinline__ float head_ul_walk(const unsigned* bits, int V, const float* z, float lse, int lane) {
    const int words = (V + 31) >> 5;
    float acc = 0.f;
    for (int w = lane; w < words; w += 64) {
        unsigned m = bits[w];
        while (m) {
            const int c = (w << 5) + __ffs(m) - 1;
            m &= m - 1;
            const float p = __expf(z[c] - lse);
            const float u = 1.0f - p;
            if constexpr (BWD) {
                if (u >= MTN_UL_CLAMP) acc += p / u;
            } else acc -= __logf(fmaxf(u, MTN_UL_CLAMP));
        }
    }
    return wave_sum(acc);
}

template <typename Args>
__global__ __launch_bounds__(256) void losshead_fwd_kernel(const Args A, int total_rows) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= total_rows) return;
    const HeadRow r = head_row(A, row, lane);
    const float* z = A.logits + (size_t)row * A.ldz;
    const int V = A.V;
    float lse, S, kd = 0.f, ul = 0.f, rd = 0.f, kl = 0.f;
    if (r.q == nullptr && r.rd_row < 0) lse = head_lse(z, V, lane, S);
    else if constexpr (HEAD_RD<Args>) {                      // head_lse's two sweeps on both rows of the pair, then the divergence sweep
        const float* zj = A.logits + (size_t)r.rd_row * A.ldz;
        float mx = -INFINITY, mj = -INFINITY;
        S = 0.f;
        for (int c = lane * 4; c < V; c += 256) {
            const float4 v = *(const float4*)(z + c);
            const float4 u = *(const float4*)(zj + c);
            mx = head_max4(mx, v);
            mj = head_max4(mj, u);
            S += (v.x + v.y) + (v.z + v.w);
        }
        mx = wave_max(mx);
        mj = wave_max(mj);
        S = wave_sum(S);
        float se = 0.f, sj = 0.f;
        for (int c = lane * 4; c < V; c += 256) {
            const float4 v = *(const float4*)(z + c);
            const float4 u = *(const float4*)(zj + c);
            se += (__expf(v.x - mx) + __expf(v.y - mx)) + (__expf(v.z - mx) + __expf(v.w - mx));
            sj += (__expf(u.x - mj) + __expf(u.y - mj)) + (__expf(u.z - mj) + __expf(u.w - mj));
        }
        const float lg = __logf(wave_sum(se)), lgj = __logf(wave_sum(sj));   // the partner's wave computes (mj, lgj) as its own (mx, lg): same bits
        lse = mx + lg;
        float J = 0.f;
        for (int c = lane * 4; c < V; c += 256) {
            const float4 v = *(const float4*)(z + c);
            const float4 u = *(const float4*)(zj + c);
            const float* vv = &v.x;
            const float* uu = &u.x;
            float tj[4], tk[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float lp = (vv[k] - mx) - lg, lq = (uu[k] - mj) - lgj;
                const float p = __expf(lp), q = __expf(lq), d = lp - lq;
                tj[k] = (p - q) * d;                         // >= 0; the partner's wave forms (q - p) * (-d): the same product
                tk[k] = p * d;
            }
            J += (tj[0] + tj[1]) + (tj[2] + tj[3]);
            kl += (tk[0] + tk[1]) + (tk[2] + tk[3]);
        }
        rd = 0.25f * wave_sum(J);
        kl = wave_sum(kl);
    }
    else if constexpr (HEAD_DISTILL<Args>) {
        const float* q = r.q;
        const bool t1 = A.temperature == 1.0f;               // (uniform: a kernel argument)
        const float iT = 1.0f / A.temperature;
        float mx = -INFINITY, mq = -INFINITY;
        S = 0.f;
        for (int c = lane * 4; c < V; c += 256) {
            const float4 v = *(const float4*)(z + c);
            const float4 u = *(const float4*)(q + c);       // ldq % 4 == 0
            mx = head_max4(mx, v);
            mq = head_max4(mq, u);
            S += (v.x + v.y) + (v.z + v.w);
        }
        mx = wave_max(mx);
        mq = wave_max(mq);
        S = wave_sum(S);
        float se = 0.f, sa = 0.f, sb = 0.f, num = 0.f;
        for (int c = lane * 4; c < V; c += 256) {
            const float4 v = *(const float4*)(z + c);
            const float4 u = *(const float4*)(q + c);
            const float* vv = &v.x;
            const float* uu = &u.x;
            float e1[4], ea[4], eb[4], tb[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float dz = vv[k] - mx;                 // <= 0
                const float db = (uu[k] - mq) * iT;          // <= 0, -inf where the teacher excludes the column
                e1[k] = __expf(dz);
                ea[k] = t1 ? e1[k] : __expf(dz * iT);
                eb[k] = __expf(db);
                tb[k] = db > -INFINITY ? eb[k] * (db - dz * iT) : 0.f;      // no 0 * inf
            }
            se += (e1[0] + e1[1]) + (e1[2] + e1[3]);
            if (!t1) sa += (ea[0] + ea[1]) + (ea[2] + ea[3]);
            sb += (eb[0] + eb[1]) + (eb[2] + eb[3]);
            num += (tb[0] + tb[1]) + (tb[2] + tb[3]);
        }
        se = wave_sum(se);
        sb = wave_sum(sb);
        num = wave_sum(num);
        const float lg = __logf(se);
        lse = mx + lg;
        const float lga = t1 ? lg : __logf(wave_sum(sa));
        kd = num / sb - __logf(sb) + lga;
    }
    if constexpr (HEAD_UL<Args>) {
        if (r.ul_t > 0) ul = head_ul_walk<false>(head_ul_bitmap(r, V, A.pad, lane), V, z, lse, lane);
    }
    if (lane == 0) {
        A.lse[row] = lse;
        float loss = 0.f;
        if (!r.zero_row) {                                   // (the KL inside each branch: hoisted, the compiler contracts it otherwise)
            if (!r.kd_seg && r.ul_t == 0 && r.rd_row < 0) loss = head_hard_kl(r, z, V, A.pad, S, lse) * (r.weighted ? r.scale * r.w : r.scale);
            else if constexpr (HEAD_RD<Args>) loss = r.scale * (head_hard_kl(r, z, V, A.pad, S, lse) + A.rd_alpha * rd);
            else if constexpr (HEAD_UL<Args>) loss = r.scale * (head_hard_kl(r, z, V, A.pad, S, lse) + A.ul_alpha * ul);
            else if constexpr (HEAD_DISTILL<Args>)
                loss = r.scale * ((1.0f - A.alpha) * head_hard_kl(r, z, V, A.pad, S, lse) + (A.alpha * A.temperature * A.temperature) * kd);
        }
        A.rowloss[row] = loss;
        if constexpr (HEAD_DISTILL<Args>) {
            if (A.rowkd) A.rowkd[row] = kd;
        }
        if constexpr (HEAD_UL<Args>) {
            if (A.rowul) A.rowul[row] = ul;
        }
        if constexpr (HEAD_RD<Args>) {
            if (A.rowrd) A.rowrd[row] = rd;
            if (A.rowkl) A.rowkl[row] = kl;
        }
    }
}

template <typename T, typename Args>
__global__ __launch_bounds__(256) void losshead_bwd_kernel(const Args A, int total_rows) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= total_rows) return;
    const HeadRow r = head_row(A, row, lane);
    const float* z = A.logits + (size_t)row * A.ldz;
    T* dz = (T*)A.dlogits + (size_t)row * A.ldd;
    const int V = A.V;
    float g = (*A.gloss) * r.scale;
    if (r.weighted) g = g * r.w;
    const float eps = r.eps, conf = r.conf;
    const float sum_td = r.zero_row ? 0.f : (r.t_is_pad ? (float)(V - 1) * eps : (float)(V - 2) * eps + conf);
    const float lse = A.lse[row];
    if (!r.kd_seg && r.ul_t == 0 && r.rd_row < 0) head_hard_bwd<T>(r, z, dz, V, A.ldd, A.pad, g, sum_td, lse, lane);
    else if constexpr (HEAD_RD<Args>) {                      // (a paired row is live: never a zeroed row)
        const float* zj = A.logits + (size_t)r.rd_row * A.ldz;
        const float lsj = A.lse[r.rd_row], kl = A.rowkl[row], h = 0.5f * A.rd_alpha;
        for (int c = lane * 4; c < A.ldd; c += 256) {
            float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
            if (c < V) {
                const float4 v = *(const float4*)(z + c);
                const float4 u = *(const float4*)(zj + c);
                float* ov = &o.x;
                const float* vv = &v.x;
                const float* uu = &u.x;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int j = c + k;
                    float td = eps;
                    if (j == A.pad) td = 0.f;
                    else if (j == r.t) td = conf;
                    const float lp = vv[k] - lse, lq = uu[k] - lsj;
                    const float p = __expf(lp), q = __expf(lq);
                    ov[k] = g * ((p * sum_td - td) + h * (p * ((lp - lq) - kl) + (p - q)));
                }
            }
            store_lp4<T>(dz + c, o);
        }
    }
    else if constexpr (HEAD_UL<Args>) {                      // (a row with candidates is live: never a zeroed row)
        const unsigned* bits = head_ul_bitmap(r, V, A.pad, lane);
        const float R = head_ul_walk<true>(bits, V, z, lse, lane);
        const float ua = A.ul_alpha;
        for (int c = lane * 4; c < A.ldd; c += 256) {
            float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
            if (c < V) {
                const float4 v = *(const float4*)(z + c);
                const unsigned m = bits[c >> 5] >> (c & 31);    // the sweep tests its own columns' bits: every element is written once
                float* ov = &o.x;
                const float* vv = &v.x;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int j = c + k;
                    float td = eps;
                    if (j == A.pad) td = 0.f;
                    else if (j == r.t) td = conf;
                    const float p = __expf(vv[k] - lse);
                    const float u = 1.0f - p;
                    float e = -(p * R);
                    if (((m >> k) & 1u) && u >= MTN_UL_CLAMP) e += p / u;
                    ov[k] = g * ((p * sum_td - td) + ua * e);
                }
            }
            store_lp4<T>(dz + c, o);
        }
    }
    else if constexpr (HEAD_DISTILL<Args>) {
        const float* q = r.q;
        const float wh = 1.0f - A.alpha, ws = A.alpha * A.temperature;
        const bool t1 = A.temperature == 1.0f;
        const float iT = 1.0f / A.temperature;
        float lsa = lse, lsb = 0.f;
        if (q != nullptr) {
            float ma = -INFINITY, sa = 0.f, mb = -INFINITY, sb = 0.f;
            for (int c = lane * 4; c < V; c += 256) {
                const float4 u = *(const float4*)(q + c);
                if (!t1) {
                    const float4 v = *(const float4*)(z + c);
                    head_online4_scaled(ma, sa, v, iT);
                }
                head_online4_scaled(mb, sb, u, iT);
            }
            lsb = head_wave_lse(mb, sb);
            if (!t1) lsa = head_wave_lse(ma, sa);
        }
        for (int c = lane * 4; c < A.ldd; c += 256) {
            float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
            if (c < V && !r.zero_row) {
                const float4 v = *(const float4*)(z + c);
                float4 u = make_float4(0.f, 0.f, 0.f, 0.f);
                if (q != nullptr) u = *(const float4*)(q + c);
                float* ov = &o.x;
                const float* vv = &v.x;
                const float* uu = &u.x;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int j = c + k;
                    float td = eps;
                    if (j == A.pad) td = 0.f;
                    else if (j == r.t) td = conf;
                    float d = wh * (__expf(vv[k] - lse) * sum_td - td);
                    if (q != nullptr) d += ws * (__expf(vv[k] * iT - lsa) - __expf(uu[k] * iT - lsb));
                    ov[k] = g * d;
                }
            }
            store_lp4<T>(dz + c, o);
        }
    }
}

// the arguments every form refuses, then the form's own fields; `D` = the arguments the kernels get (alpha == 0 drops the teachers)
template <typename Args>
static int head_check(const char* fn, const Args* A, bool bwd, int dtype, Args* D, int* total) {
#define HEAD_CHECK(cond, msg) do { if (!(cond)) { mtn_set_error("%s: %s", fn, msg); return MTN_ERR_ARG; } } while (0)
    HEAD_CHECK(!bwd || dtype == MTN_F32 || dtype == MTN_BF16, "bad dtype");
    HEAD_CHECK(A && A->n_seg >= 1 && A->n_seg <= MTN_LOSSHEAD_MAX_SEG, "bad segment count");
    HEAD_CHECK(A->V >= 4 && A->V % 4 == 0 && A->ldz % 4 == 0 && A->ldz >= A->V, "V and ldz must be multiples of 4, ldz >= V >= 4");
    HEAD_CHECK(!bwd || (A->ldd % 4 == 0 && A->ldd >= A->V), "ldd must be a multiple of 4, ldd >= V");
    HEAD_CHECK(A->pad >= 0 && A->pad < A->V, "pad outside [0, V)");
    HEAD_CHECK(A->logits && A->lse && (bwd ? (A->gloss && A->dlogits) : A->rowloss != nullptr), "null buffer");
    if constexpr (HEAD_DISTILL<Args>) {
        HEAD_CHECK(isfinite(A->alpha) && A->alpha >= 0.f && A->alpha <= 1.f, "alpha outside [0, 1]");
        HEAD_CHECK(isfinite(A->temperature) && A->temperature > 0.f, "temperature must be finite and > 0");
    }
    if constexpr (HEAD_UL<Args>) {
        HEAD_CHECK(isfinite(A->ul_alpha) && A->ul_alpha >= 0.f, "ul_alpha must be finite and >= 0");
        HEAD_CHECK(A->V <= MTN_ULOSSHEAD_MAX_V, "V above MTN_ULOSSHEAD_MAX_V");
    }
    if constexpr (HEAD_RD<Args>) HEAD_CHECK(isfinite(A->rd_alpha) && A->rd_alpha >= 0.f, "rd_alpha must be finite and >= 0");
    *D = *A;
    *total = 0;
    for (int s = 0; s < A->n_seg; ++s) {
        HEAD_CHECK(A->rows[s] > 0 && A->target[s] && A->norm[s], "bad segment");
        if constexpr (HEAD_DISTILL<Args>) {
            HEAD_CHECK(!A->teacher[s] || (A->ldq[s] >= A->V && A->ldq[s] % 4 == 0), "ldq must be a multiple of 4, ldq >= V");
            HEAD_CHECK(((uintptr_t)A->teacher[s] & 15) == 0, "teacher rows must be 16-byte aligned");
        }
        if constexpr (HEAD_WEIGHTED<Args>) {
            HEAD_CHECK(((uintptr_t)A->roww[s] & 3) == 0, "row weights must be 4-byte aligned");
            HEAD_CHECK(!isnan(A->smoothing_seg[s]), "smoothing_seg is NaN");
        }
        if constexpr (HEAD_UL<Args>) {
            HEAD_CHECK(A->seq_len[s] >= 0, "seq_len < 0");
            HEAD_CHECK(A->seq_len[s] == 0 || A->rows[s] % A->seq_len[s] == 0, "rows must be a multiple of seq_len");
        }
        if constexpr (HEAD_RD<Args>) {
            HEAD_CHECK(A->pair[s] >= 0, "pair < 0");
            HEAD_CHECK(A->pair[s] == 0 || (A->rows[s] % 2 == 0 && A->rows[s] / 2 == A->pair[s]), "a paired segment holds 2 * pair rows");
            HEAD_CHECK(A->pair[s] == 0 || A->rd_alpha == 0.f || A->rowkl, "a paired segment needs rowkl");
        }
        *total += A->rows[s];
    }
#undef HEAD_CHECK
    if constexpr (HEAD_DISTILL<Args>) {
        for (int s = 0; s < MTN_LOSSHEAD_MAX_SEG; ++s)      // never read: the plain arithmetic, no (1 - alpha) factor
            if (s >= A->n_seg || A->alpha == 0.f) D->teacher[s] = nullptr;
    }
    if constexpr (HEAD_UL<Args>) {
        for (int s = 0; s < MTN_LOSSHEAD_MAX_SEG; ++s)      // seq_len 0: the plain arithmetic, no bitmap
            if (s >= A->n_seg || A->ul_alpha == 0.f) D->seq_len[s] = 0;
    }
    if constexpr (HEAD_RD<Args>) {
        for (int s = 0; s < MTN_LOSSHEAD_MAX_SEG; ++s)      // pair 0: the plain arithmetic, no partner read
            if (s >= A->n_seg || A->rd_alpha == 0.f) D->pair[s] = 0;
    }
    return MTN_OK;
}

// dynamic LDS of a launch: the unlikelihood bitmaps, one of V bits per wave, when any segment has candidates
template <typename Args>
static size_t head_lds(const Args& D) {
    if constexpr (HEAD_UL<Args>) {
        for (int s = 0; s < D.n_seg; ++s)
            if (D.seq_len[s] > 0) return (size_t)4 * ((D.V + 31) / 32) * sizeof(unsigned);
    }
    return 0;
}

static int head_launched(const char* fn) {
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return MTN_OK;
    mtn_set_error("%s: launch failed: %s", fn, hipGetErrorString(e));
    return MTN_ERR_LAUNCH;
}

template <typename Args>
static int head_fwd(const char* fn, const Args* A, void* stream) {
    Args D;
    int total = 0;
    const int rc = head_check(fn, A, false, 0, &D, &total);
    if (rc != MTN_OK) return rc;
    hipLaunchKernelGGL(losshead_fwd_kernel<Args>, dim3((total + 3) / 4), dim3(256), head_lds(D), (hipStream_t)stream, D, total);
    return head_launched(fn);
}

template <typename Args>
static int head_bwd(const char* fn, int dtype, const Args* A, void* stream) {
    Args D;
    int total = 0;
    const int rc = head_check(fn, A, true, dtype, &D, &total);
    if (rc != MTN_OK) return rc;
    const hipStream_t st = (hipStream_t)stream;
    if (dtype == MTN_BF16) hipLaunchKernelGGL((losshead_bwd_kernel<bf16_t, Args>), dim3((total + 3) / 4), dim3(256), head_lds(D), st, D, total);
    else hipLaunchKernelGGL((losshead_bwd_kernel<float, Args>), dim3((total + 3) / 4), dim3(256), head_lds(D), st, D, total);
    return head_launched(fn);
}

extern "C" int mtn_losshead_fwd(const mtn_losshead_args* A, void* stream) { return head_fwd(__func__, A, stream); }
extern "C" int mtn_losshead_bwd(int dtype, const mtn_losshead_args* A, void* stream) { return head_bwd(__func__, dtype, A, stream); }
extern "C" int mtn_distill_fwd(const mtn_distill_args* A, void* stream) { return head_fwd(__func__, A, stream); }
extern "C" int mtn_distill_bwd(int dtype, const mtn_distill_args* A, void* stream) { return head_bwd(__func__, dtype, A, stream); }
extern "C" int mtn_wlosshead_fwd(const mtn_wlosshead_args* A, void* stream) { return head_fwd(__func__, A, stream); }
extern "C" int mtn_wlosshead_bwd(int dtype, const mtn_wlosshead_args* A, void* stream) { return head_bwd(__func__, dtype, A, stream); }
extern "C" int mtn_ulosshead_fwd(const mtn_ulosshead_args* A, void* stream) { return head_fwd(__func__, A, stream); }
extern "C" int mtn_ulosshead_bwd(int dtype, const mtn_ulosshead_args* A, void* stream) { return head_bwd(__func__, dtype, A, stream); }
extern "C" int mtn_rlosshead_fwd(const mtn_rlosshead_args* A, void* stream) { return head_fwd(__func__, A, stream); }
extern "C" int mtn_rlosshead_bwd(int dtype, const mtn_rlosshead_args* A, void* stream) { return head_bwd(__func__, dtype, A, stream); }
