// distill.hip — the loss head with teacher soft targets (word-level knowledge distillation, Hinton et al. 2015; Kim & Rush 2016).
// The hard part is losshead.hip's: label-smoothed KL in closed form from lse, S = sum_j z_j, z_t and z_pad.  The soft part needs the dense
// teacher row q next to the student row z; with T the temperature, a = z / T, b = q / T, m_a / m_b the row maxima of a / b,
//     e_j  = exp(b_j - m_b)                                    (0 where q_j = -inf)
//     kd   = sum_j e_j ((b_j - m_b) - (a_j - m_a)) / sum_j e_j - log sum_j e_j + log sum_j exp(a_j - m_a)
// which is sum_j pT_j (log pT_j - log pS_j) with the two maxima taken out of every term (they cancel exactly; the unshifted sum
// loses log2(|m_b - m_a|) bits to teacher logits with a common offset).  kd = 0 on rows whose target is <pad>; those rows never read q.
//     rowloss = scale [(1 - alpha) KL_ls + alpha T^2 kd]
//     dz_j    = g scale [(1 - alpha)(softmax_j(z) sum(td) - td_j) + alpha T (pS_j - pT_j)]
// A segment without a teacher (or alpha == 0: the host drops the teacher pointers) runs losshead.hip's arithmetic, statement for
// statement — no (1 - alpha) factor is applied there — so lse, rowloss and dlogits are those of mtn_losshead_fwd / _bwd bit for bit.
// One 64-lane wave per row, float4 loads, z and q of a sweep issued together, wave-shuffle reductions in a fixed order, no atomics.
// Forward: two sweeps (maxima and S; the sums).  Backward: two sweeps (a running (max, sum-exp) pair per lane for lse(b) — and lse(a)
// when T != 1, else the forward's lse serves; the gradient).  L2/HBM-bound: 24 KB per row at V = 3000 with a teacher.
#include "common.h"

#include <math.h>

struct DistRow {
    int seg, local;      // segment (stream) and row inside it
    long t;
    float scale;         // coef / norm
    bool zero_row, t_is_pad;
    const float* q;      // teacher row; nullptr: this row takes the loss head's path
    bool kd_seg;         // the segment is distilled: its hard part carries (1 - alpha)
};

__device__ __forceinline__ DistRow dist_row_info(const mtn_distill_args& A, int row, int lane) {
    DistRow r;
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
    r.kd_seg = A.teacher[r.seg] != nullptr;
    r.q = (r.kd_seg && !r.t_is_pad) ? A.teacher[r.seg] + (size_t)r.local * A.ldq[r.seg] : nullptr;
    return r;
}

// label-smoothed KL of one live row, unweighted (losshead.hip, lane 0)
__device__ __forceinline__ float dist_hard_kl(const mtn_distill_args& A, const DistRow& r, const float* z, float S, float lse) {
    const int V = A.V;
    const float eps = A.smoothing / (float)(V - 2), conf = 1.0f - A.smoothing;
    const float zt = z[r.t], zp = z[A.pad];
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

__device__ __forceinline__ float dist_max4(float m, const float4& v) { return fmaxf(fmaxf(m, fmaxf(v.x, v.y)), fmaxf(v.z, v.w)); }

__global__ __launch_bounds__(256) void distill_fwd_kernel(const mtn_distill_args A, int total_rows) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= total_rows) return;
    const DistRow r = dist_row_info(A, row, lane);
    const float* z = A.logits + (size_t)row * A.ldz;
    const float* q = r.q;
    const int V = A.V;
    float lse, S, kd = 0.f;
    if (q == nullptr) {                                      // the loss head's two sweeps
        float mx = -INFINITY;
        S = 0.f;
        for (int c = lane * 4; c < V; c += 256) {
            float4 v = *(const float4*)(z + c);             // V % 4 == 0 (checked on the host)
            mx = fmaxf(fmaxf(mx, fmaxf(v.x, v.y)), fmaxf(v.z, v.w));
            S += (v.x + v.y) + (v.z + v.w);
        }
        mx = wave_max(mx);
        S = wave_sum(S);
        float se = 0.f;
        for (int c = lane * 4; c < V; c += 256) {
            float4 v = *(const float4*)(z + c);
            se += (__expf(v.x - mx) + __expf(v.y - mx)) + (__expf(v.z - mx) + __expf(v.w - mx));
        }
        lse = mx + __logf(wave_sum(se));
    } else {
        const bool t1 = A.temperature == 1.0f;               // (uniform: a kernel argument)
        const float iT = 1.0f / A.temperature;
        float mx = -INFINITY, mq = -INFINITY;
        S = 0.f;
        for (int c = lane * 4; c < V; c += 256) {
            const float4 v = *(const float4*)(z + c);
            const float4 u = *(const float4*)(q + c);       // ldq % 4 == 0
            mx = dist_max4(mx, v);
            mq = dist_max4(mq, u);
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
    if (lane == 0) {
        A.lse[row] = lse;
        float loss = 0.f;
        if (!r.zero_row) {
            if (!r.kd_seg) loss = dist_hard_kl(A, r, z, S, lse) * r.scale;
            else loss = r.scale * ((1.0f - A.alpha) * dist_hard_kl(A, r, z, S, lse) + (A.alpha * A.temperature * A.temperature) * kd);
        }
        A.rowloss[row] = loss;
        if (A.rowkd) A.rowkd[row] = kd;
    }
}

// running (max, sum of exp) of a lane over x * iT, -inf entries contribute nothing
__device__ __forceinline__ void dist_online4(float& m, float& s, const float4& v, float iT) {
    const float mn = fmaxf(m, dist_max4(-INFINITY, v) * iT);
    if (mn > -INFINITY) {
        s = s * __expf(m - mn) + ((__expf(v.x * iT - mn) + __expf(v.y * iT - mn)) + (__expf(v.z * iT - mn) + __expf(v.w * iT - mn)));
        m = mn;
    }
}
__device__ __forceinline__ float dist_wave_lse(float m, float s) {
    const float M = wave_max(m);
    return M + __logf(wave_sum(m > -INFINITY ? s * __expf(m - M) : 0.f));
}

template <typename T>
__global__ __launch_bounds__(256) void distill_bwd_kernel(const mtn_distill_args A, int total_rows) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= total_rows) return;
    const DistRow r = dist_row_info(A, row, lane);
    const float* z = A.logits + (size_t)row * A.ldz;
    const float* q = r.q;
    T* dz = (T*)A.dlogits + (size_t)row * A.ldd;
    const int V = A.V;
    const float g = (*A.gloss) * r.scale;
    const float eps = A.smoothing / (float)(V - 2), conf = 1.0f - A.smoothing;
    const float sum_td = r.zero_row ? 0.f : (r.t_is_pad ? (float)(V - 1) * eps : (float)(V - 2) * eps + conf);
    const float lse = A.lse[row];
    if (!r.kd_seg) {                                         // the loss head's sweep
        for (int c = lane * 4; c < A.ldd; c += 256) {
            float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
            if (c < V && !r.zero_row) {
                float4 v = *(const float4*)(z + c);
                float* ov = &o.x;
                const float* vv = &v.x;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int j = c + k;
                    float td = eps;
                    if (j == A.pad) td = 0.f;
                    else if (j == r.t) td = conf;
                    ov[k] = g * (__expf(vv[k] - lse) * sum_td - td);
                }
            }
            store_lp4<T>(dz + c, o);
        }
        return;
    }
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
                dist_online4(ma, sa, v, iT);
            }
            dist_online4(mb, sb, u, iT);
        }
        lsb = dist_wave_lse(mb, sb);
        if (!t1) lsa = dist_wave_lse(ma, sa);
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

// everything mtn_losshead_fwd / _bwd refuse, then the distillation fields; `D` = the arguments the kernels get (alpha == 0 drops the teachers)
static int distill_check(const char* fn, const mtn_distill_args* A, bool bwd, int dtype, mtn_distill_args* D, int* total) {
#define DIST_CHECK(cond, msg) do { if (!(cond)) { mtn_set_error("%s: %s", fn, msg); return MTN_ERR_ARG; } } while (0)
    DIST_CHECK(!bwd || dtype == MTN_F32 || dtype == MTN_BF16, "bad dtype");
    DIST_CHECK(A && A->n_seg >= 1 && A->n_seg <= MTN_LOSSHEAD_MAX_SEG, "bad segment count");
    DIST_CHECK(A->V >= 4 && A->V % 4 == 0 && A->ldz % 4 == 0 && A->ldz >= A->V, "V and ldz must be multiples of 4, ldz >= V >= 4");
    DIST_CHECK(!bwd || (A->ldd % 4 == 0 && A->ldd >= A->V), "ldd must be a multiple of 4, ldd >= V");
    DIST_CHECK(A->pad >= 0 && A->pad < A->V, "pad outside [0, V)");
    DIST_CHECK(A->logits && A->lse && (bwd ? (A->gloss && A->dlogits) : A->rowloss != nullptr), "null buffer");
    DIST_CHECK(isfinite(A->alpha) && A->alpha >= 0.f && A->alpha <= 1.f, "alpha outside [0, 1]");
    DIST_CHECK(isfinite(A->temperature) && A->temperature > 0.f, "temperature must be finite and > 0");
    *D = *A;
    *total = 0;
    for (int s = 0; s < MTN_LOSSHEAD_MAX_SEG; ++s) {
        if (s >= A->n_seg) { D->teacher[s] = nullptr; continue; }
        DIST_CHECK(A->rows[s] > 0 && A->target[s] && A->norm[s], "bad segment");
        DIST_CHECK(!A->teacher[s] || (A->ldq[s] >= A->V && A->ldq[s] % 4 == 0), "ldq must be a multiple of 4, ldq >= V");
        DIST_CHECK(((uintptr_t)A->teacher[s] & 15) == 0, "teacher rows must be 16-byte aligned");
        if (A->alpha == 0.f) D->teacher[s] = nullptr;       // never read: the loss head's arithmetic, no (1 - alpha) factor
        *total += A->rows[s];
    }
#undef DIST_CHECK
    return MTN_OK;
}

extern "C" int mtn_distill_fwd(const mtn_distill_args* A, void* stream) {
    mtn_distill_args D;
    int total = 0;
    const int rc = distill_check(__func__, A, false, 0, &D, &total);
    if (rc != MTN_OK) return rc;
    hipLaunchKernelGGL(distill_fwd_kernel, dim3((total + 3) / 4), dim3(256), 0, (hipStream_t)stream, D, total);
    MTN_CHECK_LAUNCH();
    return MTN_OK;
}

extern "C" int mtn_distill_bwd(int dtype, const mtn_distill_args* A, void* stream) {
    mtn_distill_args D;
    int total = 0;
    const int rc = distill_check(__func__, A, true, dtype, &D, &total);
    if (rc != MTN_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (dtype == MTN_BF16) hipLaunchKernelGGL((distill_bwd_kernel<bf16_t>), dim3((total + 3) / 4), dim3(256), 0, st, D, total);
    else hipLaunchKernelGGL((distill_bwd_kernel<float>), dim3((total + 3) / 4), dim3(256), 0, st, D, total);
    MTN_CHECK_LAUNCH();
    return MTN_OK;
}
