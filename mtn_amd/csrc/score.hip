// score.hip — candidate scoring on the device: per target position the log-probability and the rank of the target under a row of
// logits, per sequence their sum — what a teacher-forced pass needs to say how likely the model finds a GIVEN response, without the
// (rows, V) log-probabilities ever existing (losshead.hip does the same for the training loss).  Definitions (include/mtn_hip.h
// restates them; tests/score_refs.py is their float64 form), with z the row of position (s, l) and t = target[s][l]:
//   tok_logp  z[t] - (max z + log sum exp(z - max z))                     fp32, 0 at a <pad> position
//   tok_rank  #{c : z[c] > z[t]} + #{c < t : z[c] == z[t]}                0 = the target is the arg-max (mtn_topk_rows' tie order)
//   seq_logp  the sequence's tok_logp summed in ascending position in float64 by ONE lane: the same bits in every run
//   seq_len   its counted positions
// A target outside [0, V) counts as <pad>, so no row is indexed out of bounds; columns V..ldz-1 are never read.
// One workgroup per sequence, one 64-lane wave per position (SCORE_WAVES positions per round), z[t] read first, then ONE pass over the
// row with float4 loads that carries a running (max, sum-exp) per lane and the two rank counts; lanes are combined by wave shuffles.
// A row is aligned to 16 bytes by peeling its first 0..3 columns, so any V / ldz works.  HBM/L2-bound (12 KB per position at V = 3000).
#include "common.h"

static constexpr int SCORE_WAVES = 8;

__device__ __forceinline__ int score_wave_isum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(SCORE_WAVES * 64) void score_rows_kernel(const mtn_score_args A) {
    __shared__ float s_lp[2][SCORE_WAVES];
    __shared__ int s_cnt[2][SCORE_WAVES];
    const int seq = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, V = A.V, L = A.L;
    double acc = 0.0;                                          // (thread 0's: the sequence's sum, in position order)
    int n_counted = 0;
    int round = 0;
    for (int base = 0; base < L; base += SCORE_WAVES, ++round) {
        const int l = base + wave;
        float lp = 0.f;
        int counted = 0;
        if (l < L) {                                           // (wave-uniform)
            const size_t at = (size_t)seq * L + l;
            const long t = A.target[at];
            int rank = -1;
            if (t != (long)A.pad && t >= 0 && t < (long)V) {
                const float* z = A.logits + at * (size_t)A.ldz;
                const float zt = z[t];
                const int ti = (int)t;
                float m = -INFINITY, s = 0.f;
                int above = 0;
                auto count = [&](float x, int c) { above += (x > zt || (x == zt && c < ti)) ? 1 : 0; };
                // columns [0, head) bring the row to a 16-byte boundary, [head, body_end) go four at a time, the rest one by one
                const int head = min(V, (int)((4 - (((uintptr_t)z >> 2) & 3)) & 3));
                const int body_end = head + ((V - head) & ~3);
                if (lane < head) { const float x = z[lane]; online1(m, s, x); count(x, lane); }
                for (int c = head + lane * 4; c < body_end; c += 256) {
                    const float4 v = *(const float4*)(z + c);
                    online4(m, s, v);
                    count(v.x, c); count(v.y, c + 1); count(v.z, c + 2); count(v.w, c + 3);
                }
                if (body_end + lane < V) { const float x = z[body_end + lane]; online1(m, s, x); count(x, body_end + lane); }
                online_wave(m, s);
                rank = score_wave_isum(above);
                lp = (zt - m) - logf(s);
                counted = 1;
            }
            if (lane == 0) { A.tok_logp[at] = lp; A.tok_rank[at] = rank; }
        }
        // the round's values in position order through LDS; two slot sets used alternately: one barrier per round
        if (lane == 0) { s_lp[round & 1][wave] = lp; s_cnt[round & 1][wave] = counted; }
        __syncthreads();
        if (threadIdx.x == 0) {
            const int n = min(SCORE_WAVES, L - base);
            for (int w = 0; w < n; ++w) { acc += (double)s_lp[round & 1][w]; n_counted += s_cnt[round & 1][w]; }
        }
    }
    if (threadIdx.x == 0) { A.seq_logp[seq] = acc; A.seq_len[seq] = n_counted; }
}

extern "C" int mtn_score_rows(const mtn_score_args* a, void* stream) {
    MTN_CHECK_ARG(a && a->logits && a->target && a->tok_logp && a->tok_rank && a->seq_logp && a->seq_len, "null buffer");
    MTN_CHECK_ARG(a->V >= 2 && a->V < (1 << 24), "2 <= V < 2^24");
    MTN_CHECK_ARG(a->ldz >= a->V, "ldz >= V");
    MTN_CHECK_ARG(a->L >= 1 && a->n_seq >= 1, "n_seq >= 1, L >= 1");
    hipLaunchKernelGGL(score_rows_kernel, dim3(a->n_seq), dim3(SCORE_WAVES * 64), 0, (hipStream_t)stream, *a);
    MTN_CHECK_LAUNCH();
    return MTN_OK;
}
