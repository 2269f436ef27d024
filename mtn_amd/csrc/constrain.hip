// constrain.hip — constrained decoding on the device: one workgroup rewrites a row of log-probabilities from the row's own history
// BEFORE the selection launch reads it (select.hip topk_rows for beam / greedy, sample.hip for sampling), so that a constrained
// search stays one captured graph.  Definitions (include/mtn_hip.h restates them; tests/constrain_refs.py is their numpy form):
//   history  h[0..n-1], the tokens the row's hypothesis has generated (no <sos>), from an explicit table or from the step log that
//            mtn_beam_advance / mtn_sample_rows write: position by position from the newest back, following the logged parents;
//   penalty  every DISTINCT token c of h: out[c] = logp[c] * theta — one fp32 multiply, once per token however often it occurs;
//   n-gram   every j with h[j .. j+N-2] == h[n-N+1 .. n-1] bans the token that followed: out[h[j+N-1]] = -inf (N = 1: every token of
//            h); a ban overrides the penalty;
//   rest     copied bit for bit (nothing is touched at all when out is logp).
// Phase A stages the log one chunk of CON_CHUNK positions at a time (all threads load a dialogue's `width` parents and tokens of each
// position: one round of independent loads), then one thread walks the chunk in LDS: the chain of parents is a chain of LDS reads, not
// of global ones.  Phase B gives every history position to one thread: the FIRST occurrence of a token applies the penalty (so the
// multiply happens once and no two threads write one column), a barrier, then the matching positions write their bans.  Several
// matching positions may be followed by the same token and then store to one column — all of them the same value, -inf, so the
// result does not depend on which store lands last.  No atomics.  The first-occurrence scan reads up to j earlier positions for
// position j: O(n^2 / CON_THREADS) LDS reads per row, a few dozen at the n of about 30 that answers reach and at most about 2 600 per
// thread at n = CON_MAX_L — still far below one row's pass through the model, which is why the bound L <= 1024 needs no other scan.
#include "common.h"

static constexpr int CON_THREADS = 256;
static constexpr int CON_MAX_L = 1024;                        // history positions (the persistent decode step's longest search)
static constexpr int CON_MAX_W = 16;                          // hypotheses per dialogue (mtn_beam_advance's width)
static constexpr int CON_CHUNK = 128;                         // positions of the step log staged per round

struct ConstrainArgs { mtn_constrain_args a; };

__global__ __launch_bounds__(CON_THREADS) void constrain_rows_kernel(const ConstrainArgs CA) {
    const mtn_constrain_args& A = CA.a;
    __shared__ int s_h[CON_MAX_L];
    __shared__ int s_tok[CON_CHUNK * CON_MAX_W];
    __shared__ unsigned char s_par[CON_CHUNK * CON_MAX_W];
    __shared__ int s_r;
    const int row = blockIdx.x, tid = threadIdx.x, V = A.V, N = A.ngram;
    const float* xr = A.logp + (size_t)row * A.ldx;
    float* orow = A.out + (size_t)row * A.ldo;

    // out of place: the whole row first (16-byte loads where both rows are aligned), the few constrained columns over it below
    if (orow != xr) {
        const bool aligned = ((((uintptr_t)xr) | ((uintptr_t)orow)) & 15) == 0;
        const int V4 = aligned ? V / 4 : 0;
        for (int i = tid; i < V4; i += CON_THREADS) ((float4*)orow)[i] = ((const float4*)xr)[i];
        for (int c = V4 * 4 + tid; c < V; c += CON_THREADS) orow[c] = xr[c];
    }

    // ---- phase A: h[0..n-1] in LDS
    int n;
    if (A.hist) {
        n = min(max(A.hist_len[row], 0), A.L);                // (the host checked L <= ldh)
        for (int j = tid; j < n; j += CON_THREADS) s_h[j] = A.hist[(size_t)row * A.ldh + j];
    } else {
        const int Wd = A.width, base = row - row % Wd;        // (rows is a multiple of width: base + i < rows)
        n = min(max(A.step[row / A.rows_per_step], 0), A.L);
        if (tid == 0) s_r = row - base;
        for (int hi = n; hi > 0; hi -= CON_CHUNK) {
            const int lo = max(0, hi - CON_CHUNK), cnt = (hi - lo) * Wd;
            for (int e = tid; e < cnt; e += CON_THREADS) {
                const int j = lo + e / Wd, i = e % Wd;
                const size_t at = (size_t)j * A.rows + base + i;
                s_tok[e] = A.log_tok[at];
                const int p = A.log_parent ? A.log_parent[at] : i;           // (rows past the live count hold stale values: clamped)
                s_par[e] = (unsigned char)min(max(p, 0), Wd - 1);
            }
            __syncthreads();
            if (tid == 0) {
                int r = s_r;
                for (int j = hi - 1; j >= lo; --j) {
                    const int e = (j - lo) * Wd + r;
                    s_h[j] = s_tok[e];
                    r = s_par[e];
                }
                s_r = r;
            }
            __syncthreads();                                  // (s_tok / s_par are rewritten next round)
        }
    }
    __syncthreads();                                          // h is complete, and so is the copy of the row

    // ---- phase B: penalty by the first occurrence of every token, then the bans over it
    if (A.theta != 1.f) {
        for (int j = tid; j < n; j += CON_THREADS) {
            const int c = s_h[j];
            if (c < 0 || c >= V) continue;
            bool first = true;
            for (int q = 0; q < j; ++q) first = first && (s_h[q] != c);
            if (first) orow[c] = xr[c] * A.theta;
        }
    }
    __syncthreads();
    if (N >= 1) {
        for (int j = tid; j + N <= n; j += CON_THREADS) {
            bool match = true;
            for (int q = 0; q + 1 < N; ++q) match = match && (s_h[j + q] == s_h[n - N + 1 + q]);
            const int c = s_h[j + N - 1];
            if (match && c >= 0 && c < V) orow[c] = -INFINITY;
        }
    }
}

extern "C" int mtn_constrain_rows(const mtn_constrain_args* a, void* stream) {
    MTN_CHECK_ARG(a && a->logp && a->out, "null buffer");
    MTN_CHECK_ARG(a->rows > 0 && a->V > 0 && a->V < (1 << 24) && a->ldx >= a->V && a->ldo >= a->V, "bad row matrix");
    MTN_CHECK_ARG(a->ngram >= 0 && a->ngram <= 8 && a->theta >= 1.f, "0 <= ngram <= 8, theta >= 1");
    MTN_CHECK_ARG(a->L >= 1 && a->L <= CON_MAX_L, "1 <= L <= 1024");
    if (a->hist) {
        MTN_CHECK_ARG(a->hist_len && a->ldh >= a->L, "explicit history: hist_len, ldh >= L");
    } else {
        MTN_CHECK_ARG(a->log_tok && a->step, "step-log history: log_tok and step");
        MTN_CHECK_ARG(a->width >= 1 && a->width <= CON_MAX_W && a->rows % a->width == 0 && a->rows_per_step >= 1,
                      "step-log history: 1 <= width <= 16, rows a multiple of width, rows_per_step >= 1");
    }
    ConstrainArgs CA; CA.a = *a;
    hipLaunchKernelGGL(constrain_rows_kernel, dim3(a->rows), dim3(CON_THREADS), 0, (hipStream_t)stream, CA);
    MTN_CHECK_LAUNCH();
    return MTN_OK;
}
