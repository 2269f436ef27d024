/*
 * mtn_hip.h — C ABI of libmtn_hip.so: MI355X (gfx950) kernels for the MTN transformer hot path.
 *
 * The reference (henryhungle/MTN) has no FFI: its operator boundary is the Python nn.Module call
 * surface in mtn.py.  Each entry point below replaces the op sequence of one reference operator
 * (file:line cited per function) and is what a ctypes binding in the reference would call
 * (INTEGRATION.md shows the stub).  Conventions:
 *   - extern "C", plain pointers and sizes, no exceptions cross the boundary;
 *   - every function returns 0 on success, nonzero on error; mtn_last_error() gives the text;
 *   - all tensors are BORROWED device pointers, row-major, innermost dimension contiguous;
 *     the caller allocates outputs / saved-for-backward buffers and owns their lifetime;
 *   - kernels are enqueued on the hipStream_t passed in (void*), never synchronise, keep no
 *     global mutable state: re-entrant per stream, capturable into a hipGraph;
 *   - "lowp" buffers hold the compute element type selected by `dtype`:
 *       MTN_F32  : float   (exact-fp32 MFMA path, parity mode)
 *       MTN_BF16 : bfloat16 (fp32 accumulate; throughput mode)
 *     residual streams, LayerNorm / softmax statistics, biases, LN gains and all gradients of
 *     parameters are always float.
 */
#ifndef MTN_HIP_H
#define MTN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MTN_F32 0
#define MTN_BF16 1

#define MTN_OK 0
#define MTN_ERR_ARG 1
#define MTN_ERR_LAUNCH 2

/* Library / error reporting. */
const char* mtn_last_error(void);
/* 100: rounds 1-3.  110 (round 4): mtn_gemm_problem gained `ln`, mtn_mha_args / mtn_ffn_args gained `ln_fold` (callers must zero
 * the structs or set them), mtn_attn_args gained kv_acc / kv_last in round 3, and mtn_mha_bwd_ws_f32_floats() /
 * mtn_ffn_bwd_ws_f32_floats() return larger workspaces (multi-pass dK / dV sums; LayerNorm row-sum partials).
 * 111: mtn_transpose_desc gained `dst_off` (the transposed copies have a compact buffer of their own).
 * 112 (round 5): new entry points only (mtn_measure_mfma_peak_shapes, ...: see INTEGRATION.md); mtn_measure_mfma_peak now reports
 * the better of two MFMA shapes.
 * 113 (round 6): mtn_decode_args gained the trailing field `max_m`; mtn_decode_step takes W <= 16 rows, clamps `grid` to the device's
 * compute-unit count and bounds its polls in time (see there).
 * 114: mtn_assemble_tokens_desc gained the trailing field `row_len` (NULL = no cut; a zeroed struct keeps meaning that).
 * 115: new entry point mtn_sample_rows.  116: new entry point mtn_score_rows.  117: new entry point mtn_constrain_rows.
 * 121: new entry point mtn_mbr_select.  122: new entry points mtn_eval_metrics and mtn_eval_workspace_bytes.
 * 123: new entry points mtn_distill_fwd / _bwd.  124: new entry points mtn_lerp_f32, mtn_ema_step and mtn_swap_f32.
 * 125: new entry points mtn_wlosshead_fwd / _bwd, mtn_eval_table_build, mtn_eval_score_rows, mtn_scst_assemble and mtn_scst_advantage.
 * Entry points added since (mtn_ulosshead_fwd / _bwd; mtn_grad_sumsq_partials, mtn_grad_sumsq, mtn_clip_scale; mtn_grad_accum;
 * mtn_sched_mix; mtn_rlosshead_fwd / _bwd) are detected by symbol: additions only, the version stays 125. */
int mtn_version(void);

/* ------------------------------------------------------------------------------------------
 * Dropout stream: keep-mask bit for element `idx` of site `salt` is a pure function of
 * (*seed, salt, idx), so backward regenerates it.  `seed` is a DEVICE pointer (a replayed
 * hipGraph sees a fresh value each step).  p == 0 or seed == NULL disables dropout.
 * (reference: nn.Dropout at mtn.py:123,230,246,277)
 * ------------------------------------------------------------------------------------------ */
typedef struct {
    float p;
    uint32_t salt;
    const uint64_t* seed;
} mtn_dropout;

/* ------------------------------------------------------------------------------------------
 * GEMM (building block of every Linear on the path: mtn.py:243-244,256-258,267,273-280).
 *   C[i][j] = epilogue( sum_k opA(i,k) * opB(j,k) )          i<M, j<N, k<K
 *   a_trans == 0 : opA(i,k) = A[i*lda + k]      a_trans == 1 : opA(i,k) = A[k*lda + i]
 *   b_trans == 0 : opB(j,k) = B[j*ldb + k]      b_trans == 1 : opB(j,k) = B[k*ldb + j]
 *   epilogue(v) : v += bias[j]; relu; dropout; gate (v = gate[i][j] > 0 ? v*gate_scale : 0);
 *                 v += residual[i*ldr + j]; then stored to out_f32 and/or out_lp (row stride ldc).
 *   rowsum_out (optional): rowsum_out[i] = sum_k opA(i,k)   (bias gradients ride on the dW GEMM).
 * Forward Linear: y = x W^T  -> A=x, B=W (both non-trans).  dX = dY W -> A=dY, B=W with b_trans.
 * dW = dY^T X -> A=dY with a_trans, B=X with b_trans.
 * Constraints: A,B are lowp of `dtype`; K, lda, ldb multiples of 8; 16-byte aligned bases.
 * Up to MTN_GEMM_MAX_GROUP independent problems are executed by ONE launch.
 * ------------------------------------------------------------------------------------------ */
/* Optional optimiser epilogue of a parameter-gradient GEMM (dW = dY^T X, a_trans = b_trans = 1): C is not stored as a
 * gradient; it IS the gradient of the parameter block p[M,N] (row stride ldc, the same element offsets as out_f32), and the
 * Adam update of mtn_adam_step is applied to it tile by tile while the accumulators are still in registers:
 *   g = C * *grad_scale;  m,v updated;  p -= lr/bc1 * m / (sqrt(v)/sqrt(bc2) + eps);
 *   p_lp[i*ldc+j] = lowp(p)   (optional; the compute-dtype weight copy)
 *   p_lpT[j*ldT+i] = lowp(p)  (optional; the transposed copy the dX GEMMs read)
 * This removes the gradient's HBM round trip (8 B/param), the separate transpose pass, and hides the optimiser's 26 B/param
 * behind the contraction.  Only valid when this GEMM is the ONLY contribution to that gradient in the step (no residual /
 * accumulation, no gradient exchange between ranks).  write_grad != 0 also stores C to out_f32. */
typedef struct {
    float *p, *m, *v;
    void* p_lp;
    void* p_lpT;
    int ldT;
    int write_grad;
    const float* state;      /* device [8]: as mtn_adam_step */
    const float* grad_scale; /* optional device scalar */
    float beta1, beta2, eps;
} mtn_adam_fuse;

/* LayerNorm backward by linearity (round 4; bf16, row-major A, B as the weight lies: dX = dY W).
 * A sublayer computes q = W LN(x) + b with LN(x) = a2 (x - mean) rstd + b2 (mtn.py:111-114, 127).  The two row sums LayerNorm
 * backward needs from g = dq W —  s1 = sum_c a2_c g_c  and  s2 = sum_c a2_c (x_c - mean) g_c  — are linear in dq:
 *     s1 = sum_k dq_k u_k,                 u_k = sum_c W_kc a2_c
 *     s2 = 1/rstd sum_k dq_k (q_k - c_k),  c_k = b_k + sum_c W_kc b2_c        (q = the SAVED projection output)
 * so the kernels that PRODUCE dq emit them as per-row partial sums (one pair per row and column block, plain stores, no
 * cross-workgroup synchronisation) and the GEMM g = dq W finishes LayerNorm backward in its epilogue:
 *     dx = rstd a2 g - rstd s1/d - s2 rstd^2/(std (d-1)) (x - mean) + dres
 * instead of writing g for a separate LayerNorm-backward launch.  u | c ("fold vectors", float [2K]) come from mtn_ln_fold().
 *   mode MTN_LN_EMIT    (the GEMM that produces dq itself: dh = (dy W2) gated, FFN sublayers; N % 64 == 0, 64-column tiles):
 *       part[row][N/64][2] += {sum v u, sum v (gate * gate_inv_scale - c)} over each 64-column block of the row; v = the stored value
 *       (`gate` is required, and ldc — and ldr, with a residual — must be a multiple of 4: the gate value is read on the epilogue's
 *        16-byte path only; anything else is refused, MTN_ERR_ARG)
 *   mode MTN_LN_CONSUME (g = dq W, N = d_model <= 512):  out_f32 / out_lp of the problem are ignored (may be NULL);
 *       part[row][np][2] are summed in index order; dx, dx_lp (through dx_lp_drop, as mtn_ln_bwd_desc) are written;
 *       colpart [ceil(M/8)][2N] receives the da2 | db2 partial rows of mtn_layernorm_bwd (same layout: finalize unchanged).
 *   (mode 3, round 4's forward twin — LayerNorm FORWARD by linearity — was measured without net gain and removed in version 112.) */
#define MTN_LN_EMIT 1
#define MTN_LN_CONSUME 2
typedef struct mtn_ln_epilogue_s {
    int mode;
    const float* fold;     /* EMIT: u[N] then c[N] */
    float gate_inv_scale;  /* EMIT: 1 / (the gate's dropout scale) */
    float* part;           /* EMIT: written; CONSUME: read */
    int np;                /* CONSUME: partial pairs per row */
    const float *x, *a2, *mean, *rstd, *dres; /* CONSUME: the fields of mtn_ln_bwd_desc; x, mean, rstd saved by forward, dres optional */
    float eps;
    float* dx;
    void* dx_lp;           /* optional, compute dtype */
    mtn_dropout dx_lp_drop;
    float* colpart;        /* optional */
} mtn_ln_epilogue;

typedef struct {
    const void* A;
    const void* B;
    int lda, ldb;
    int M, N, K;
    int a_trans, b_trans;
    const float* bias;
    int relu;
    mtn_dropout drop;
    const void* gate; /* lowp [M,N], row stride ldc */
    float gate_scale;
    const float* residual;
    int ldr;
    float* out_f32;
    void* out_lp;
    int ldc;
    int lp_drop_after_residual; /* != 0: `drop` is NOT applied to v; it is applied to the out_lp copy only, after the residual
                                   (an accumulated gradient leaving also as the masked compute-dtype operand of its consumer) */
    float* rowsum_out;
    const mtn_adam_fuse* adam; /* HOST pointer, read during the call only; NULL = plain GEMM */
    const struct mtn_ln_epilogue_s* ln; /* HOST pointer, read during the call only; NULL = none (LayerNorm-backward epilogue, above) */
} mtn_gemm_problem;

#define MTN_GEMM_MAX_GROUP 16
int mtn_gemm(int dtype, int count, const mtn_gemm_problem* problems /* host array */, void* stream);
/* Table form for parameter-gradient problems (a_trans = b_trans = 1, bf16, plain C or the optimiser epilogue): up to 1024
 * problems in ONE launch of 128 x 128 tiles, in the order given (put contractions of different length next to each other:
 * resident workgroups then drift out of phase and the epilogue's HBM streaming overlaps other tiles' contractions).  The
 * problem list is staged to device memory on `stream`; safe under hipGraph capture. */
int mtn_gemm_tt_table(int dtype, int count, const mtn_gemm_problem* problems /* host array */, void* stream);
/* The same launch also carrying the REST of the optimiser step (round 5, version 112) — `opt.step()` of data_utils.py:154 for the
 * parameters no dW epilogue covers, so that nothing runs behind the launch:
 *   ln[]        LayerNorm gains / biases: gradient = the sum of the partial rows left by the LayerNorm-backward kernels (what
 *               mtn_layernorm_bwd_finalize computes, same summation order, same bits; stored at g + a_off / g + b_off) + Adam;
 *   chunks      ranges of the flat buffers whose gradient is COMPLETE before the launch (embedding tables): Adam as
 *               mtn_adam_step_chunks;
 *   bias_adam   every problem whose rowsum_out lies inside [g, g + n_flat): that bias is updated by the tile that sums its gradient.
 * All with the arithmetic of mtn_adam_step (bit-identical results).  The caller leaves exactly these ranges out of any later pass.
 * ln / chunk_off / chunk_len are HOST arrays read during the call; offsets and n_flat are in elements of the flat buffers. */
typedef struct { const float* partial; int nparts, d; long a_off, b_off; } mtn_tt_ln_unit;
typedef struct {
    float *p, *g, *m, *v; void* lp;          /* flat fp32 parameters, gradients, both moments; compute-dtype copy (NULL = none) */
    long n_flat;
    int n_ln; const mtn_tt_ln_unit* ln;
    int n_chunks; const long* chunk_off; const int* chunk_len;   /* <= 4096 elements each, multiples of 4 */
    int bias_adam;
    const float* state; const float* grad_scale; float beta1, beta2, eps;     /* as mtn_adam_fuse */
} mtn_tt_aux;
int mtn_gemm_tt_table_aux(int dtype, int count, const mtn_gemm_problem* problems /* host array */, const mtn_tt_aux* aux /* host, NULL = none */, void* stream);

/* ------------------------------------------------------------------------------------------
 * LayerNorm, MTN variant (mtn.py:103-114): y = a2 * (x-mean) / (std_unbiased + eps) + b2.
 * fwd: x [rows,d] float.  Optional outputs: y_f32, y_lp (lowp), mean[rows], rstd[rows]
 *      with rstd = 1/(std+eps).
 * bwd: g = dL/dy [rows,d] float; dres (optional) = gradient arriving on the residual branch,
 *      added to dx.  dx [rows,d] float (may alias dres).  da2/db2 [d] float are WRITTEN
 *      (not accumulated); `partial` is caller scratch of mtn_layernorm_bwd_partial_floats().
 * ------------------------------------------------------------------------------------------ */
#define MTN_LN_MAX_GROUP 8
typedef struct {
    int rows, d;
    float eps;
    const float *x, *a2, *b2;
    float* y_f32;
    void* y_lp;
    float *mean, *rstd;
    /* Optional fused source (Embeddings + PositionalEncoding, mtn.py:282-309): when `tokens` is set the row is built as
     * x[row] = dropout(lut[tokens[row]] * emb_scale + pe[row % seq_len]) instead of being read from `x`; when only `pe` is
     * set, x[row] = dropout(x[row] + pe[row % seq_len]) (feature streams, mtn.py:378).  `x_out` (optional) receives that
     * row (saved for backward).  no_ln != 0: no normalisation, y = the row (target embedding, mtn.py:59). */
    const long* tokens;
    const float* lut;
    float emb_scale;
    const float* pe;
    int seq_len;
    mtn_dropout drop;
    float* x_out;
    int no_ln;
} mtn_ln_fwd_desc;
/* Embedding backward: dlut[tokens[row]] += dx[row] * emb_scale * keep(row*d+c)/(1-p).
 * Default (lut_rows > 0 on every descriptor: the vocabulary size of the table behind dlut): bitwise reproducible — each
 * vocabulary entry is owned by one wave (frequent entries by one workgroup) that scans the token lists of all streams sharing
 * the table and adds the matching rows in list order, no atomics; measured 31 vs 13 us (uniform tokens) and 175 vs 69 us
 * (ragged, 25 % pads) at cfg2 batch 32 against the alternative.  MTN_EMBED_DETERMINISTIC=0 in the environment (or lut_rows == 0)
 * selects that alternative: float atomic adds, whose rounding depends on arrival order — then the only run-to-run noise on the
 * whole path. */
typedef struct {
    int rows, d;
    const long* tokens;
    const float* dx;
    float emb_scale;
    mtn_dropout drop;
    float* dlut;
    int lut_rows;
} mtn_embed_bwd_desc;
int mtn_embed_bwd_group(int count, const mtn_embed_bwd_desc* descs /* host array, <= MTN_LN_MAX_GROUP */, void* stream);
typedef struct {
    int rows, d;
    float eps;
    const float *x, *a2, *mean, *rstd, *g, *dres;
    float* dx;
    float* partial; /* NULL: dx only */
    /* optional second output: dx as the NEXT backward stage wants it — through that sublayer's output-dropout mask and in
       the compute dtype (saves its cast launch).  dx_lp NULL = off; dx_lp_dtype MTN_F32 | MTN_BF16. */
    void* dx_lp;
    int dx_lp_dtype;
    mtn_dropout dx_lp_drop;
} mtn_ln_bwd_desc;
/* Grouped forms: up to MTN_LN_MAX_GROUP independent row streams per launch. */
int mtn_layernorm_fwd_group(int dtype, int count, const mtn_ln_fwd_desc* descs /* host array */, void* stream);
int mtn_layernorm_bwd_group(int count, const mtn_ln_bwd_desc* descs /* host array */, void* stream);
int mtn_layernorm_fwd(int dtype, int rows, int d, float eps, const float* x, const float* a2, const float* b2,
                      float* y_f32, void* y_lp, float* mean, float* rstd, void* stream);
/* Fold vectors of the Linears that follow a LayerNorm (see mtn_ln_epilogue): for each descriptor, with W [K, d] in the compute
 * dtype (bf16), out[k] = sum_c W[k][c] a2[c] and out[K + k] = bias[k] + sum_c W[k][c] b2[c].  One launch for the whole model:
 * `descs_device` is a DEVICE array of `count` descriptors, `block_desc` a DEVICE int32 array giving the descriptor of each
 * 64-row block (block_start = the descriptor's first block), total_blocks = sum ceil(K / 64).  d % 8 == 0, d <= 2048. */
typedef struct {
    const void* w;
    const float *bias, *a2, *b2;
    float* out;
    int K, block_start;
} mtn_ln_fold_desc;
int mtn_ln_fold(int dtype, const mtn_ln_fold_desc* descs_device, const int* block_desc, int total_blocks, int d, void* stream);
long mtn_layernorm_bwd_partial_floats(int rows, int d);
int mtn_layernorm_bwd_nparts(int rows);
/* da2/db2 == NULL: only dx is produced now and `partial` is left for a later grouped mtn_layernorm_bwd_finalize()
 * (many LayerNorms per launch, off the critical path of backward).  partial == NULL: dx only, no parameter gradients. */
typedef struct {
    const float* partial; /* [nparts][2*d] as written by mtn_layernorm_bwd */
    int nparts, d;
    float *da2, *db2;
} mtn_ln_finalize_desc;
#define MTN_LN_FINALIZE_MAX_GROUP 112 /* descriptors per launch (3.6 KB of kernel arguments): all LayerNorms of a cfg2 step in one */
int mtn_layernorm_bwd_finalize(int count, const mtn_ln_finalize_desc* descs /* host array */, void* stream);
int mtn_layernorm_bwd(int rows, int d, float eps, const float* x, const float* a2, const float* mean,
                      const float* rstd, const float* g, const float* dres, float* dx, float* da2, float* db2,
                      float* partial, void* stream);

/* ------------------------------------------------------------------------------------------
 * Scaled-dot-product attention core (mtn.py:221-231) for all heads of all batch rows.
 *   q  : lowp, element (b,i,h,c) at q[(b*a+i)*ldq + h*dk + c]      i<a
 *   k,v: lowp, element (b,j,h,c) at k[(b*m+j)*ldkv + h*dk + c]     j<m
 *   mask: uint8, element (b,i,j) at mask[b*mask_sb + i*mask_sq + j]; 0 => score := -1e9
 *         (mask_sq == 0 broadcasts over query rows; mask == NULL => nothing masked)
 *   o  : lowp [(b*a+i)*ldo + h*dk + c];  lse: float2 per (b,head,i) at lse[2*((b*h+hh)*a+i)] = {row max, 1/row sum}
 *        (kept apart: a fully masked row has max = -1e9, where max + log(sum) would lose log(sum))
 * bwd: d_o lowp (same layout as o) -> dq (ldq layout), dk/dv (ldkv layout), all lowp.
 *      Gradient does not flow through masked scores (masked_fill).  Any number of query rows (the PE table of the
 *      reference goes to 5000, mtn.py:293): the MFMA kernel walks them in passes of 32.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
    int B, h, a, m, dk;
    const void *q, *k, *v;
    int ldq, ldkv;
    const uint8_t* mask;
    long mask_sb, mask_sq;
    mtn_dropout drop;
    void* o;
    int ldo;
    float* lse;
    /* backward only */
    const void* d_o;
    void *dq, *dk_out, *dv_out;
    /* backward, set by the library (callers leave them 0): one launch covers query rows q0 .. q0+qn-1 of every sequence;
       sequences longer than 32 rows are walked in several passes, kv_accum != 0 = add dk/dv to the earlier passes' sums,
       kv_last != 0 = this pass writes the final dk/dv */
    int q0, qn, kv_accum;
    /* backward, optional (caller): fp32 workspace of 2 * B * m * h * dk floats.  With it a multi-pass backward keeps the dK / dV
       sums of the passes in fp32 ([B*m][h*dk] for dK, then the same for dV) and rounds to the output type once, in the last
       pass; without it the passes accumulate in the (low-precision) output buffers. */
    float* kv_acc;
    int kv_last;
} mtn_attn_args;
#define MTN_ATTN_MAX_GROUP 4
/* Grouped forms: up to MTN_ATTN_MAX_GROUP independent attention problems (different shapes allowed) per launch. */
int mtn_attention_fwd_group(int dtype, int count, const mtn_attn_args* args /* host array */, void* stream);
int mtn_attention_bwd_group(int dtype, int count, const mtn_attn_args* args /* host array */, void* stream);
int mtn_attention_fwd(int dtype, const mtn_attn_args* args, void* stream);
int mtn_attention_bwd(int dtype, const mtn_attn_args* args, void* stream);

/* ------------------------------------------------------------------------------------------
 * Fused sublayers: SublayerConnection.forward (mtn.py:125-127) around MultiHeadedAttention
 * (mtn.py:248-267) or PositionwiseFeedForward (mtn.py:279-280):
 *     y = x + dropout( f( LayerNorm(x) ) )
 * Weight layout: w_qkv is the three input Linears stacked [3d,d] (q,k,v order = linears[0..2]),
 * b_qkv [3d]; w_o/b_o = linears[3].  Self-attention (kv source = LayerNorm(x)) runs one packed
 * QKV projection; cross-attention projects q from LayerNorm(x) and k,v from `mem` [B,m,d] lowp.
 * Saved-for-backward buffers are caller-allocated (sizes in comments).
 * ------------------------------------------------------------------------------------------ */
typedef struct {
    int B, a, m, d, h;
    int self_attn;
    float ln_eps;
    mtn_dropout drop_attn; /* on softmax probabilities (mtn.py:230) */
    mtn_dropout drop_out;  /* on the sublayer output (mtn.py:127)   */
    const float* x;        /* [B,a,d] */
    const void* mem;       /* lowp [B,m,d]; unused when self_attn */
    const uint8_t* mask;
    long mask_sb, mask_sq;
    const float *ln_a, *ln_b;
    const void* w_qkv; /* lowp [3d,d] */
    const float* b_qkv;
    const void* w_o; /* lowp [d,d] */
    const float* b_o;
    const void* w_qkv_t; /* lowp [d,3d] = w_qkv^T, optional (backward: NULL -> dX = dY W reads w_qkv as it lies, b_trans = 1 on the LDS-DMA GEMM: what the training step does since round 3) */
    const void* w_o_t;   /* lowp [d,d]  = w_o^T,  optional; REQUIRED for the fused head backward (it reads w_o^T rows), NULL -> staged path */
    float* y;    /* [B,a,d] */
    void* xn;    /* lowp [B*a,d]  saved */
    float* mean; /* [B*a]         saved */
    float* rstd; /* [B*a]         saved */
    void* qkv;   /* lowp: self [B*a,3d]; cross [B*a,d] (q only)   saved */
    void* kv;    /* lowp cross only [B*m,2d]                      saved */
    void* o;     /* lowp [B*a,d]  saved */
    float* lse;  /* [2*B*h*a]     saved */
    /* ---- backward (mtn_mha_sublayer_bwd) ---- */
    const float* dy; /* [B,a,d] */
    float* dx;       /* [B,a,d] written */
    float* dmem;     /* [B,m,d] float gradient of mem (cross only; NULL = not needed) */
    int dmem_accumulate; /* 0: dmem is written; 1: dmem += (memory shared by several sublayers) */
    float *d_ln_a, *d_ln_b;                   /* [d] written */
    float *d_w_qkv, *d_b_qkv, *d_w_o, *d_b_o; /* written */
    void* ws_lp;   /* lowp scratch: mtn_mha_bwd_ws_lp_elems() elements */
    float* ws_f32; /* float scratch: mtn_mha_bwd_ws_f32_floats() */
    int defer_param_grads; /* 1: backward skips the dW/db GEMMs and the LayerNorm finalize; the caller batches them
                              later from mtn_mha_param_grad_work() (ws_lp/ws_f32 and saved buffers must stay alive) */
    /* ---- gradient hand-off between consecutive sublayers of a chain (all optional) ----
       dyl_ready: dropout-masked compute-dtype image of dy already produced by the sublayer that ran before this one in
                  backward (its next_dyl): the cast stage is skipped and the dW GEMMs read it instead of ws_lp's copy.
       next_dyl / next_drop: ask this backward's LayerNorm stage to also write dx through `next_drop` (the output dropout of
                  the sublayer that will consume dx as its dy) in the compute dtype, [rows, d]. */
    const void* dyl_ready;
    void* next_dyl;
    mtn_dropout next_drop;
    /* forward, cross attention: 1 = `kv` already holds K|V of the memory (projected ahead of the layer loop for every layer
       that attends the same constant memory, one grouped GEMM): the sublayer skips that projection.  Backward is unchanged. */
    int kv_ready;
    /* backward, optional: the memory gradient after THIS sublayer's contribution is final (the caller knows: last user of a
       shared gradient buffer) and its producer wants it once more through its output dropout in the compute dtype
       [B*m, d] — written by the dmem GEMM's epilogue instead of a cast launch */
    void* dmem_lp;
    mtn_dropout dmem_lp_drop;
    /* optional: fold vectors of w_qkv behind this sublayer's LayerNorm (mtn_ln_fold: float [2K], K = 3d self / d cross: only the
       q block sees LN(x)).  With them (bf16, fused head backward) LayerNorm backward rides in the dLN-out GEMM's epilogue
       (mtn_ln_epilogue) and the group's LayerNorm-backward launch disappears; NULL = the separate launch. */
    const float* ln_fold;
    /* (version 112: the five trailing fields of round 4's LayerNorm FORWARD by linearity — xa, x_stats, ya, y_stats, next_ln_a — are gone) */
} mtn_mha_args;
int mtn_mha_sublayer_fwd(int dtype, const mtn_mha_args* args, void* stream);
int mtn_mha_sublayer_bwd(int dtype, const mtn_mha_args* args, void* stream);
/* Deferred parameter-gradient work of one sublayer backward: fills up to 3 GEMM problems (host structs, nothing is
 * launched) and one LayerNorm finalize descriptor; returns the number of GEMM problems.  Feed them to mtn_gemm()
 * (any grouping) and mtn_layernorm_bwd_finalize() once the sublayer's backward has been enqueued. */
int mtn_mha_param_grad_work(int dtype, const mtn_mha_args* args, mtn_gemm_problem* out3, mtn_ln_finalize_desc* out_ln);
long mtn_mha_bwd_ws_lp_elems(int B, int a, int m, int d, int self_attn);
long mtn_mha_bwd_ws_f32_floats(int B, int a, int m, int d);

typedef struct {
    int rows, d, d_ff;
    float ln_eps;
    mtn_dropout drop_hidden; /* mtn.py:280 */
    mtn_dropout drop_out;    /* mtn.py:127 */
    const float* x;          /* [rows,d] */
    const float *ln_a, *ln_b;
    const void* w1; /* lowp [d_ff,d] */
    const float* b1;
    const void* w2; /* lowp [d,d_ff] */
    const float* b2;
    const void* w1_t; /* lowp [d,d_ff] = w1^T, optional (backward; NULL -> w1 as it lies, b_trans = 1) */
    const void* w2_t; /* lowp [d_ff,d] = w2^T, optional (backward; NULL -> w2 as it lies, b_trans = 1) */
    float* y;    /* [rows,d] */
    void* xn;    /* lowp [rows,d]    saved */
    float* mean; /* saved */
    float* rstd; /* saved */
    void* hid;   /* lowp [rows,d_ff] saved (post-ReLU, post-dropout) */
    /* ---- backward ---- */
    const float* dy;
    float* dx;
    float *d_ln_a, *d_ln_b, *d_w1, *d_b1, *d_w2, *d_b2;
    void* ws_lp;   /* lowp scratch: rows*d + rows*d_ff elements */
    float* ws_f32; /* float scratch: mtn_ffn_bwd_ws_f32_floats() */
    int defer_param_grads;
    /* ---- gradient hand-off between consecutive sublayers of a chain (all optional) ----
       dyl_ready: dropout-masked compute-dtype image of dy already produced by the sublayer that ran before this one in
                  backward (its next_dyl): the cast stage is skipped and the dW GEMMs read it instead of ws_lp's copy.
       next_dyl / next_drop: ask this backward's LayerNorm stage to also write dx through `next_drop` (the output dropout of
                  the sublayer that will consume dx as its dy) in the compute dtype, [rows, d]. */
    const void* dyl_ready;
    void* next_dyl;
    mtn_dropout next_drop;
    /* forward, optional: compute-dtype copy of y [rows,d], written by the same epilogue — for an output that a later sublayer
       attends as un-projected memory (an auto-encoder stream, mtn.py:215), which otherwise costs a cast launch */
    void* y_lp;
    const float* ln_fold; /* optional: fold vectors of w1 (float [2 d_ff]), as mtn_mha_args.ln_fold */
} mtn_ffn_args;
int mtn_ffn_sublayer_fwd(int dtype, const mtn_ffn_args* args, void* stream);
int mtn_ffn_sublayer_bwd(int dtype, const mtn_ffn_args* args, void* stream);
long mtn_ffn_bwd_ws_f32_floats(int rows, int d, int d_ff);
int mtn_ffn_param_grad_work(int dtype, const mtn_ffn_args* args, mtn_gemm_problem* out2, mtn_ln_finalize_desc* out_ln);

/* ------------------------------------------------------------------------------------------
 * Lockstep sublayer groups.  The sublayers of one DecoderLayer that do not depend on each other (x's text attention,
 * the two auto-encoder chains) share every kernel launch: stage 1 one grouped LayerNorm, stage 2 one grouped GEMM
 * (QKV / Q+KV / FFN-1), stage 3 one grouped attention (attention members only), stage 4 one grouped GEMM (output
 * projection / FFN-2 with bias+dropout+residual).  Backward mirrors it in 5 grouped stages.  Launch count per group is
 * 4 (5) whatever the number of members; up to MTN_SUBLAYER_MAX_GROUP attention + as many FFN members.
 * Backward always defers parameter gradients (see mtn_*_param_grad_work).
 * ------------------------------------------------------------------------------------------ */
#define MTN_SUBLAYER_MAX_GROUP 4
/* Forward of a group whose members are bf16 with d = 512, h = 8 (d_k = 64), a <= 64 query rows per sample and memories of
 * <= 256 rows runs stages 1-3 as ONE launch (csrc/fused.hip: LayerNorm -> head slice of the input projections -> attention,
 * or LayerNorm -> column slice of w_1 + ReLU + dropout, per (block of samples, head | column slice) workgroup); results and
 * saved buffers are those of the four-launch path.  mtn_fused_enable(0) turns that off for the process (A/B measurements and
 * the tests that compare the two paths); returns the previous setting (-1 = never set: environment MTN_FUSED=0 disables). */
int mtn_fused_enable(int on);
/* How many sublayer groups took which path since the library was loaded: out4 = {forward fused, forward per-stage, backward
 * fused (groups with attention members), backward per-stage}.  The parity tests use it to assert that the fused kernels ran. */
int mtn_fused_counters(long* out4);
/* K|V projections of CONSTANT memories for many sublayers (problems as for mtn_gemm: bf16, K = 512, bias epilogue into out_lp; any
 * count).  The first n_now problems are computed now.  The others may WAIT (riders on, every grouped launch of the list would take
 * the wide one-shot K = 512 kernel): they leave as rider workgroups of the fused forward launches of mtn_sublayer_group_fwd, on
 * compute units those launches leave empty (csrc/gemm_k512.hip, csrc/fused.hip), in the order given — pass them in the order of
 * their first use.  mtn_sublayer_group_fwd first launches stand-alone whatever is still pending of a K|V buffer its members read
 * (and of everything in front of it), and mtn_riders_flush() launches all that is left: nothing is skipped, and a buffer's bits do not
 * depend on which launch carried its tiles.  Operands and outputs must stay valid until then.  Otherwise — riders off, other
 * shapes, batches whose launches take the persistent form — the call is the grouped mtn_gemm launches of the whole list, now.
 * Environment (mtn_reload_env): MTN_RIDERS=0 riders off; MTN_RIDER_MAX_SLOTS=<n> at most n rider workgroups per launch;
 * MTN_RIDER_FFN_HOSTS=0|1 launches with feed-forward members carry riders or not. */
int mtn_kv_project(int dtype, int count, const mtn_gemm_problem* problems /* host array */, int n_now, void* stream);
/* Launch stand-alone whatever is still pending.  Call it at the end of every forward that deferred work. */
int mtn_riders_flush(void* stream);
int mtn_riders_enabled(void);
/* out4 = {K|V tiles computed by rider workgroups, tiles launched stand-alone from the pending list, such stand-alone launches,
 * tiles pending now} since the library was loaded. */
int mtn_rider_counters(long* out4);
/* Backward groups (since the library was loaded) whose LayerNorm backward rode in the epilogue of the dLN-out GEMM (mtn_ln_epilogue)
 * instead of its own launch: the tests use it to assert which path ran. */
long mtn_ln_epilogue_groups(void);
int mtn_sublayer_group_fwd(int dtype, int n_mha, const mtn_mha_args* mha, int n_ffn, const mtn_ffn_args* ffn, void* stream);
int mtn_sublayer_group_bwd(int dtype, int n_mha, const mtn_mha_args* mha, int n_ffn, const mtn_ffn_args* ffn, void* stream);

/* ------------------------------------------------------------------------------------------
 * Elementwise helpers on the path.
 * ------------------------------------------------------------------------------------------ */
/* dst(lowp) = cast(src float); n elements. */
int mtn_cast_f32_to_lp(int dtype, long n, const float* src, void* dst, void* stream);
typedef struct {
    long n;
    const float* src;
    void* dst;
    mtn_dropout drop;
    const float* gate; /* optional: elements with gate[i] <= 0 are zeroed (ReLU backward from the saved activation) */
} mtn_cast_desc;
#define MTN_CAST_MAX_GROUP 8
/* Grouped cast / dropout-backward: dst_g(lowp)[i] = src_g[i] * keep_g(i)/(1-p_g) [* (gate_g[i] > 0)]. */
int mtn_cast_group(int dtype, int count, const mtn_cast_desc* descs /* host array */, void* stream);
/* dst(lowp)[i] = src[i] * keep(i)/(1-p): gradient entering a dropped-out branch (mtn.py:127). */
int mtn_dropout_bwd_to_lp(int dtype, long n, const float* src, mtn_dropout drop, void* dst, void* stream);

/* ------------------------------------------------------------------------------------------
 * Loss head: Generator log-softmax (mtn.py:62-69) + LabelSmoothing KLDivLoss(sum) (label_smoothing.py:20-32) +
 * the weighted sum of SimpleLossCompute (data_utils.py:133-144), per row, without materialising log-probabilities or
 * target distributions.  Rows of up to MTN_LOSSHEAD_MAX_SEG streams (main decoder output, auto-encoder outputs) are
 * stacked: rows[s] rows of stream s with targets target[s] (int64), loss weight coef[s] / *norm[s] (norm = device scalar).
 *   fwd: logits float [sum rows, ldz] -> lse[row], rowloss[row] (already weighted; the loss is their sum)
 *   bwd: dlogits lowp [sum rows, ldd] = *gloss * weight * (softmax * sum(td) - td); columns V..ldd-1 are zero-filled
 * ------------------------------------------------------------------------------------------ */
#define MTN_LOSSHEAD_MAX_SEG 4
typedef struct {
    int n_seg;
    int rows[MTN_LOSSHEAD_MAX_SEG];
    const long* target[MTN_LOSSHEAD_MAX_SEG];
    const float* norm[MTN_LOSSHEAD_MAX_SEG];
    float coef[MTN_LOSSHEAD_MAX_SEG];
    int V, ldz, pad;
    float smoothing;
    const float* logits;
    float* lse;
    float* rowloss;
    const float* gloss; /* backward: device scalar dL/dloss */
    void* dlogits;
    int ldd;
} mtn_losshead_args;
int mtn_losshead_fwd(const mtn_losshead_args* args, void* stream);
int mtn_losshead_bwd(int dtype, const mtn_losshead_args* args, void* stream);

/* Loss head with teacher soft targets (version 123; csrc/losshead.hip): word-level knowledge distillation.  Every field of
 * mtn_losshead_args keeps its meaning.  teacher[s] is a device matrix [rows[s]][ldq[s]] of float, 16-byte aligned, ldq >= V and
 * ldq % 4 == 0 (columns V..ldq-1 are never read), NULL = segment s has no teacher.  A teacher row holds log-probabilities or logits:
 * it is normalised here, as mtn_ensemble_rows normalises its members.  With z the student row, q the teacher row, t the target,
 * KL_ls and td the loss head's (the lone-<pad> quirk included), scale = coef[s] / *norm[s], T = temperature:
 *   a_j = z_j / T, b_j = q_j / T, pS = softmax(a), pT = softmax(b)
 *   kd      = sum_j pT_j (log pT_j - log pS_j); a column with q_j = -inf contributes exactly 0 (no 0 * inf).  Evaluated with the row
 *             maxima m_a, m_b taken out: kd = sum_j e_j ((b_j - m_b) - (a_j - m_a)) / sum_j e_j - log sum_j e_j + log sum_j exp(a_j - m_a),
 *             e_j = exp(b_j - m_b)
 *   kd      = 0 on every row whose target is <pad> (the teacher row is not read); on the quirk row (a lone <pad> at a segment's row 0)
 *             the hard part is the loss head's KL_ls as on any live row
 *   rowloss = scale [(1 - alpha) KL_ls + alpha T^2 kd]          rowkd (optional, [sum rows]) = kd, unscaled
 *   lse     = the T = 1 log-sum-exp of z, as mtn_losshead_fwd writes it
 *   bwd:      dlogits_j = *gloss scale [(1 - alpha)(softmax_j(z) sum(td) - td_j) + alpha T (pS_j - pT_j)], the second term 0 on
 *             <pad>-target rows; columns V..ldd-1 are +0.0.  Reads lse (of the forward call), logits and the teacher rows.
 * A segment with teacher == NULL, and every segment when alpha == 0, never reads a teacher and applies no (1 - alpha) factor: lse,
 * rowloss and dlogits are those of mtn_losshead_fwd / _bwd on the same inputs bit for bit, rowkd is 0.
 * MTN_ERR_ARG, nothing launched: whatever mtn_losshead_fwd / _bwd refuse; alpha outside [0, 1] or not finite; temperature <= 0 or not
 * finite; ldq < V, ldq % 4 != 0 or a misaligned pointer on a segment with a teacher.  A teacher row without a finite entry is NOT
 * checked (device memory): its kd and gradient are NaN. */
typedef struct {
    int n_seg;
    int rows[MTN_LOSSHEAD_MAX_SEG];
    const long* target[MTN_LOSSHEAD_MAX_SEG];
    const float* norm[MTN_LOSSHEAD_MAX_SEG];
    float coef[MTN_LOSSHEAD_MAX_SEG];
    int V, ldz, pad;
    float smoothing;
    const float* logits;
    float* lse;
    float* rowloss;
    const float* gloss; /* backward: device scalar dL/dloss */
    void* dlogits;
    int ldd;
    const float* teacher[MTN_LOSSHEAD_MAX_SEG];
    long ldq[MTN_LOSSHEAD_MAX_SEG];
    float alpha;
    float temperature;
    float* rowkd; /* optional */
} mtn_distill_args;
int mtn_distill_fwd(const mtn_distill_args* args, void* stream);
int mtn_distill_bwd(int dtype, const mtn_distill_args* args, void* stream);

/* Loss head with signed row weights (version 125; csrc/losshead.hip): the policy-gradient loss of self-critical sequence training
 * (Rennie et al. 2017), where a sampled row's weight is -(reward - baseline).  Every field of mtn_losshead_args keeps its meaning.
 * roww[s] is a device array of rows[s] floats, 4-byte aligned, NULL = every weight of segment s is 1.  smoothing_seg[s] >= 0 is the label
 * smoothing of segment s (0: KL_ls = -log p(target) on a live row); smoothing_seg[s] < 0 = the segment takes `smoothing`.  With KL_ls, td
 * and the zeroed rows the loss head's (the lone-<pad> quirk included) at the segment's smoothing, scale = coef[s] / *norm[s], w = roww[s][row]:
 *   rowloss = scale w KL_ls                                 lse = as mtn_losshead_fwd writes it (it does not depend on w)
 *   bwd:      dlogits_j = *gloss scale w (softmax_j(z) sum(td) - td_j); columns V..ldd-1 are +0.0
 * w may be negative or zero; a row with w == 0 writes rowloss = +0.0 and a dlogits row of +0.0, as a zeroed <pad> row does.  A non-finite
 * weight is device data and is NOT checked: its rowloss and dlogits row are not finite.
 * A segment with roww == NULL and the loss head's smoothing runs the same code as the plain loss head: lse, rowloss and dlogits
 * are those of mtn_losshead_fwd / _bwd on the same inputs bit for bit.
 * MTN_ERR_ARG, nothing launched: whatever mtn_losshead_fwd / _bwd refuse; a roww pointer that is not 4-byte aligned; a smoothing_seg that is
 * NaN. */
typedef struct {
    int n_seg;
    int rows[MTN_LOSSHEAD_MAX_SEG];
    const long* target[MTN_LOSSHEAD_MAX_SEG];
    const float* norm[MTN_LOSSHEAD_MAX_SEG];
    float coef[MTN_LOSSHEAD_MAX_SEG];
    int V, ldz, pad;
    float smoothing;
    const float* logits;
    float* lse;
    float* rowloss;
    const float* gloss; /* backward: device scalar dL/dloss */
    void* dlogits;
    int ldd;
    const float* roww[MTN_LOSSHEAD_MAX_SEG];
    float smoothing_seg[MTN_LOSSHEAD_MAX_SEG];
} mtn_wlosshead_args;
int mtn_wlosshead_fwd(const mtn_wlosshead_args* args, void* stream);
int mtn_wlosshead_bwd(int dtype, const mtn_wlosshead_args* args, void* stream);

/* Loss head with token-level unlikelihood (csrc/losshead.hip; detected by symbol, mtn_version() stays 125): the training-time repetition
 * penalty of Welleck et al. 2019.  Every field of mtn_losshead_args keeps its meaning.  A segment with seq_len[s] = T > 0 holds rows[s] / T
 * sequences of T positions, local row = b T + t (how trg_y.view(-1) lies); the earlier targets are read from target[s].  For a row whose
 * target y_t is not <pad>, with z its logits, lse its log-sum-exp, p_j = exp(z_j - lse), and the negative candidates the SET
 * C = { y_0 .. y_{t-1} } \ { y_t, <pad> } (each token once), scale = coef[s] / *norm[s], KL_ls, td, the zeroed rows and the lone-<pad> quirk
 * the loss head's:
 *   u_c     = 1 - p_c
 *   ul      = sum_{c in C} -log(max(u_c, MTN_UL_CLAMP))     summed in an order the set fixes: two launches give the same bytes
 *   rowloss = scale (KL_ls + ul_alpha ul)                   rowul (optional, [sum rows]) = ul, unscaled;  lse = as mtn_losshead_fwd writes it
 *   bwd:      live(c) = c in C and u_c >= MTN_UL_CLAMP      (a clamped candidate has gradient 0, as torch.clamp gives)
 *             r_c = p_c / u_c for live c, R = sum_{live c} r_c
 *             dlogits_j = *gloss scale [(softmax_j sum(td) - td_j) + ul_alpha ([j live] r_j - p_j R)]; columns V..ldd-1 are +0.0
 * ul = 0 and no extra gradient on every <pad>-target row (the quirk row included) and on every row with t = 0: those rows, every row of a
 * segment with seq_len[s] == 0, and every segment when ul_alpha == 0 (the host drops seq_len) run the plain head's code: lse, rowloss and
 * dlogits are those of mtn_losshead_fwd / _bwd on the same inputs bit for bit, rowul is +0.0.
 * Candidates with u_c between 1e-9 and the clamp's far side (p_c between 0.9 and 1 - 1e-9) are outside what the tests hold: there 1 - p_c
 * loses up to log2(1 / u_c) bits in float and which side of the clamp a candidate falls on is not stable.
 * MTN_ERR_ARG, nothing launched: whatever mtn_losshead_fwd / _bwd refuse; ul_alpha negative or not finite; seq_len[s] < 0;
 * rows[s] % seq_len[s] != 0; V > MTN_ULOSSHEAD_MAX_V (a bitmap of V bits per row lives in LDS).  Entries past n_seg are not looked at. */
#define MTN_UL_CLAMP 1e-5f
#define MTN_ULOSSHEAD_MAX_V 65536
typedef struct {
    int n_seg;
    int rows[MTN_LOSSHEAD_MAX_SEG];
    const long* target[MTN_LOSSHEAD_MAX_SEG];
    const float* norm[MTN_LOSSHEAD_MAX_SEG];
    float coef[MTN_LOSSHEAD_MAX_SEG];
    int V, ldz, pad;
    float smoothing;
    const float* logits;
    float* lse;
    float* rowloss;
    const float* gloss; /* backward: device scalar dL/dloss */
    void* dlogits;
    int ldd;
    int seq_len[MTN_LOSSHEAD_MAX_SEG];
    float ul_alpha;
    float* rowul; /* optional */
} mtn_ulosshead_args;
int mtn_ulosshead_fwd(const mtn_ulosshead_args* args, void* stream);
int mtn_ulosshead_bwd(int dtype, const mtn_ulosshead_args* args, void* stream);

/* Loss head with a paired consistency term (csrc/losshead.hip; detected by symbol, mtn_version() stays 125): R-Drop (Liang et al. 2021),
 * the symmetric KL divergence between the next-token distributions of two passes of one position under independent dropout masks.  Every
 * field of mtn_losshead_args keeps its meaning.  pair[s] = 0: segment s is unpaired.  pair[s] = N > 0: the segment holds 2 N rows and local
 * rows i and i + N are the two passes of one position.  For a row i of a paired segment whose OWN target is not <pad>, with partner
 * j = i +- N, z_i / z_j their logits, m / lg the row maximum and log sum_c exp(z_c - m) of each (lse = m + lg), logp_c = (z_ic - m_i) - lg_i,
 * logq_c = (z_jc - m_j) - lg_j (the maxima taken out: a common offset between the two rows costs no bits), p = exp(logp), q = exp(logq),
 * d_c = logp_c - logq_c, scale = coef[s] / *norm[s], KL_ls, td, the zeroed rows and the lone-<pad> quirk the loss head's:
 *   J       = sum_c (p_c - q_c) d_c          (= KL(p||q) + KL(q||p); every term is >= 0.  Summed in one fixed column order, so the two rows
 *                                             of a pair hold the same float products in the same order: rowrd[i] == rowrd[i + N] bit for bit)
 *   kl      = sum_c p_c d_c                  (= KL(p||q), the directed one)              rowkl ([sum rows]) = kl: the backward reads it
 *   rd      = J / 4                          rowrd (optional, [sum rows]) = rd, unscaled
 *   rowloss = scale (KL_ls + rd_alpha rd)    lse = as mtn_losshead_fwd writes it
 *   bwd:      with p_k = exp(z_ik - lse[i]), q_k = exp(z_jk - lse[j]), d_k = (z_ik - lse[i]) - (z_jk - lse[j]), kl = rowkl[i]:
 *             dlogits_k = *gloss scale [(softmax_k sum(td) - td_k) + rd_alpha / 2 (p_k (d_k - kl) + p_k - q_k)]; columns V..ldd-1 are +0.0.
 *             Reads logits, lse and rowkl of the forward call.
 * Both rows of a pair carry rd and the normaliser of a doubled batch counts both passes' tokens, so the sum of rowloss is the mean of the
 * two passes' label-smoothed losses plus rd_alpha / 4 (KL(p||q) + KL(q||p)) per original token; the 1/2 of the backward is 2 * 1/4: a
 * row's logits enter its own rd and its partner's.
 * rd = +0.0, kl = +0.0 and no extra gradient on every row whose target is <pad> (the quirk row included): those rows never read their
 * partner.  They, every row of a segment with pair[s] == 0, and every segment when rd_alpha == 0 (the host drops pair) run the plain
 * head's code: lse, rowloss and dlogits are those of mtn_losshead_fwd / _bwd on the same inputs bit for bit, rowrd is +0.0.  No atomics:
 * two launches on the same inputs give the same bytes.
 * MTN_ERR_ARG, nothing launched: whatever mtn_losshead_fwd / _bwd refuse; rd_alpha negative or not finite; pair[s] < 0;
 * rows[s] != 2 * pair[s] on a paired segment; rowkl == NULL with a paired segment and rd_alpha > 0.  Entries past n_seg are not looked at. */
typedef struct {
    int n_seg;
    int rows[MTN_LOSSHEAD_MAX_SEG];
    const long* target[MTN_LOSSHEAD_MAX_SEG];
    const float* norm[MTN_LOSSHEAD_MAX_SEG];
    float coef[MTN_LOSSHEAD_MAX_SEG];
    int V, ldz, pad;
    float smoothing;
    const float* logits;
    float* lse;
    float* rowloss;
    const float* gloss; /* backward: device scalar dL/dloss */
    void* dlogits;
    int ldd;
    int pair[MTN_LOSSHEAD_MAX_SEG];
    float rd_alpha;
    float* rowrd; /* optional */
    float* rowkl; /* forward: written; backward: read */
} mtn_rlosshead_args;
int mtn_rlosshead_fwd(const mtn_rlosshead_args* args, void* stream);
int mtn_rlosshead_bwd(int dtype, const mtn_rlosshead_args* args, void* stream);

/* Transposed compute-dtype weight copies (operand of dX = dY W on the LDS-DMA GEMM path): for each descriptor the
 * [rows, cols] matrix at src+off is written as [cols, rows] at dst+dst_off (v111: the copies have a compact buffer of
 * their own — by default only the W_o^T matrices are kept).  `descs_device` is a DEVICE array (built once),
 * tile_start = running sum of ceil(rows/64)*ceil(cols/64), total_tiles = the final sum. */
typedef struct {
    long off;       /* element offset of the matrix in the source buffer */
    int rows, cols;
    int tile_start;
    int reserved;
    long dst_off;   /* element offset of the transposed copy in dst */
} mtn_transpose_desc;
int mtn_transpose_group(int dtype, const void* src, void* dst, const mtn_transpose_desc* descs_device, int count,
                        int total_tiles, void* stream);

/* ------------------------------------------------------------------------------------------
 * Optimiser: Adam(betas=(0.9,0.98), eps=1e-9) under the Noam schedule
 * (train.py:190, data_utils.py:92-117), fused over ONE flat parameter buffer.
 *   state (device, 8 floats): [0]=step [1]=lr [2]=1-b1^t [3]=1-b2^t  (updated by mtn_noam_tick)
 *   mtn_adam_step: g *= grad_scale (optional float device scalar, e.g. 1/global_ntokens);
 *     m,v updated, p -= lr/bc1 * m / (sqrt(v)/sqrt(bc2) + eps); p_lp (optional) = cast(p).
 * ------------------------------------------------------------------------------------------ */
int mtn_noam_tick(float* state, float factor, int model_size, int warmup, float beta1, float beta2, void* stream);
int mtn_adam_step(int dtype, long n, float* p, const float* g, float* m, float* v, void* p_lp, const float* state,
                  const float* grad_scale, float beta1, float beta2, float eps, void* stream);
/* The same update over chunks [off[c], off[c]+len[c]) of the flat buffers (off, len: DEVICE arrays; multiples of 4, len <=
 * 4096): the parameters that the GEMM optimiser epilogue (mtn_adam_fuse) does not cover. */
int mtn_adam_step_chunks(int dtype, int n_chunks, const long* off, const int* len, float* p, const float* g, float* m, float* v,
                         void* p_lp, const float* state, const float* grad_scale, float beta1, float beta2, float eps, void* stream);

/* ------------------------------------------------------------------------------------------
 * Averaging in weight space (version 124; csrc/average.hip), over fp32 buffers of n elements.  Stream-ordered, capturable into a
 * hipGraph; nothing is allocated or synchronised.  Base pointers are 16-byte aligned; nothing outside [0, n) is touched.
 *   mtn_lerp_f32: acc[i] = acc[i] + coef * (x[i] - acc[i]) as THREE separately rounded fp32 operations (subtract, multiply, add; never
 *     an fma), so that numpy float32 reproduces it bit for bit.  x is read only.  The running mean of K inputs is K calls with
 *     coef = w_k / (w_1 + ... + w_k).
 *   mtn_ema_step: the same arithmetic with x = p and the coefficient computed on the device from the optimiser state mtn_noam_tick
 *     maintains: t = state[0] (the step number after the tick: 1 on the first step), c = max(1 - decay, 9 / (10 + t)) in fp32, which is
 *     1 - min(decay, (1 + t) / (10 + t)) — the usual warm-up, so that early steps do not pin the average to the initial weights.  Every
 *     thread computes c itself (no second launch); coef_out (optional device float) receives it.  p and state are read only.
 *   mtn_swap_f32: a[i] <-> b[i] in one pass.
 * MTN_ERR_ARG, nothing launched: n < 0; a null or misaligned pointer (coef_out may be NULL); acc == x, ema == p or a == b; coef outside
 * [0, 1] or not finite; decay outside [0, 1) or not finite.  n == 0 returns MTN_OK with nothing launched.
 * ------------------------------------------------------------------------------------------ */
int mtn_lerp_f32(long n, float* acc, const float* x, float coef, void* stream);
int mtn_ema_step(long n, float* ema, const float* p, const float* state, float decay, float* coef_out, void* stream);
int mtn_swap_f32(long n, float* a, float* b, void* stream);

/* ------------------------------------------------------------------------------------------
 * Gradient clipping by global norm (csrc/gradnorm.hip; detected by symbol, version 125): torch.nn.utils.clip_grad_norm_'s arithmetic over ONE flat fp32
 * gradient buffer, left in device memory where mtn_adam_step reads it as grad_scale.  Stream-ordered, capturable into a hipGraph;
 * nothing is allocated, no atomics, no host read.  Every sum is taken in an order that is a pure function of n (never of the device),
 * so two launches over the same bytes give the same bytes.
 *   mtn_grad_sumsq_partials(n): how many doubles mtn_grad_sumsq writes for a buffer of n floats: min(2048, ceil((n / 4) / 256)), at
 *     least 1; 0 for n <= 0.  Host, a pure function of n.
 *   mtn_grad_sumsq: partial[b] = the sum over workgroup b's elements of (double)g[i] * (double)g[i], accumulated in double (the product
 *     of two floats is exact there, so magnitudes whose square leaves fp32's range, 1e-25 or 1e25, keep their norm).  Workgroup b of G =
 *     mtn_grad_sumsq_partials(n), thread t of 256, takes the 16-byte vectors j = b * 256 + t, j + 256 G, ... below n / 4, each thread
 *     one chain in that order (x, y, z, w inside a vector); workgroup 0's threads t < n % 4 then add tail element (n / 4) * 4 + t.  The
 *     workgroup's total: xor butterfly over the 64 lanes (offsets 32, 16, ..., 1), then the four waves' totals in wave order.  g is
 *     read only.
 *   mtn_clip_scale (one workgroup): thread t sums partial[t], partial[t + 256], ... in that order, the same tree adds the threads;
 *     norm = sqrt(sum) * |base| with base = *base_scale (1 when NULL); coef = min(1, max_norm / (norm + 1e-6)) in double
 *     (clip_grad_norm_'s definition, its 1e-6 included); *scale_out = (float)((double)base * coef), rounded once — and the base's own
 *     bits (1.0f without one) when coef == 1, so an unclipped step multiplies by exactly one.  max_norm = +inf measures and never
 *     clips.  A norm that is not finite: coef and *scale_out are NaN (Adam propagates it; error_if_nonfinite=False).  *norm_out
 *     (optional) = norm.  stats (optional device double[5]), updated by one thread with plain loads and stores (stream order keeps
 *     calls apart): [0] += norm and [1] = max([1], norm) when the norm is finite, [2] += 1, [3] += 1 when coef < 1, [4] += 1 when the
 *     norm is not finite.  scale_out may be base_scale itself (it is read first).
 * MTN_ERR_ARG, nothing launched: n <= 0; a null or misaligned pointer (g at 16 bytes, doubles at 8, floats at 4; base_scale, norm_out
 * and stats may be NULL); n_partial < 1 or above 2048; max_norm NaN or <= 0.
 * ------------------------------------------------------------------------------------------ */
int mtn_grad_sumsq_partials(long n);
int mtn_grad_sumsq(long n, const float* g, double* partial, void* stream);
int mtn_clip_scale(int n_partial, const double* partial, float max_norm, const float* base_scale, float* scale_out, double* norm_out,
                   double* stats, void* stream);

/* ------------------------------------------------------------------------------------------
 * Gradient accumulation over a window of K micro-batches (csrc/gradaccum.hip; detected by symbol, version 125).  Micro-step k leaves
 * its gradient g_k in the flat fp32 gradient buffer, normalised by its own token counts, and w_k is its target-token count over all
 * ranks (a device float).  The window's gradient is
 *     G = (sum_k w_k g_k) / (sum_k w_k),
 * the gradient of the token-weighted mean of the micro-steps' losses.  For the main decoder stream that is the gradient of the step on
 * the concatenated batch; for the auto-encoder streams it is that gradient when the micro-batches share their query-to-target token
 * ratio — otherwise a micro-batch's auto-encoder term carries the weight w_k / sum w and not its share of the query tokens.
 * One pass over n floats per micro-step: 16-byte accesses, mtn_grad_sumsq's grid (mtn_grad_sumsq_partials(n) workgroups of 256, a pure
 * function of n), workgroup 0's threads t < n % 4 take the tail.  Stream-ordered, capturable, nothing allocated, no atomics, no host
 * read.  Every operation below is ONE separately rounded fp32 operation, never an fma: numpy float32 reproduces the bytes.  w = *w.
 *   MTN_ACCUM_FIRST: acc[i] = w * g[i];                       *total_out = w;              total_in is ignored.
 *   MTN_ACCUM_ADD:   acc[i] = acc[i] + w * g[i];              *total_out = *total_in + w.  (a multiply, then an add)
 *   MTN_ACCUM_LAST:  t = *total_in + w;  inv = (float)(1.0 / (double)t), computed by every thread;
 *                    g[i] = (acc[i] + w * g[i]) * inv;        *total_out = t.               acc is read only.
 *     With partial non-NULL the launch also writes, from the g it has just written, the mtn_grad_sumsq_partials(n) doubles
 *     mtn_grad_sumsq would: each thread's chain in that kernel's order, the same workgroup tree, the same bytes.
 * g is written in LAST only.  One thread of workgroup 0 stores *total_out with a plain store while every thread reads *total_in: they
 * are different floats (the caller alternates two slots).  The caller guarantees t > 0: a zero total gives inf / NaN as the arithmetic
 * says; nothing is checked on the device.
 * MTN_ERR_ARG, nothing launched: another mode; n < 0; acc or g null or not 16-byte aligned; acc == g; w or total_out null; w, total_in
 * or total_out not 4-byte aligned; total_in null outside FIRST; total_out == total_in or == w; partial not 8-byte aligned, or non-NULL
 * outside LAST.  n == 0 returns MTN_OK with nothing launched.
 * ------------------------------------------------------------------------------------------ */
#define MTN_ACCUM_FIRST 0
#define MTN_ACCUM_ADD 1
#define MTN_ACCUM_LAST 2
int mtn_grad_accum(int mode, long n, float* acc, float* g, const float* w, const float* total_in, float* total_out, double* partial,
                   void* stream);

/* ------------------------------------------------------------------------------------------
 * Scheduled sampling, the token mix (csrc/sched.hip; detected by symbol, version 125): the two-pass, parallel form (Mihaylova & Martins
 * 2019; Duckworth et al. 2019).  logits [B * T, ldx] (fp32, row stride ldx >= V; columns V..ldx-1 are never read) are the generator's rows
 * of a teacher-forced pass over the gold decoder inputs trg [B, T]; row (b, t - 1) predicts trg[b][t].  One launch writes mixed [B, T]:
 * a copy of trg in which a fraction p of the positions holds the model's own prediction.  tests/sched_refs.py is the definition in numpy.
 *   step     = state[0], the optimiser's device state (the step number mtn_noam_tick maintains, a float holding an integer); only
 *              state[0] is read.
 *   p        = p_max * min(1, max(0, step - start) / ramp) in fp32: a subtract, a max, a divide, a min and a multiply, each rounded
 *              separately (no fma), start and ramp converted to float.  ramp == 0: p = p_max when step >= start, else 0.
 *   coin     u = (sample_hash(seed + (uint64)step, ((uint64)key[b] << 12) | t, 0xFFFFFFFF) >> 8) * 2^-24 (exact in fp32; sample_hash is
 *              mtn_sample_rows' counter hash, csrc/common.h).  Position (b, t) is ELIGIBLE iff t >= 1 and trg[b][t] != pad; it is
 *              replaced iff it is eligible, u < p, and its row yields a pick (below).  Everywhere else mixed[b][t] = trg[b][t].
 *   pick     over the columns c of row (b, t - 1) with c != pad and c not among banned[0..n_banned-1]:
 *     MTN_SCHED_ARGMAX  the score is s_c = z_c;
 *     MTN_SCHED_SAMPLE  Gumbel-max, one pass, no CDF scan: s_c = z_c * inv_temperature + g_c (a multiply, then an add),
 *              g_c = -log(-log(u_c)), u_c = ((sample_hash(the coin's seed, the coin's key, c) >> 8) + 0.5) * 2^-24, which lies strictly
 *              inside (0, 1).  With k = hash >> 8: for k < 2^23, u_c is exact in fp32 and w_c = -logf(u_c); for k >= 2^23, u_c is not an
 *              fp32 number (rounded it would reach 1 at k = 2^24 - 1), but v_c = 1 - u_c = ((2^24 - 1 - k) + 0.5) * 2^-24 is, and
 *              w_c = -log1pf(-v_c); then g_c = -logf(w_c).  V < 2^24, so the coin's position word 0xFFFFFFFF collides with no column.
 *     The largest s_c wins, ties to the lowest c (-inf scores take part: a row of -inf picks its lowest admitted column).  A row with
 *     every column excluded, or with a NaN among its admitted scores, yields no pick: the gold token stays and the position does not
 *     count as replaced.  The mix never writes pad or a banned id, and never changes a pad position.
 *   stats    3 unsigned 64-bit counters, accumulated (atomic adds; zero them to start a count): [0] += eligible positions,
 *            [1] += replaced positions, [2] += replaced positions whose pick != trg[b][t].
 *   pick_score (optional, [B, T] fp32): s of the winning column at a replaced position, NaN elsewhere.
 * One workgroup of 256 threads per (b, t); the coin is evaluated first, uniformly, and a kept position returns without touching its
 * logits row.  A replaced row is read once, with 16-byte loads when the row starts at a 16-byte boundary and scalar loads otherwise.
 * Stream-ordered, capturable; nothing allocated, no host read.  seed is a host scalar: draws differ between replays because step does.
 * MTN_ERR_ARG, nothing launched: a null pointer (pick_score may be NULL) or a misaligned one (logits, state, pick_score at 4 bytes, the
 * rest at 8); mixed == trg (the gold ids must survive replays); B or T negative; T >= 4096; V < 1 or V >= 2^24; ldx < V; pick neither
 * MTN_SCHED_ARGMAX nor MTN_SCHED_SAMPLE; p_max outside [0, 1] or NaN; start or ramp negative; n_banned outside [0, 4];
 * inv_temperature not finite or <= 0.  B == 0 or T == 0 returns MTN_OK with nothing launched.
 * ------------------------------------------------------------------------------------------ */
#define MTN_SCHED_ARGMAX 0
#define MTN_SCHED_SAMPLE 1
typedef struct {
    int B, T, V; long ldx;
    const float* logits;              /* device: [B * T, ldx] */
    const long* trg;                  /* device: [B, T] */
    const long* key;                  /* device: [B] */
    const float* state;               /* device: the optimiser state, [0] = step */
    long pad; int n_banned; int banned[4];
    float p_max; int start, ramp;
    int pick; float inv_temperature; long seed;
    long* mixed;                      /* device: [B, T], not trg */
    unsigned long long* stats;        /* device: 3 */
    float* pick_score;                /* device: [B, T], or NULL */
} mtn_sched_args;
int mtn_sched_mix(const mtn_sched_args* args /* host */, void* stream);

/* ------------------------------------------------------------------------------------------
 * Device-side batch assembly (replaces the host padding of data_handler.py:206-274 `make_batch` and the mask passes of
 * data_utils.py:23-54 `Batch`).  The corpus stays resident in HBM: each token field as one flat int64 buffer with per-item
 * start/len tables, each feature type as one flat [frames, F] float buffer with per-video start/len tables.  A batch is
 * the list of item ids (`ids`, device int32[B]; NULL = items 0..B-1).
 *   tokens  : out[b,l] = l < len ? flat[start+l] : pad; mask[b,l] = (out != pad); std_mask[b,i,j] = (out[b,j] != pad) &
 *             (j <= i) (optional, data_utils.py:48-54); *n_nonpad += #non-pad (optional, data_utils.py:45; zero it first).
 *             len = min(item length, L, row_len[b] if row_len and row_len[b] >= 0): row_len cuts rows short (the reference's
 *             random answer truncation, data_handler.py:255-260); out, mask, std_mask and n_nonpad all follow that len.
 *   features: frames start, start+skip, ...; out[b,v,:] = frame if it exists and has any element != 1, else 0;
 *             mask[b,v] = that validity (the reference pads with ones, detects all-ones frames, then zeroes them).
 * ------------------------------------------------------------------------------------------ */
#define MTN_ASSEMBLE_MAX_GROUP 8
typedef struct {
    const int64_t* flat;  /* all items of this field, concatenated */
    const int64_t* start; /* [n_items] offset of each item in flat */
    const int32_t* len;   /* [n_items] */
    const int32_t* ids;   /* [B] items of this batch, or NULL */
    int B, L;             /* L = padded length (>= longest item of the batch; longer items are cut) */
    int64_t pad;
    int64_t* out;         /* [B, L] */
    uint8_t* mask;        /* [B, L] or NULL */
    uint8_t* std_mask;    /* [B, L, L] or NULL */
    int64_t* n_nonpad;    /* scalar accumulator or NULL */
    const int32_t* row_len; /* [B] cap of each row's length (< 0: no cap), or NULL (since version 114) */
} mtn_assemble_tokens_desc;
int mtn_assemble_tokens(int count, const mtn_assemble_tokens_desc* descs /* host array */, void* stream);
typedef struct {
    const float* flat;    /* [total_frames, F] */
    const int64_t* start; /* [n_videos] first frame of each video */
    const int32_t* len;   /* [n_videos] frames per video */
    const int32_t* ids;   /* [B] videos of this batch, or NULL */
    int B, V, F, skip;    /* V = padded frame count; skip >= 1 (every skip-th frame, data_handler.py:233) */
    float* out;           /* [B, V, F] */
    uint8_t* mask;        /* [B, V] or NULL */
} mtn_assemble_features_desc;
int mtn_assemble_features(int count, const mtn_assemble_features_desc* descs /* host array */, void* stream);

/* ------------------------------------------------------------------------------------------
 * Candidate selection of the beam search (data_utils.py:219 argsorts each hypothesis' vocabulary row on the host).
 * Per row of x [rows, V] (row stride ldx): the k largest entries in descending order (equal values: ascending column),
 * packed as out[row] = { k values, k column indices as floats, x[row][extra_col] } (2k+1 floats; extra_col < 0: 0).
 * 1 <= k <= 16, V < 2^24.
 * ------------------------------------------------------------------------------------------ */
int mtn_topk_rows(const float* x, int rows, int V, long ldx, int k, int extra_col, float* out, void* stream);
/* One step of the beam search's hypothesis bookkeeping on the device (round 5, version 112; data_utils.py:209-240 — the loop body behind
 * `model.decode`): from the rows' heads left by mtn_topk_rows (k_top values, k_top columns, the <eos> column's value per live hypothesis)
 * build the new beam exactly as the reference does (hypotheses in order, candidates in descending log-probability, <unk> / <eos>
 * skipped, the worst member replaced while a candidate beats it), WRITE what the next mtn_decode_step reads (newest tokens, ancestor
 * table, position) and LOG the step for the host: log_* are [L][dialogues * width] (log_n_*: [L][dialogues]); log_done holds
 * lp + logp[<eos>] + penalty * (length + 1) of every hypothesis alive at a step >= min_len.  flags[0] is raised when a row's head holds
 * an exact tie (the reference's order then comes from the full row: re-run that search on the host path).  width <= 16.
 * State (zeroed / initialised by the caller per search): lp [dialogues * width] doubles, n_live / step [dialogues]. */
typedef struct {
    int dialogues, width, L, k_top, k, beam, unk, eos, pad, min_len;
    double penalty;
    const float* top;           /* [dialogues * width][2 * k_top + 1] */
    long* tokens; int* pos; int* anc;             /* as mtn_decode_args */
    double* lp; int* n_live; int* step; int* flags;
    int* log_parent; int* log_tok; double* log_score; double* log_done; int* log_n_old; int* log_n_new;
} mtn_beam_args;
int mtn_beam_advance(const mtn_beam_args* args /* host */, void* stream);
/* Diverse (group) beam search, Hamming diversity (version 119; Vijayakumar et al. 2016): one step of the hypothesis bookkeeping where the
 * beam of B hypotheses of a dialogue is split into G groups of B' = B / G.  It extends mtn_beam_advance above (data_utils.py:209-240) and
 * stands in its place in a captured search, one launch per token (csrc/diverse.hip).
 *   Row layout    group g of dialogue d owns rows d*B + g*B' .. + B'-1 of the session (the session width stays B); every group starts from
 *                 one <sos> hypothesis in its first row.
 *   Group order   at a step the groups of a dialogue are processed in order g = 0 .. G-1.
 *   Counts        c_g[v] = number of hypotheses in the FINAL new beams of groups 0 .. g-1 at this step whose newest token is v, counted
 *                 with multiplicity; a candidate that entered a beam and was replaced later in the same walk does not count.
 *   Penalised row group g reads, for each of its live hypotheses, r'[v] = fl32(r[v] - fl32(fl32(lambda) * (float)c_g[v])): one fp32
 *                 multiply and one fp32 subtract, never contracted into an fma.  r is the row after mtn_constrain_rows, if one runs.
 *   Group step    exactly mtn_beam_advance's step on the group's own hypotheses with beam B': candidates in descending r', <unk> / <eos>
 *                 never extend a hypothesis, the worst member replaced while a candidate beats it, double sums rounded to float32.
 *   Finished      log_done uses r[<eos>]: <eos> is never an extension, so its count is always 0.
 *   Scores        accumulate the penalised values (as under a repetition penalty); rows are not renormalised.
 *   Ties          two equal values among the k_top entries of a live row's head, before the penalty or after it, raise flags[0]: the
 *                 visiting order is then the reference's argsort of the full PENALISED row (re-run that search on the host path).
 * Why the head suffices: group g penalises at most B - B' tokens, so at least B' + 2 of the B + 2 largest entries of r keep their value, and
 * everything outside the head is <= them before and after the penalty: the B' winners and the two skipped symbols of a row lie inside the
 * head mtn_topk_rows delivers for a plain search at the same beam.  The kernel penalises the k_top head entries, re-sorts them (stable,
 * descending) and walks the first k of them (k = B' + 2).
 * beam.dialogues = D * G pseudo-dialogues, beam.width = beam.beam = B': state and step log are written in mtn_beam_advance's layout for
 * D * G dialogues of width B' (n_live / step / log_n_* one entry per group, log parents relative to the group's first row), so a host
 * rebuild and mtn_constrain_rows' step-log walk (width = rows_per_step = B') read them as they are.  One workgroup per REAL dialogue walks
 * its groups in order; parents never cross groups; *pos is written once.  groups = 1 is mtn_beam_advance, bit for bit.
 * MTN_ERR_ARG (nothing is launched): a null buffer, groups < 1, dialogues no multiple of groups, width * groups > 16,
 * k_top < width * groups + 3 (B + 2 entries and the tie sentinel) or > 16, k outside [1, k_top], diversity negative or not finite. */
typedef struct {
    mtn_beam_args beam;
    int groups; float diversity;
} mtn_diverse_args;
int mtn_diverse_advance(const mtn_diverse_args* args /* host */, void* stream);
/* Sampling decode (version 115): one drawn token per row of logp [rows, V] (fp32 log-probabilities, row stride ldx; ldx = 0: every row
 * reads the same distribution; V < 2^24), one workgroup per row.  With l = step[row], the row's position:
 *   1. ban     the n_banned <= 4 ids in banned[], and eos while l < min_len, get probability 0;
 *   2. T       p_i ~ exp((logp_i - max) / temperature), temperature > 0 (max over what is not banned);
 *   3. top-k   top_k = 0 (or >= V): off; otherwise keep every token whose logp is >= the k-th largest — ties at the threshold are
 *              all kept, so the kept set depends on no sort order; any k up to V;
 *   4. top-p   top_p = 1: off; otherwise, over what top-k kept, keep { i : p_i >= t* }, t* the largest threshold whose kept mass is
 *              >= top_p x the mass — ties all kept;
 *   5. draw    u = (hash(seed, key[row], l) >> 8) / 2^24, a pure integer counter hash (csrc/sample.hip sample_hash); the token is the
 *              first kept index, in vocabulary order, whose running kept mass exceeds u x kept mass.  The arg-max of what is not
 *              banned is always kept, so a draw always exists.
 * seed, key and step are DEVICE memory (kernel arguments are frozen into a captured graph; one graph serves every search of a shape).
 * Per row the call logs, at [l][row] of the [L][rows] logs, the token, logp[token] (the model's log-probability, not the filtered
 * one) and u, and sets step[row] = l + 1; a row whose step is outside [0, L) is left alone.  With tokens / pos / anc (as
 * mtn_decode_args; each may be NULL) it also writes what the next mtn_decode_step reads: tokens[row] = the token,
 * anc[row][l + 1] = row (identity ancestors), *pos = l + 1.  Rows go on after <eos>: the caller cuts there. */
typedef struct {
    int rows, V; long ldx;
    const float* logp;
    float temperature; int top_k; float top_p;
    int n_banned; int banned[4]; int eos, min_len;
    const long* seed;           /* device: 1 */
    const long* key;            /* device: [rows] */
    int* step;                  /* device: [rows] */
    int L;
    int* log_tok; float* log_logp; float* log_u;  /* device: [L][rows] */
    long* tokens; int* pos; int* anc;             /* as mtn_decode_args, or NULL */
} mtn_sample_args;
int mtn_sample_rows(const mtn_sample_args* args /* host */, void* stream);
/* Contrastive search (csrc/contrastive.hip; detected by symbol, mtn_version() stays 125; Su et al. 2022, "A Contrastive Framework for
 * Neural Text Generation"; not in the reference): among the k most probable next tokens, take the one whose decoder state is least similar
 * to the states of the prefix.  This call is the selection and bookkeeping of ONE generated token; it reads the output of the decoder's
 * final norm, which no other entry point looks at.
 * A dialogue owns k consecutive session rows (rows dialogue * k ..).  At position l = step[dialogue] >= 1 every row r holds the common
 * prefix <sos>, y_1 .. y_{l-1} at positions 0 .. l-1 of tokens and its own candidate token v_r at position l; v_r was the r-th admitted
 * entry of the previous step's head and cand_logp[r] is that entry's log-probability.  With h[r][j] = hidden[row r][position j][0..d):
 *   pen_r = max over 0 <= j < l of  dot(h[r][l], h[r][j]) / ( sqrt(|h[r][l]|^2) * sqrt(|h[r][j]|^2) )     (0 when either norm is 0)
 *   s_r   = fl32( fl32((1 - alpha) * expf(cand_logp[r])) - fl32(alpha * pen_r) )        (two multiplies and a subtract, never an fma)
 *   r*    = the row of largest s_r, ties to the lowest row
 * A row whose s_r is NaN (a NaN cosine makes pen_r NaN), or whose cand_logp is -inf, never wins; if no row can win, r* is row 0.
 * Everything is fp32, and the order of every sum is a pure function of d (the same on the 16-byte and the scalar path), so two launches
 * give the same bytes.  y_l = v_{r*}; the step logs, at [l][dialogue] of the [L][dialogues] logs, y_l, cand_logp[r*] (the model's own
 * log-probability, with the bits of the head entry), pen_{r*} and r*.  Then:
 *   - y_l is stored at position l of all k rows; y_l == eos sets done[dialogue];
 *   - otherwise, while l + 1 < L, the candidates for position l + 1 are the first k ADMITTED entries of row r*'s head, in the head's
 *     order.  The head is what mtn_topk_rows leaves in top for the next-token row of row r*: k_top values, k_top columns (as floats), one
 *     more word.  An entry is not admitted if its id is one of banned[0..n_banned), or if it is eos while l < min_len.  Row r gets the r-th
 *     admitted entry's column at position l + 1 and its value as cand_logp[r]; with fewer than k admitted entries the remaining rows
 *     repeat the last admitted column with cand_logp = -inf (k_top >= min(16, k + n_banned + 1) admits at least one; were none admitted,
 *     they would repeat the head's first column);
 *   - step[dialogue] = l + 1, and workgroup 0 stores *pos = min(max(l + 1, 0), L - 1), what the next decoder pass reads.
 * l == 0 is the bootstrap: nothing is scored or logged, r* is the dialogue's first row, and candidates for position 1 are dealt from its
 * head.  A dialogue that is done, or whose step is outside [0, L), only advances its step.
 * The response is y_1 .. up to eos, at most L - 1 tokens without one.  alpha = 0 is greedy (the head is sorted: row 0 wins), and so is
 * k = 1 for every alpha.
 * One launch, one workgroup per dialogue, which reads and writes only its own dialogue's words; no atomics, nothing allocated, no host
 * read: capturable.  16-byte loads where d and both strides are multiples of 4 and hidden is 16-byte aligned, scalar loads otherwise.
 * MTN_ERR_ARG, nothing launched: a null pointer; hidden, top, cand_logp, step, done or a log not 4-byte aligned, tokens or pos not 8-byte
 * aligned; k outside 1..16, k_top outside min(16, k + n_banned + 1)..16, d outside 1..1024, L outside 1..2^20, n_banned outside 0..4;
 * alpha outside [0, 1] or not finite; pos_stride < d or row_stride < (L - 1) * pos_stride + d (the dense strides, d and L * d, at
 * least); dialogues < 0 or dialogues * k overflowing int.  dialogues == 0 returns MTN_OK with nothing launched. */
typedef struct {
    int dialogues, k, L, d, k_top;
    float alpha;
    int eos, min_len;
    int n_banned; int banned[4];
    const float* hidden;        /* device: [dialogues * k][L][d] through the strides below */
    long row_stride, pos_stride;    /* in elements */
    const float* top;           /* device: [dialogues * k][2 * k_top + 1], as mtn_topk_rows leaves it */
    long* tokens;               /* device: [dialogues * k][L] */
    long* pos;                  /* device: 1 */
    float* cand_logp;           /* device: [dialogues * k] */
    int* step;                  /* device: [dialogues] */
    int* done;                  /* device: [dialogues] */
    int* log_tok; float* log_logp; float* log_pen; int* log_rank;   /* device: [L][dialogues] */
} mtn_contrastive_args;
int mtn_contrastive_advance(const mtn_contrastive_args* args /* host */, void* stream);
/* Candidate scoring (version 116): how likely the model finds GIVEN tokens.  logits [n_seq * L, ldz] (fp32, row stride ldz >= V; columns
 * V..ldz-1 are never read; 2 <= V < 2^24) are the generator's rows of a teacher-forced pass, target [n_seq, L] the token each position
 * should produce.  One launch, no atomics; per position (s, l), with z its row and t = target[s][l]:
 *   tok_logp[s][l] = z[t] - logsumexp(z[0..V-1])     (max-shifted, fp32)
 *   tok_rank[s][l] = #{c : z[c] > z[t]} + #{c < t : z[c] == z[t]}     (0: t is the arg-max; equal values rank by ascending column, the
 *                    order mtn_topk_rows documents)
 * A position whose target is `pad`, or lies outside [0, V), gets tok_logp = 0, tok_rank = -1 and is not counted.  Per sequence:
 *   seq_logp[s] = sum of tok_logp[s][0..L-1] in ascending position, accumulated in double by one lane (the same bits in every run)
 *   seq_len[s]  = number of counted positions
 * A finished beam hypothesis' score (mtn_beam_args log_done; data_utils.py:211-215) is seq_logp + penalty * seq_len when target is the
 * hypothesis followed by <eos>. */
typedef struct {
    int n_seq, L, V, pad; long ldz;
    const float* logits;        /* [n_seq * L][ldz] */
    const long* target;         /* [n_seq][L] */
    float* tok_logp;            /* [n_seq][L] */
    int* tok_rank;              /* [n_seq][L] */
    double* seq_logp;           /* [n_seq] */
    int* seq_len;               /* [n_seq] */
} mtn_score_args;
int mtn_score_rows(const mtn_score_args* args /* host */, void* stream);
/* Constrained decoding (version 117): rewrite each row of logp [rows, V] (fp32 log-probabilities, row stride ldx >= V; V < 2^24) from
 * the history of the row's own hypothesis, before a selection launch (mtn_topk_rows, mtn_sample_rows) reads it.  One launch, one workgroup
 * per row, no atomics; out [rows, V] (row stride ldo >= V) may BE logp (then only the constrained columns are written), otherwise the
 * two must not overlap.
 * History h[0..n-1]: the tokens the hypothesis has generated, oldest first, without <sos>; n <= L <= 1024.  Two sources:
 *   explicit   hist != NULL: h = hist[row][0..n-1], n = hist_len[row] clamped to [0, L] (row stride ldh >= L);
 *   step log   hist == NULL: the logs mtn_beam_advance / mtn_sample_rows write, log_tok / log_parent [L][rows] (parents relative to the
 *              first row of the dialogue, i.e. of the row's group of `width` rows; log_parent NULL: every row is its own parent).  With
 *              n = step[row / rows_per_step] clamped to [0, L] (rows_per_step = width where a dialogue has one step counter, 1 where
 *              every row has its own), base = row - row % width and r = row % width:
 *                  for j = n-1 .. 0:  h[j] = log_tok[j][base + r];  r = log_parent[j][base + r] clamped to [0, width)
 *              — how the host rebuilds a hypothesis from the log.  Rows past a dialogue's live count read stale entries: harmless, their
 *              output is never read.  rows is a multiple of width, width <= 16.
 *   hist, hist_len, the logs and step are DEVICE memory (kernel arguments are frozen into a captured graph; these change per step).
 * Transform:
 *   1. penalty  theta >= 1 (1: off): for every DISTINCT token c of h, out[c] = logp[c] * theta — one fp32 multiply, applied once however
 *               often c occurs.  Log-probabilities are <= 0, so this lowers them.  The row is NOT renormalised: scores, finished scores and
 *               logged logp values of a search under a penalty are the penalised ones (mtn_sample_rows normalises over its kept set anyway).
 *   2. n-gram   ngram = N in [1, 8] (0: off): for every j in [0, n - N] with h[j .. j+N-2] == h[n-N+1 .. n-1], out[h[j+N-1]] = -inf: no
 *               N-gram of the history can occur a second time.  N = 1 bans every token of h.  A ban overrides the penalty.
 *   3. every other column is copied bit for bit.
 * A token of h outside [0, V) takes part in the comparisons of 2 but names no column: nothing is written for it.  Banned columns are
 * -inf: mtn_topk_rows sorts them last (they never enter a head while k finite columns exist) and mtn_sample_rows never draws them. */
typedef struct {
    int rows, V; long ldx, ldo;
    const float* logp; float* out;
    int ngram; float theta;
    int L;
    const int* hist; long ldh; const int* hist_len;               /* device: [rows][ldh], [rows]; or hist = NULL */
    const int* log_tok; const int* log_parent; const int* step;   /* device: [L][rows] (log_parent may be NULL), [rows / rows_per_step] */
    int width, rows_per_step;
} mtn_constrain_args;
int mtn_constrain_rows(const mtn_constrain_args* args /* host */, void* stream);
/* Ensemble decoding (version 118): combine the rows of M checkpoints, 1 <= M <= 8, into one row of log-probabilities that the selection
 * launches above read as they read a single model's.  x[m] is member m's row matrix [rows, V] (fp32, row stride ld[m] >= V; V < 2^24):
 * logits or log-probabilities — every member row is normalised here, with lse_m = logsumexp over c of x_m[c].  w[m] >= 0 are the weights;
 * the caller has normalised them to sum 1.  One launch, one workgroup per row, fixed reduction order, no atomics: two launches give the
 * same bits.  out [rows, V] (row stride ldo >= V) must not overlap any input.
 *   mode 0, prob     out[c] = log sum_m w_m exp(x_m[c] - lse_m): the arithmetic mean of the members' probabilities, evaluated as
 *                    max_m a_m + log sum_m exp(a_m - max_m a_m) with a_m = log w_m + x_m[c] - lse_m.  Normalised as it stands.
 *   mode 1, logprob  s[c] = sum over the m with w_m > 0 of w_m (x_m[c] - lse_m); out[c] = s[c] - logsumexp over c of s[c]: the weighted
 *                    geometric mean, renormalised.
 * A member with w_m == 0 contributes nothing in either mode, even where its entry is -inf (it is never read: no 0 * inf).  prob: a -inf
 * entry contributes 0, and a column that is -inf in every weighted member gives -inf.  logprob: a -inf entry in any weighted member gives
 * -inf.  Every weighted member row must hold at least one finite entry; this is NOT checked (the rows are device memory).
 * MTN_ERR_ARG: a null pointer, M outside 1..8, ld or ldo < V, V >= 2^24, a negative or non-finite weight, all weights 0, another mode. */
typedef struct {
    int rows, V, M, mode;
    const float* x[8]; long ld[8]; float w[8];
    float* out; long ldo;
} mtn_ensemble_args;
int mtn_ensemble_rows(const mtn_ensemble_args* args /* host */, void* stream);
/* Minimum-Bayes-risk selection (version 121; not in the reference, like sampling): of the K <= MTN_MBR_MAX_HYP hypotheses of a set — the
 * samples or the n-best list of a dialogue — answer with the one that agrees most, in n-grams, with the others (csrc/mbr.hip).  A hypothesis
 * is a list of token ids without <sos> / <eos>; tokens compare as int32, any value.  For hypotheses h, r and an order n:
 *   c_n(h)    = max(len(h) - n + 1, 0)
 *   m_n(h, r) = the clipped n-gram match count: the sum over distinct n-grams g of min(count of g in h, count of g in r)
 * and for the maximum order N in 1..4:
 *   F_n(h, r) = (double)(2 m_n) / (double)(c_n(h) + c_n(r)), exactly 0.0 when that denominator is 0
 *   U(h, r)   = (F_1 + F_2 + .. + F_N) / (double)N, the additions in ascending n starting from 0.0
 * U is symmetric and lies in [0, 1]; U(h, h) = min(len(h), N) / N; an empty hypothesis has U = 0 with everything, itself included.
 * With weights w (doubles; finite), over the n_hyp valid hypotheses of the set:
 *   expected[i] = sum_j w_j U(h_i, h_j) in ascending j, self included, from 0.0: one multiply then one add per step, never an fma
 *   best        = the index of the largest expected value, the lower index among equals (-1 when n_hyp = 0)
 *   order[rank_i] = i with rank_i = #{j : expected[j] > expected[i], or expected[j] == expected[i] and j < i}
 * Every operation is integer or a single IEEE double operation in this order: a host implementation that follows it agrees bit for bit.
 * An index >= n_hyp gets expected = -1.0, follows the valid ones in `order` by ascending index, and its rows and columns of util are 0.0.
 * Two sources of hypotheses (all pointers are DEVICE memory: kernel arguments are frozen into a captured graph):
 *   explicit    tok != NULL: tok [sets][K][ldl] int32, len [sets][K] clamped to [0, L], n_hyp [sets] clamped to [0, K], w [sets][K] or
 *               NULL = uniform, w_j = 1.0 / (double)n_hyp;
 *   sample log  tok == NULL: set s owns columns s*K .. s*K+K-1 of log_tok [L][sets * K], the token log mtn_sample_rows writes; a
 *               hypothesis is its column's tokens before the first `eos`, the first L - 1 tokens without one (the cut
 *               mtn_amd/decode.py sample_decode_many makes); n_hyp = K; len, n_hyp and ldl are not read; w as above.
 * One launch, one workgroup per set, fixed reduction order, no float atomics: two launches give the same bits, and a set's outputs do not
 * depend on what other sets share the launch.  util [sets][K][K] (U of every pair) is optional.
 * MTN_ERR_ARG (nothing is launched): a null required buffer, sets < 1, K outside 1..16, L outside 1..128, N outside 1..4, ldl < L with
 * explicit hypotheses. */
#define MTN_MBR_MAX_HYP 16
typedef struct {
    int sets, K, L, N; long ldl;
    const int* tok; const int* len; const int* n_hyp;             /* device: explicit hypotheses, or tok = NULL */
    const double* w;                                              /* device: [sets][K], or NULL */
    const int* log_tok; int eos;                                  /* device: [L][sets * K], the sample log */
    double* expected; int* best; int* order;                      /* device: [sets][K], [sets], [sets][K] */
    double* util;                                                 /* device: [sets][K][K], or NULL */
} mtn_mbr_args;
int mtn_mbr_select(const mtn_mbr_args* args /* host */, void* stream);
/* Corpus metrics of generated responses (version 122; csrc/eval.hip): BLEU-1..4, ROUGE-L and CIDEr of Q items on the device.  The reference
 * scores with coco-caption on the host (run.sh stage 4, utils/evaluate.py); these are the numbers it prints, without METEOR, on token ids.
 * Item q is one hypothesis h of hyp_len[q] tokens (0..L) and n_ref[q] references (1..R, R <= MTN_EVAL_MAX_REF) of ref_len[q][r] tokens
 * (0..L), L <= 128.  Tokens compare as int32, any value; nothing is an index.  For orders n = 1..4: count_s(g) = the occurrences of the
 * n-gram g in sentence s, c_n(s) = max(len(s) - n + 1, 0).
 *   BLEU, per item (integers)   guess_n = c_n(h);  match_n = sum over distinct g of min(count_h(g), max_r count_r(g));
 *                               closest = the reference length l that minimises (|l - len(h)|, l): ties go to the shorter.
 *   BLEU, corpus                G_n, M_n, T = sum len(h), C = sum closest as int64 sums over the items;  p = 1;  for n = 1..4:
 *                               p = p * (M_n + 1e-15) / (G_n + 1e-9), Bleu_n = p^(1/n);  ratio = (T + 1e-15) / (C + 1e-9); where ratio < 1
 *                               every Bleu_n is multiplied by exp(1 - 1/ratio).
 *   ROUGE-L, per item           LCS(h, r) the longest-common-subsequence length;  P = max_r LCS / len(h), Rc = max_r LCS / len(r) (an empty
 *                               sentence gives 0), beta = 1.2;  score = (1 + beta^2) P Rc / (Rc + beta^2 P), 0 where P = 0 or Rc = 0.
 *                               The corpus value is the mean.
 *   document frequency          df(g) = the number of ITEMS whose reference set holds g at least once (not the number of references);
 *                               exact: two different n-grams never share a count.
 *   CIDEr, per item             idf(g) = ln Q - ln max(1, df(g)) (a hypothesis n-gram no reference holds has df 0);  v_s(g) = count_s(g) idf(g);
 *                               |s|_n = sqrt(sum_g v_s(g)^2) over the n-grams of order n;  sim_n(h, r) = sum over g in h of min(v_h(g), v_r(g)) v_r(g),
 *                               divided by |h|_n |r|_n where both are non-zero, then multiplied by exp(-(len h - len r)^2 / (2 * 6^2));
 *                               score = 10 * (1/4) sum_n (1/n_ref) sum_r sim_n(h, r).  The corpus value is the mean.  Q = 1, or a corpus in
 *                               which every n-gram occurs in every item, gives exactly 0.
 * Layout (all pointers DEVICE memory): hyp [Q][ldl], hyp_len [Q], ref [Q][R][ldl], ref_len [Q][R], n_ref [Q]; lengths are clamped to [0, L]
 * and n_ref to [1, R]; what lies past a length or past n_ref is never read as a token.  Outputs: stats [Q][10] = guess_1..4, match_1..4,
 * len(h), closest;  rouge [Q], cider [Q];  corpus [8] = Bleu_1..4, ROUGE_L, CIDEr, T, C;  optional df_of_ref [Q][R][L][4] = the df of the
 * n-gram that starts at each reference position, 0 where there is none.
 * workspace: the document-frequency table, owned by the caller — 16-byte aligned, at least mtn_eval_workspace_bytes(Q, R, L) bytes (0 for
 * sizes mtn_eval_metrics refuses); its contents before and after a call mean nothing.
 * Four launches on `stream` (clear, table, per item, reduction), no grid barrier.  Integers are exact; all floating point is double with
 * every sum across lanes in a fixed order; the table counts with integer atomics only: two calls give the same bytes, and an item's stats
 * and rouge do not depend on the other items (its cider does, through df and Q).
 * MTN_ERR_ARG (nothing is launched): a null required buffer, Q < 1, R outside 1..8, L outside 1..128, ldl < L, Q R L > 2^28, a workspace
 * that is null, misaligned or too small. */
#define MTN_EVAL_MAX_REF 8
typedef struct {
    int Q, R, L; long ldl;
    const int* hyp; const int* hyp_len;                           /* device: [Q][ldl], [Q] */
    const int* ref; const int* ref_len; const int* n_ref;         /* device: [Q][R][ldl], [Q][R], [Q] */
    void* workspace; long workspace_bytes;                        /* device */
    int* stats; double* rouge; double* cider; double* corpus;     /* device: [Q][10], [Q], [Q], [8] */
    int* df_of_ref;                                               /* device: [Q][R][L][4], or NULL */
} mtn_eval_args;
long mtn_eval_workspace_bytes(int Q, int R, int L);
int mtn_eval_metrics(const mtn_eval_args* args /* host */, void* stream);
/* Rewards against a FIXED reference corpus (version 125; csrc/scst.hip with the device code of mtn_eval_metrics, csrc/eval_common.h).
 * mtn_eval_metrics rebuilds its document-frequency table from the evaluated items on every call; a training loop scores a few sampled
 * rows per step against a corpus that never changes.  The corpus is Qc items laid out as mtn_eval_args' ref / ref_len / n_ref (ref
 * [Qc][R][ldl], the same clamping, R <= 8, L <= 128) and stays in device memory, untouched, as long as the table is used: the table's keys
 * point into it.
 *   mtn_eval_table_build   two launches (clear, table): the df table of mtn_eval_metrics over the Qc items, into `workspace` (16-byte
 *                          aligned, at least mtn_eval_workspace_bytes(Qc, R, L) bytes).  Reads none of the fields from N on.
 *   mtn_eval_score_rows    ONE launch, a workgroup per hypothesis: hyp [N][ldl] with hyp_len [N] (clamped to [0, L]); hypothesis n is
 *                          scored against the references of corpus item item[n] (device int32; any order, repeats allowed; clamped to
 *                          [0, Qc) on the device).  stats [N][10], rouge [N] and cider [N] are, definition for definition, the per-item
 *                          outputs of mtn_eval_metrics with Q = Qc and df = the corpus table's; with N = Qc, item[n] = n they are its bytes.
 *                          The launch reads the table and writes nothing into it; no atomics; all arithmetic is double with fixed-order
 *                          sums: two calls give the same bytes.  `workspace` must hold what mtn_eval_table_build left for the same
 *                          Qc, R, L, ldl and ref (not checked: device memory).
 * MTN_ERR_ARG (nothing is launched): a null required buffer, Qc < 1, R outside 1..8, L outside 1..128, ldl < L, Qc R L > 2^28, a workspace
 * that is null, misaligned or too small; for mtn_eval_score_rows also N < 1. */
typedef struct {
    int Qc, R, L; long ldl;
    const int* ref; const int* ref_len; const int* n_ref;         /* device: [Qc][R][ldl], [Qc][R], [Qc] */
    void* workspace; long workspace_bytes;                        /* device: the table */
    int N;
    const int* hyp; const int* hyp_len; const int* item;          /* device: [N][ldl], [N], [N] */
    int* stats; double* rouge; double* cider;                     /* device: [N][10], [N], [N] */
} mtn_eval_rows_args;
int mtn_eval_table_build(const mtn_eval_rows_args* args /* host */, void* stream);
int mtn_eval_score_rows(const mtn_eval_rows_args* args /* host */, void* stream);
/* Self-critical sequence training, the two launches between the sampling search and the train step (version 125; csrc/scst.hip).
 * mtn_scst_assemble: the sample log log_tok [L][rows] (as mtn_sample_rows writes it) -> teacher-forcing targets and reward inputs, one
 * launch, a wave per row.  Row r is cut at its first <eos>: n = the smallest l with log_tok[l][r] == eos, or L - 1 when there is none (a
 * row without <eos> keeps L - 1 tokens: decode.py sample_decode_many's rule); y = log_tok[0..n-1][r].  Written, T >= L and ldh >= L:
 *   trg   [rows][T] (int64)  = sos, y_0 .. y_{n-1}, then pad          trg_y [rows][T] (int64) = y_0 .. y_{n-1}, eos, then pad
 *   hyp   [rows][ldh] (int32) = y_0 .. y_{n-1}, then pad up to column L - 1 (columns L..ldh-1 are left alone);  hyp_len [rows] = n
 * MTN_ERR_ARG (nothing is launched): a null buffer, rows < 1, L < 1, T < L, ldh < L.
 * mtn_scst_advantage: rewards -> the signed row weights mtn_wlosshead reads, one launch.  reward [D][S] (double) is the reward of sample s of
 * dialogue d; b_ds = baseline[d] where `baseline` (double [D], e.g. the reward of the greedy response) is given, else the leave-one-out
 * mean of the other S - 1 rewards of dialogue d (Luo 2020): (sum over s' != s, ascending s', in double) / (S - 1).  Written:
 *   roww [D S][T] (float)   every target row of sample (d, s), i.e. roww[(d S + s) T + t] for all t: (float)(-(r_ds - b_ds))
 *   adv  [D][S]   (double, optional)   r_ds - b_ds
 *   mean_reward, mean_baseline (double device scalars)   (sum_d (sum_s x_ds)) / (D S), inner sums in ascending s, then ascending d
 * A dialogue whose rewards are equal (and whose partial sums are exact, as for S = 2) gets weights of magnitude 0.
 * MTN_ERR_ARG (nothing is launched): a null required buffer, D outside 1..1024, S outside 1..64, S < 2 without a baseline, T < 1. */
typedef struct {
    int rows, L, T;
    const int* log_tok;                 /* device: [L][rows] */
    int sos, eos, pad;
    long* trg; long* trg_y;             /* device: [rows][T] */
    int* hyp; long ldh; int* hyp_len;   /* device: [rows][ldh], [rows] */
} mtn_scst_assemble_args;
int mtn_scst_assemble(const mtn_scst_assemble_args* args /* host */, void* stream);
typedef struct {
    int D, S, T;
    const double* reward;               /* device: [D][S] */
    const double* baseline;             /* device: [D], or NULL = leave-one-out mean */
    float* roww;                        /* device: [D S][T] */
    double* adv;                        /* device: [D][S], or NULL */
    double* mean_reward; double* mean_baseline; /* device scalars */
} mtn_scst_advantage_args;
int mtn_scst_advantage(const mtn_scst_advantage_args* args /* host */, void* stream);
/* Generator (mtn.py:62-69) at inference: out[row][c] = x[row][c] - logsumexp(x[row][0..V-1]) over logit rows x [rows, V] (row
 * strides ldx / ldo; out may be x).  The logits themselves are one mtn_gemm (x W^T + b, fp32 out). */
int mtn_log_softmax_rows(const float* x, int rows, int V, long ldx, float* out, long ldo, void* stream);

/* ------------------------------------------------------------------------------------------
 * Measurement support (bench.py `roofline`): a census of the GEMM launches of one step.  Between mtn_census_begin() and
 * mtn_census_end() (returns the number of launches) every mtn_gemm call is recorded on the host (no device work, no
 * change to the launch); mtn_census_info() describes launch i — which kernel the dispatch picked, its workgroup count,
 * algorithmic FLOPs (2·M·N·K summed over the group) and algorithmic bytes (operands read once + outputs written once) —
 * and mtn_census_replay() re-issues it `reps` times on `stream` so the caller can bracket it with HIP events.  The replay
 * reuses the recorded device pointers: call it only while the model's buffers are alive (outputs are overwritten).
 * ------------------------------------------------------------------------------------------ */
typedef struct {
    int dtype, count, variant, workgroups;
    double flops, bytes;
    int M[4], N[4], K[4];               /* shapes of the first four problems of the group */
} mtn_census_launch;
int mtn_census_begin(void);
int mtn_census_end(void);
int mtn_census_info(int i, mtn_census_launch* out);
int mtn_census_replay(int i, int reps, void* stream);
const char* mtn_census_variant_name(int variant);
/* Achievable dense bf16 MFMA rate of this box (register-only MFMA issue on independent accumulator chains, synchronises on its
 * own events): the measured denominator bench.py reports beside the 2.5 PFLOP/s spec figure.  scratch: >= 2048*256 floats.
 * mtn_measure_mfma_peak: the better of the two instruction shapes; mtn_measure_mfma_peak_shapes (112): both — v_mfma_f32_16x16x32_bf16
 * (the shape the path's kernels issue) and v_mfma_f32_32x32x16_bf16 (half the operand bytes per FLOP: the shape the guide's
 * 2 495 TFLOP/s figure is measured with). */
int mtn_measure_mfma_peak(int iters, float* scratch, void* stream, double* tflops);
int mtn_measure_mfma_peak_shapes(int iters, float* scratch, void* stream, double* tflops_16x16x32, double* tflops_32x32x16);
/* Achievable HBM rate of this box: a 16-byte-per-lane streaming copy src -> dst of `bytes` bytes (both buffers >= bytes, well
 * beyond the 256 MiB Infinity Cache; synchronises on its own events), (read + written bytes) / time in GB/s — the measured
 * denominator bench.py reports beside the 8 TB/s spec for the HBM-bound parameter-gradient + optimiser launch. */
int mtn_measure_hbm_peak(const void* src, void* dst, long bytes, void* stream, double* gbps);
/* ------------------------------------------------------------------------------------------
 * One decode step of the target stream as ONE persistent launch (round 5, version 112; W <= 16 and `max_m` since 113; csrc/decode.hip).  Replaces, for W <= 16 live
 * hypotheses, the per-token pass of `beam_search_decode` / `greedy_decode` (data_utils.py:197-208: `model.decode` + final LayerNorm)
 * in its cached form: the newest position of every hypothesis through N layers x (self-attention over the prefix cache, cross-attentions
 * over hoisted K|V, feed-forward), walking `stages` (a DEVICE array, built once per dialogue shape; stage 0 = MTN_DEC_EMBED, last = MTN_DEC_FINAL).
 * bf16 weights.  `grid` (<= 256: one per CU, all resident; clamped to the device's compute-unit count, and the call is refused when the three
 * classes do not fit) is the most workgroups the launch may use: W x h (<= 128) attention units + d / 16
 * writers of the residual stream + up to 128 for the wide projections — three classes, so that consecutive stages run on different
 * workgroups and each class prefetches its next stage while the others work.  Stages hand values over as 8-byte {data, tag} granules
 * (no grid barrier): xg / qg / og / hg are the granule buffers (zeroed ONCE by the caller); out_lp [W][d] bf16 = final LayerNorm
 * output (the generator's operand); sync: 4 unsigned, zeroed once: sync[0] = launch generation (advanced by the kernel), sync[2] = its check-in counter, sync[1] != 0 =
 * a poll timed out (50 ms, e.g. because another kernel held compute units and not every workgroup was resident) and the results are invalid:
 * every later launch returns at once until the caller zeroes sync[1] and sync[2] and ADVANCES sync[0] by one (stale granules of the failed
 * step must not match); mtn_amd/decode.py then re-runs the search on the launch-per-sublayer pass.
 * W x d <= 8192 and W x (2 max(d, d_ff) + 16) <= 66048 (16 rows up to d_ff = 2048, 8 at d_ff = 4096).
 * ------------------------------------------------------------------------------------------ */
#define MTN_DEC_EMBED 0     /* x = lut[token] * emb_scale + pe[pos] */
#define MTN_DEC_SELF_QKV 1  /* q | k | v = LayerNorm(x) W^T + b (N = 3d): q -> scratch, k | v -> cache row (hypothesis, pos) */
#define MTN_DEC_SELF_ATT 2  /* softmax(q K^T / sqrt(dk)) V over prefix positions 0..pos; position t of hypothesis j lives in cache slot anc[j][t] */
#define MTN_DEC_OUT 3       /* x += o W^T + b  (K = d) */
#define MTN_DEC_CROSS 4     /* q = LayerNorm(x) W_q^T + b_q per head, attention over the memory's hoisted K|V (kv, m keys, mask) */
#define MTN_DEC_FFN1 5      /* hid = relu(LayerNorm(x) W1^T + b1)  (N = d_ff) */
#define MTN_DEC_FFN2 6      /* x += hid W2^T + b2  (K = d_ff) */
#define MTN_DEC_FINAL 7     /* out_lp = LayerNorm(x) */
typedef struct {
    int kind, N, K;
    const void* w;              /* [N][K] bf16 (nn.Linear layout); MTN_DEC_CROSS: the q block of the packed q|k|v weight ([d][d]) */
    const float* bias;          /* [N] */
    const float* ln_a; const float* ln_b; float ln_eps;
    const void* kv;             /* MTN_DEC_CROSS: [W * m][2d] bf16, k | v of hypothesis j's memory rows j*m .. */
    int m;
    const unsigned char* mask; long mask_stride;     /* MTN_DEC_CROSS: key mask [W][mask_stride] uint8 (0 = masked: score -1e9); NULL = none */
    void* cache;                /* MTN_DEC_SELF_QKV / _ATT: this layer's prefix cache [W][L][2d] bf16 */
} mtn_decode_stage;
typedef struct {
    int W, d, h, L, n_stages, d_ff;
    void* xg; void* qg; void* og; void* hg;   /* granule buffers (8 bytes {data, tag} each), zeroed once: [W][d], [W][3d/2], [W][d/2], [W][d_ff/2] */
    void* out_lp;
    const long* tokens;         /* [W] newest token of every hypothesis */
    const float* lut; float emb_scale; const float* pe;     /* target embedding table [V][d], sqrt(d), positional encodings [>= L][d] */
    const int* pos;             /* device scalar: the position being decoded (0-based) */
    const int* anc;             /* [W][L] cache slot that holds position t of hypothesis j's prefix (anc[j][pos] = j) */
    unsigned* sync;
    void* dbg;                  /* NULL, or 4 x n_stages uint64: 100 MHz wall-clock stamps per stage of the first workgroup of the stage's class
                                   (entered / operands arrived / computed / stores issued) — tools/decode_timeline.py */
    int max_m;                  /* (113) the longest memory (`m`) of any MTN_DEC_CROSS stage, <= 1024: the stage list lives in device memory,
                                   so the host-side argument check needs it here */
} mtn_decode_args;
int mtn_decode_step(const mtn_decode_args* args /* host */, const mtn_decode_stage* stages_device, int grid, void* stream);
/* Test support (113): `n_wg` one-wave workgroups that hold `lds_bytes` of LDS each for `usec` microseconds and do nothing — compute units
 * taken away from whatever runs beside it.  tests/test_decode_gpu.py uses it to make mtn_decode_step's residency assumption fail. */
int mtn_debug_hold_cus(int n_wg, int lds_bytes, int usec, void* stream);
/* The library's development / test switches (MTN_GEMM_*, MTN_ATTN_*, MTN_LN_*, MTN_EMBED_DETERMINISTIC, ...) are read from the
 * environment once per call site and cached: a process that changes one after the library has used it calls this to make the
 * next launches re-read them.  Returns the new generation number. */
int mtn_reload_env(void);
/* Measurement support: a stream restricted to `n_cus` compute units (hipExtStreamCreateWithCUMask, bits dealt round-robin to the
 * 8 XCDs), for overlap experiments (tools/overlap_cu_mask_probe.py).  The caller destroys it with mtn_stream_destroy(). */
int mtn_stream_create_cu_masked(int n_cus, int low_priority, void** stream_out);
int mtn_stream_destroy(void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MTN_HIP_H */
