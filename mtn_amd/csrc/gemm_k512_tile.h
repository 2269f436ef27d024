// gemm_k512_tile.h — one 128 x 256 output tile of y = x W^T + b with K = 512 (the wide one-shot construction of gemm_k512.hip), as a
// device function: the body of gemm_k512w_kernel, and of the K|V rider workgroups that travel in the fused forward launches
// (fused.hip) — one arithmetic order wherever a tile is computed, so a tile's bits do not depend on which launch carried it.
#pragma once
#include "fused_common.h"

static constexpr int GK_THREADS = 512;
static constexpr int GK_K = 512;
static constexpr int GK_LDS = 128 * FH_ROWB;              // 128 KiB: the x image; reused as the output staging area
static constexpr int GK_CPITCH = 272;                     // bytes per staged output row (256 + 16)
static constexpr int GW_CPITCH = 528;                     // wide tile: bytes per staged output row (512 + 16)

struct GkProblem { const bf16_t* A; const bf16_t* B; const float* bias; bf16_t* out; int lda, ldb, ldc, M, N, tiles_m; };

// tile t of problem P (row tiles vary fastest: see gemm_k512_kernel); smem: GK_LDS bytes, 512 threads
__device__ __forceinline__ void gk_wide_tile(const GkProblem& P, const int t, unsigned char* smem) {
    const int tid = threadIdx.x, lane = tid & 63, l15 = lane & 15, lg = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tn = t / P.tiles_m, tm = t - tn * P.tiles_m;
    const int row0 = tm * 128, col0 = tn * 256;
    const int R = (P.M - row0) < 128 ? (P.M - row0) : 128;
    {
        const unsigned ldab = (unsigned)P.lda * 2u;
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)(P.A + (size_t)row0 * P.lda), 0, (R - 1) * ldab + FH_ROWB, 0x00020000);
        for (int r = wave; r < 128; r += 8) {
            const unsigned vo = r < R ? (unsigned)r * ldab + (unsigned)((lane ^ (r & 15)) << 4) : 0x80000000u;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_void_t*)(smem + r * FH_ROWB), 16, vo, 0, 0, 0);
        }
    }
    float4 bq[2];
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) {
        const int colq = col0 + 128 * cb + 16 * wave + 4 * lg;
        bq[cb] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (P.bias && colq < P.N) bq[cb] = *(const float4*)(P.bias + colq);
    }
    __builtin_amdgcn_sched_barrier(0);
    // W fragments in CONTRACTION order (step s of both column blocks, then step s + 1, ...): the MFMAs of step s start as soon as its
    // two fragments have landed, while the later ones are still being accepted — a wave's 32 loads take ~6 us to issue, and the kernel
    // used to wait for all of them before its first MFMA.
    uint4 wf[2][16];                                             // column block cb: columns col0 + 128 cb + 16 wave .. + 15
    {
        const bf16_t* wrow[2];
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) {
            int n = col0 + 128 * cb + 16 * wave + (lane >> 2);
            n = n < P.N ? n : P.N - 1;
            wrow[cb] = P.B + (size_t)n * P.ldb + (lane & 3) * 8;
        }
#pragma unroll
        for (int s = 0; s < 16; ++s) { wf[0][s] = *(const uint4*)(wrow[0] + s * 32); wf[1][s] = *(const uint4*)(wrow[1] + s * 32); }
    }
    __builtin_amdgcn_sched_barrier(0);
    // the x image (and the bias) has landed once at most the 32 W loads behind it fly: s_waitcnt vmcnt(32) lgkmcnt(15) expcnt(7) as a
    // BUILTIN, so that the compiler's own counter knows that no LDS-DMA is outstanding any more (behind an inline-asm wait it would put
    // vmcnt(0) in front of the first LDS read it sees)
    __builtin_amdgcn_s_waitcnt(0x8F70);
    __builtin_amdgcn_s_barrier();
    f32x4_t acc[2][8];
#pragma unroll
    for (int cb = 0; cb < 2; ++cb)
#pragma unroll
        for (int mt = 0; mt < 8; ++mt) acc[cb][mt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    const int src = (4 * l15 + lg) * 4;
#pragma unroll
    for (int s = 0; s < 16; ++s) {
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) {                         // coalesced load order -> MFMA operand order
            wf[cb][s].x = (unsigned)__builtin_amdgcn_ds_bpermute(src, (int)wf[cb][s].x);
            wf[cb][s].y = (unsigned)__builtin_amdgcn_ds_bpermute(src, (int)wf[cb][s].y);
            wf[cb][s].z = (unsigned)__builtin_amdgcn_ds_bpermute(src, (int)wf[cb][s].z);
            wf[cb][s].w = (unsigned)__builtin_amdgcn_ds_bpermute(src, (int)wf[cb][s].w);
        }
#pragma unroll
        for (int mt = 0; mt < 8; ++mt) {
            const uint4 xf = fh_xfrag(smem, mt * 16 + l15, s * 4 + lg);
            mma16<bf16_t>(acc[0][mt], wf[0][s], xf);
            mma16<bf16_t>(acc[1][mt], wf[1][s], xf);
        }
    }
    __syncthreads();                                             // the x image is dead: it becomes the output staging area
#pragma unroll
    for (int cb = 0; cb < 2; ++cb)
#pragma unroll
        for (int mt = 0; mt < 8; ++mt) {
            const int r = mt * 16 + l15;
            *(uint2*)(smem + r * GW_CPITCH + (128 * cb + 16 * wave + 4 * lg) * 2) =
                make_uint2(fh_pack2(acc[cb][mt][0] + bq[cb].x, acc[cb][mt][1] + bq[cb].y), fh_pack2(acc[cb][mt][2] + bq[cb].z, acc[cb][mt][3] + bq[cb].w));
        }
    __syncthreads();
    // whole 512-byte row segments: 32 lanes per row, 16 rows per pass
#pragma unroll
    for (int ps = 0; ps < 8; ++ps) {
        const int r = ps * 16 + (tid >> 5), c = tid & 31;
        const int col = col0 + c * 8;
        if (r < R && col < P.N)
            *(uint4*)(P.out + (size_t)(row0 + r) * P.ldc + col) = *(const uint4*)(smem + r * GW_CPITCH + c * 16);
    }
}

// K|V rider units of one fused forward launch (fused.hip): rider workgroup r computes tile tile0[j] + r - start[j] of problem p[j],
// j = the problem with start[j] <= r < start[j + 1].  By value in the launch's kernel arguments: a captured graph replays it as it is.
#define GK_RIDER_PROBLEMS 4
struct GkRider {
    int units;                                   // rider workgroups of the launch (0: none)
    int start[GK_RIDER_PROBLEMS + 1];
    int tile0[GK_RIDER_PROBLEMS];
    GkProblem p[GK_RIDER_PROBLEMS];
};
__device__ __forceinline__ void gk_rider_unit(const GkRider& K, const int r, unsigned char* smem) {
    int j = 0;
    while (j + 1 < GK_RIDER_PROBLEMS && r >= K.start[j + 1]) ++j;
    gk_wide_tile(K.p[j], K.tile0[j] + r - K.start[j], smem);
}

// host side (gemm_k512.hip: pending K|V work)
void gk_rider_take(int slots, GkRider* K);                                       // up to `slots` pending tiles, from the head of the queue
int gk_pending_flush_reads(int n, const void* const* outs, void* stream);        // stand-alone launches of what writes outs[0 .. n), and of all before it
