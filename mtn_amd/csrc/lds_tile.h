// lds_tile.h — the two LDS idioms of the LDS-DMA kernels, each written once: how a bf16 operand tile gets from memory into an LDS
// image (lane-linear 16-byte chunks, swizzled on the SOURCE side), and how a fragment comes back out of a contraction-major image
// (the transposing LDS read).  A swizzle decides the layout of an image, so the issuer and the reader of one image name the SAME
// policy type below.
#pragma once
#include "common.h"

typedef __attribute__((address_space(3))) void lds_void_t;

// ---- swizzle policies: f(row) is XOR-ed into the index of the 16-byte slot inside the row ------------------------------------------
// row-major images (rows of contraction bytes, read 16 bytes per lane): rows of >= 256 B would put the 16 rows of a fragment read on
// one 16-byte slot -> (row & 15); 128-byte rows (two rows per sweep of the LDS banks) -> (row & 7): the 16 lanes one ds_read_b128
// cycle serves hit 16 different slots.  (row & 7) is also the swizzle of the fused kernels' [row][64] head images.
template <int MASK> struct SwzRow { static __device__ __forceinline__ int f(int row) { return row & MASK; } };
// [k][64 features] images (128-byte rows) of the dW kernel and the fused kernels' V image: the 4 rows of a transposing read hit
// different banks
struct SwzPair7 { static __device__ __forceinline__ int f(int krow) { return (krow >> 1) & 7; } };
// [k][BN columns] images of a B operand stored contraction-major (gemm_dma_kernel, BTR): the 8 rows one LDS cycle of the transposing
// read touches (k0..k0+3 of two lane groups, 8 rows apart) sit in 8 different 32-byte bank groups:
// 128-byte rows (BN = 64): even / odd rows own the two halves of the bank sweep, the slot PAIR moves with bits 1 and 3 of k;
// 64-byte rows (BN = 32): four consecutive rows own a quarter each, bit 3 of k selects the 32-byte half.
template <int BN> struct SwzKn {
    static __device__ __forceinline__ int f(int krow) {
        if constexpr (BN == 64) return ((((krow >> 1) & 1) | (((krow >> 3) & 1) << 1)) << 1);
        else return ((krow >> 3) & 1) << 1;
    }
};
// [k][128 features] images (256-byte rows = one full sweep of the LDS banks): s(k) = 2*(k & 3) + 8*((k >> 3) & 1): the 8 rows one
// transposing read touches per LDS cycle (k0..k0+3 of lane groups 0 and 1, 8 rows apart) sit in 8 different 32-byte bank groups
struct SwzK128 { static __device__ __forceinline__ int f(int krow) { return ((krow & 3) << 1) | (((krow >> 3) & 1) << 3); } };

// ---- the transposing fragment read -------------------------------------------------------------------------------------------------
// ds_read_b64_tr_b16, semantics measured on gfx950 (tools/tr_probe.hip): inside each 16-lane group, result lane i element j = element
// (i%4) of the 8-byte chunk supplied by lane 4j + i/4.  So lane t of a group supplies &T[k0 + t/4][n0 + 4*(t%4)] and lane i receives
// T[k0..k0+3][n0+i]: a 4(k) x 16(n) block delivered column-per-lane; two reads (k0 and k0+4) make one 16x16x32 fragment with the
// standard slot order (lane group g covers k = 8g..8g+7).
// Fragment of a [row][ROW_BYTES] bf16 image swizzled with SWZ: columns n_off + (lane & 15) (n_off a multiple of 16), rows
// row0 + 8*lg .. +7 — 32 contraction rows from row0 across the four lane groups.
template <int ROW_BYTES, typename SWZ>
__device__ __forceinline__ uint4 tr_frag(const unsigned char* img, int row0, int n_off, int l15, int lg) {
    uint4 f;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int krow = row0 + 8 * lg + 4 * r + (l15 >> 2);
        const int col = n_off + 4 * (l15 & 3);                       // element column
        const int slot = (col >> 3) ^ SWZ::f(krow);                  // swizzled 16-byte slot
        const unsigned addr = (unsigned)(size_t)(img + krow * ROW_BYTES + slot * 16 + (col & 7) * 2);
        unsigned long long v;
        asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(v) : "v"(addr));
        if (r == 0) { f.x = (unsigned)v; f.y = (unsigned)(v >> 32); }
        else { f.z = (unsigned)v; f.w = (unsigned)(v >> 32); }
    }
    return f;
}

// ---- LDS-DMA tile issue ------------------------------------------------------------------------------------------------------------
// One operand tile of ROWS rows x ROW_BYTES bytes by NW waves: ROWS * ROW_BYTES / (1024 * NW) instructions per wave, each 1 KiB
// (1024 / ROW_BYTES rows).  LDS-DMA writes lane-linear, so the swizzle is applied to the per-lane SOURCE chunk (the reader applies the
// same involution); a chunk outside the operand is pushed past the buffer descriptor's bound and arrives as zeros.
//
// Row-major operand (rows of contraction elements of type T), tile rows row0.., contraction from k0.
template <typename T, int ROW_BYTES, int ROWS, int NW, typename SWZ = SwzRow<(ROW_BYTES / 16 < 16 ? ROW_BYTES / 16 : 16) - 1>>
__device__ __forceinline__ void dma_issue_rows(__amdgpu_buffer_rsrc_t rsrc, unsigned char* lds_tile, int ld_bytes, int R, int K,
                                               int row0, int k0, int wave, int lane) {
    constexpr int EPV = 16 / (int)sizeof(T);                         // elements per 16-byte chunk
    constexpr int CPR = ROW_BYTES / 16;                              // 16-byte chunks per row
    constexpr int RPI = 1024 / ROW_BYTES;                            // rows per wave-instruction
#pragma unroll
    for (int j = 0; j < ROWS * ROW_BYTES / (1024 * NW); ++j) {
        const int inst = j * NW + wave;
        const int row = inst * RPI + lane / CPR;                     // tile row written by this lane
        const int c = (lane % CPR) ^ SWZ::f(row);                    // source chunk that lands in slot (lane % CPR)
        const int gk = k0 + c * EPV;
        int grow = row0 + row;
        grow = grow < R ? grow : R - 1;                              // rows past the end only feed outputs that are never stored
        unsigned voff = (gk < K) ? (unsigned)grow * (unsigned)ld_bytes + (unsigned)gk * (unsigned)sizeof(T) : 0x80000000u;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (lds_void_t*)(lds_tile + inst * 1024), 16, voff, 0, 0, 0);
    }
}
// Contraction-major bf16 operand ([K][N] row-major): the [ROWS k][ROW_BYTES / 2 columns] tile from (k0, col0) lands as it lies.
template <int ROW_BYTES, int ROWS, int NW, typename SWZ>
__device__ __forceinline__ void dma_issue_kn(__amdgpu_buffer_rsrc_t rsrc, unsigned char* lds_tile, int ld_bytes, int N, int K,
                                             int col0, int k0, int wave, int lane) {
    constexpr int CPR = ROW_BYTES / 16;                              // 16-byte chunks per row
    constexpr int RPI = 1024 / ROW_BYTES;                            // k rows per wave-instruction
#pragma unroll
    for (int j = 0; j < ROWS * ROW_BYTES / (1024 * NW); ++j) {
        const int inst = j * NW + wave;
        const int krow = inst * RPI + lane / CPR;                    // row of the tile written by this lane
        const int c = (lane % CPR) ^ SWZ::f(krow);                   // source chunk that lands in slot (lane % CPR)
        const int gk = k0 + krow, gn = col0 + c * 8;
        unsigned voff = (gk < K && gn < N) ? (unsigned)gk * (unsigned)ld_bytes + (unsigned)gn * 2u : 0x80000000u;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (lds_void_t*)(lds_tile + inst * 1024), 16, voff, 0, 0, 0);
    }
}
