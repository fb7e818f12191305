// The exact-fp32 MFMA tile GEMM of the gallery libraries (otam_tile in otam_tile.h, the body of otam_gallery_kernel in gallery.hip, of
// otam_indexed_kernel in live.hip and of otam_grouped_kernel in groups.hip; text_logits_kernel in gallery_text.hip, text_logits_grouped_kernel in live_text.hip):
// a 256-thread workgroup (4 waves) computes a TILE x TILE block of A[., E] x B[., E]^T with v_mfma_f32_16x16x4_f32 (an exact fp32 fmaf
// chain per k step).  Both operands are staged through LDS in BK-float chunks, the next chunk's global loads in flight while the current
// one is multiplied.  Wave w owns the 32 x 32 quarter (w >> 1, w & 1) as 2 x 2 MFMA tiles.  Inside a chunk, MFMA step s of lane half h
// takes k = 8h + s: every lane reads its k values as two ds_read_b128 per tile (A and B use the same k map, so the products are those of
// the plain GEMM, summed in another order).
// Every chunk is summed from zero and then added to the running sum: an element is a chain of at most BK products per chunk plus E / BK
// chunk adds, not one chain of E.  The single chain missed 1e-6 on 1 - cos where |cos| is near 1 (a sum of like-signed products): worst
// error at E = 512 on an MI355X 1.54e-6 before, 0.36e-6 now (tests/test_gpu_otam.py, families near and anti).
#pragma once
#include "common.h"

constexpr int TILE = 64, BK = 32, SLD = BK + 4 /* staging row stride: 16-B aligned rows */;

__device__ __forceinline__ float4 load_row4(const float* __restrict__ X, size_t row, int col, int E, bool ok) {
    return ok ? *reinterpret_cast<const float4*>(X + row * E + col) : make_float4(0.f, 0.f, 0.f, 0.f);
}

// The whole K loop of one workgroup's tile.  A / B: row-major [., E] operands (E % 4 == 0, 16-byte aligned rows); the tile's rows are
// arow0 .. arow0 + a_rows - 1 of A (a_rows <= TILE) and, for tile row r of B, the row a B-ROW MAP names: brow(r), asked once per
// staged row before the K loop, answers with a handle whose row() is the row of B and whose ok() says whether it exists (zeros are
// staged when not).  What a handle computes late stays cheap in registers: the identity's (TileRows below) keeps only r.
// sA, sB: [TILE][SLD] staging buffers.
// acc[mi][ni]: this wave's 2 x 2 MFMA tiles (C/D map of the 16x16 MFMA: column = lane & 15, row = 4 (lane >> 4) + register), zeroed
// here.  Ends with a barrier: on return every wave's fragment reads are done and the caller may overwrite the staging buffers.
template <class BRowMap>
__device__ __forceinline__ void fp32_tile_gemm_rows(const float* __restrict__ A, size_t arow0, int a_rows, const float* __restrict__ B,
                                                    BRowMap brow, int E, float* sA, float* sB, f32x4 (&acc)[2][2]) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // staging: 2 float4 of A and 2 of B per thread and chunk; rows / columns outside the operands are zero (they add +0 to the sums)
    const int sr0 = tid >> 3, sr1 = (tid + 256) >> 3, sc = (tid & 7) * 4;          // staged rows of the two float4s, their column
    const auto br0 = brow(sr0), br1 = brow(sr1);                                   // the two staged B rows of this thread
    float4 ra0, ra1, rb0, rb1;
    auto load_chunk = [&](int k0) {
        const int col = k0 + sc;
        ra0 = load_row4(A, arow0 + sr0, col, E, sr0 < a_rows && col < E);
        ra1 = load_row4(A, arow0 + sr1, col, E, sr1 < a_rows && col < E);
        rb0 = load_row4(B, br0.row(), col, E, br0.ok() && col < E);
        rb1 = load_row4(B, br1.row(), col, E, br1.ok() && col < E);
    };
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32, fr = lane & 15, fh = lane >> 4;
    load_chunk(0);
    for (int k0 = 0; k0 < E; k0 += BK) {
        __syncthreads();                                                  // the previous chunk's fragment reads are done
        *reinterpret_cast<float4*>(sA + sr0 * SLD + sc) = ra0;
        *reinterpret_cast<float4*>(sA + sr1 * SLD + sc) = ra1;
        *reinterpret_cast<float4*>(sB + sr0 * SLD + sc) = rb0;
        *reinterpret_cast<float4*>(sB + sr1 * SLD + sc) = rb1;
        __syncthreads();
        if (k0 + BK < E) load_chunk(k0 + BK);                             // next chunk in flight during this one's MFMAs
        f32x4 a[2][2], b[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const float* pa = sA + (wm + 16 * i + fr) * SLD + fh * 8;
            const float* pb = sB + (wn + 16 * i + fr) * SLD + fh * 8;
            a[i][0] = *reinterpret_cast<const f32x4*>(pa);
            a[i][1] = *reinterpret_cast<const f32x4*>(pa + 4);
            b[i][0] = *reinterpret_cast<const f32x4*>(pb);
            b[i][1] = *reinterpret_cast<const f32x4*>(pb + 4);
        }
        f32x4 part[2][2];                                                 // this chunk's sums: a chain of BK products from zero
#pragma unroll
        for (int s = 0; s < 8; ++s)
#pragma unroll
            for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                for (int ni = 0; ni < 2; ++ni)
                    part[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[mi][s >> 2][s & 3], b[ni][s >> 2][s & 3],
                                                                        s ? part[mi][ni] : f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int ni = 0; ni < 2; ++ni) acc[mi][ni] += part[mi][ni];
    }
    __syncthreads();
}

// The identity map: the tile's B rows are brow0 .. brow0 + b_rows - 1 (b_rows <= TILE), as A's are.
struct TileRows {
    size_t row0;
    int rows;
    struct Row {
        size_t row0;
        int r, rows;
        __device__ __forceinline__ size_t row() const { return row0 + r; }
        __device__ __forceinline__ bool ok() const { return r < rows; }
    };
    __device__ __forceinline__ Row operator()(int r) const { return Row{row0, r, rows}; }
};
// A row looked up before the K loop (a gather through an index list): negative = no such row.
struct LookedUpRow {
    long long at;
    __device__ __forceinline__ size_t row() const { return (size_t)at; }
    __device__ __forceinline__ bool ok() const { return at >= 0; }
};

__device__ __forceinline__ void fp32_tile_gemm(const float* __restrict__ A, size_t arow0, int a_rows, const float* __restrict__ B,
                                               size_t brow0, int b_rows, int E, float* sA, float* sB, f32x4 (&acc)[2][2]) {
    fp32_tile_gemm_rows(A, arow0, a_rows, B, TileRows{brow0, b_rows}, E, sA, sB, acc);
}
