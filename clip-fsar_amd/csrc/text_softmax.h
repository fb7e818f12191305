// The softmax half of the text logits, shared by gallery_text.hip (one dense [NQ, C] rectangle) and live_text.hip (a ragged list of
// rectangles over a slot store): the epilogue of the 64 x 64 logit tile with its per-row softmax partial, the block reductions, the merge
// of a row's partials and the two row bodies -- the class-wide softmax and the COMBINE fusion.  One copy, so a row of a group and the
// same row of a dense call go through the same operations in the same order.
#pragma once
#include <stdint.h>

#include "fp32_tile_gemm.h"

constexpr int ILD = TILE + 1 /* logit image */;
static_assert(TILE * ILD <= 2 * TILE * SLD, "the logit image must fit into the staging buffers");

// ---- epilogue of a text-logit tile, after fp32_tile_gemm_rows (whose last barrier lets img alias the staging buffers):
//   logits = scale * (dot / en / tn) into the LDS image; then each wave stores 16 of the tile's rows (lane = class column, coalesced) and
//   reduces each row to the softmax partial (tile max, sum of expf(x - max)).
// sen / stn: the norms of the tile's queries / classes (1.f for padding).  out: the tile's first logit, ld floats between its rows.
// part: the (max, sum) pair of the tile's first row and this class tile, pstride floats between the pairs of consecutive rows.
__device__ __forceinline__ void text_tile_epilogue(const f32x4 (&acc)[2][2], float* img, const float* sen, const float* stn, float sc_,
                                                   int a_rows, int b_rows, float* __restrict__ out, size_t ld, float* __restrict__ part,
                                                   size_t pstride) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32, fr = lane & 15, fh = lane >> 4;
    // C/D map of the 16x16 MFMA: column = lane & 15, row = 4 (lane >> 4) + register
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int row = wm + 16 * mi + 4 * fh + g, col = wn + 16 * ni + fr;
                img[row * ILD + col] = sc_ * (acc[mi][ni][g] / sen[row] / stn[col]);   // tail.hip:266's order, no eps
            }
    __syncthreads();
    const bool ok = lane < b_rows;
    for (int r = wave; r < a_rows; r += 4) {                              // wave-uniform loop: 16 rows per wave
        const float x = img[r * ILD + lane];
        if (ok) out[(size_t)r * ld + lane] = x;
        const float m = wave_max(ok ? x : -__builtin_inff());
        const float s = wave_sum(ok ? expf(x - m) : 0.f);
        if (lane == 0) {
            float* p = part + (size_t)r * pstride;
            p[0] = m;
            p[1] = s;
        }
    }
}

// ---- block-wide reductions of a 256-thread workgroup (red: 4 floats of LDS; safe to call back to back)
__device__ __forceinline__ float block_max(float v, float* red) {
    v = wave_max(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}
__device__ __forceinline__ float block_sum(float v, float* red) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// the merged softmax statistics of one query row from its tile partials: M = max m_j, S = sum s_j expf(m_j - M)
__device__ __forceinline__ void merge_partials(const float* __restrict__ pq, int ntiles, float* red, float& M, float& S) {
    float m = -__builtin_inff();
    for (int j = threadIdx.x; j < ntiles; j += 256) m = fmaxf(m, pq[2 * j]);
    M = block_max(m, red);
    float s = 0.f;
    for (int j = threadIdx.x; j < ntiles; j += 256) s += pq[2 * j + 1] * expf(pq[2 * j] - M);
    S = block_sum(s, red);
}

// f(x) over the C floats of a row: a scalar head up to 16-byte alignment, float4 loads, a scalar tail
template <class F>
__device__ __forceinline__ void row_pass4(const float* __restrict__ row, int C, F f) {
    const int head = min(C, (int)(((16u - ((uint32_t)(uintptr_t)row & 15u)) & 15u) >> 2));
    for (int c = threadIdx.x; c < head; c += 256) f(row[c]);
    const int n4 = (C - head) >> 2;
    const float4* r4 = reinterpret_cast<const float4*>(row + head);
    for (int i = threadIdx.x; i < n4; i += 256) {
        const float4 v = r4[i];
        f(v.x);
        f(v.y);
        f(v.z);
        f(v.w);
    }
    for (int c = head + 4 * n4 + threadIdx.x; c < C; c += 256) f(row[c]);
}

// ---- class-wide softmax of one query row by its workgroup: x, o [C] (o may alias x: every element is read and written by the same
// thread), pq: the row's ntiles partials
__device__ __forceinline__ void text_softmax_row(const float* x, const float* __restrict__ pq, float* o, int C, int ntiles, float* red) {
    float M, S;
    merge_partials(pq, ntiles, red, M, S);
    for (int c = threadIdx.x; c < C; c += 256) o[c] = expf(x[c] - M) / S;
}

// ---- COMBINE fusion of one query row (few_shot.py:2921-2928, combine_kernel's formula); v [C]: the row's OTAM logits (o may alias x)
__device__ __forceinline__ void text_combine_row(const float* x, const float* __restrict__ pq, const float* __restrict__ v, float* o, int C,
                                                 int ntiles, float coff, float* red) {
    float M, S;
    merge_partials(pq, ntiles, red, M, S);
    float mv = -__builtin_inff();
    row_pass4(v, C, [&](float x) { mv = fmaxf(mv, (8.0f + x) / 8.0f); });       // (8 - cum)/8 with cum = -v
    const float Mv = block_max(mv, red);
    float sv = 0.f;
    row_pass4(v, C, [&](float x) { sv += expf((8.0f + x) / 8.0f - Mv); });
    const float Sv = block_sum(sv, red);
    for (int c = threadIdx.x; c < C; c += 256) {
        const float p = expf(x[c] - M) / S;
        const float soft = expf((8.0f + v[c]) / 8.0f - Mv) / Sv;
        o[c] = powf(p, coff) * powf(soft, 1.0f - coff);
    }
}
