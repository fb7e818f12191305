// Text half of the support gallery (libclipfsar_gallery_text.so, C ABI in include/clipfsar_gallery_text.h): the EVAL_TEXT / COMBINE eval
// branches (few_shot.py:2835-2930) at any number of classes -- frame means, the zero-shot text logits scale * cos as one exact-fp32 MFMA
// GEMM with per-tile softmax partials in its epilogue, the class-wide softmax and the COMBINE fusion.
// A library of its own: libclipfsar_hip.so and libclipfsar_gallery.so keep their pinned export sets.
#include <stdint.h>

#include "fp32_tile_gemm.h"
#include "side_lib.h"
#include "../../include/clipfsar_gallery_text.h"

namespace {

constexpr int MAX_FRAMES = 1024;

// ---- mean over the frames: one workgroup per row.  Sum in t order, then / T (text_match_kernel's order, few_shot.py:2838)
__global__ __launch_bounds__(128) void frame_mean_kernel(const float* __restrict__ feats, float* __restrict__ out, int T, int E) {
    const float* f = feats + (size_t)blockIdx.x * T * E;
    float* o = out + (size_t)blockIdx.x * E;
    for (int e = threadIdx.x; e < E; e += 128) {
        float a = 0.f;
        for (int t = 0; t < T; ++t) a += f[(size_t)t * E + e];
        a /= (float)T;
        o[e] = a;
    }
}

// ---- zero-shot text logits of a gallery.  A workgroup (4 waves) owns 64 queries x 64 classes.
//   GEMM: [NQ, E] x [C, E]^T, fp32_tile_gemm (fp32_tile_gemm.h) with one row per query / class.
//   Epilogue: logits = scale * (dot / en / tn) into an LDS image of the tile (aliasing the staging buffers); then each wave stores
//   16 of its rows (lane = class column, coalesced) and reduces each row to the softmax partial (tile max, sum of expf(x - max)).
constexpr int ILD = TILE + 1 /* logit image */;

__global__ __launch_bounds__(256) void text_logits_kernel(const float* __restrict__ emb, const float* __restrict__ en,
                                                          const float* __restrict__ text, const float* __restrict__ tn,
                                                          const float* __restrict__ scale, float* __restrict__ logits,
                                                          float* __restrict__ partials, int NQ, int C, int E) {
    static_assert(TILE * ILD <= 2 * TILE * SLD, "the logit image must fit into the staging buffers");
    __shared__ __attribute__((aligned(16))) float smem[2 * TILE * SLD];
    __shared__ float sen[TILE], stn[TILE];
    float* sA = smem;                                  // [TILE][SLD]
    float* sB = smem + TILE * SLD;                     // [TILE][SLD]
    float* img = smem;                                 // [TILE][ILD], after the K loop
    const int c0 = blockIdx.x * TILE, q0 = blockIdx.y * TILE;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int a_rows = min(TILE, NQ - q0), b_rows = min(TILE, C - c0);           // valid rows of each operand
    if (tid < TILE) sen[tid] = tid < a_rows ? en[q0 + tid] : 1.f;
    else if (tid < 2 * TILE) stn[tid - TILE] = tid - TILE < b_rows ? tn[c0 + tid - TILE] : 1.f;

    f32x4 acc[2][2];
    fp32_tile_gemm(emb, (size_t)q0, a_rows, text, (size_t)c0, b_rows, E, sA, sB, acc);   // ends with a barrier: the logit image overwrites the staging buffers
    const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32, fr = lane & 15, fh = lane >> 4;
    const float sc_ = scale[0];
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
    const int ntiles = gridDim.x;
    const bool ok = lane < b_rows;
    for (int r = wave; r < a_rows; r += 4) {                              // wave-uniform loop: 16 rows per wave
        const float x = img[r * ILD + lane];
        if (ok) logits[(size_t)(q0 + r) * C + c0 + lane] = x;
        const float m = wave_max(ok ? x : -__builtin_inff());
        const float s = wave_sum(ok ? expf(x - m) : 0.f);
        if (lane == 0) {
            float* p = partials + ((size_t)(q0 + r) * ntiles + blockIdx.x) * 2;
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

// ---- class-wide softmax: one workgroup per query (probs may alias logits: every element is read and written by the same thread)
__global__ __launch_bounds__(256) void text_softmax_kernel(const float* logits, const float* __restrict__ partials, float* probs, int C,
                                                           int ntiles) {
    __shared__ float red[4];
    const size_t q = blockIdx.x;
    float M, S;
    merge_partials(partials + q * ntiles * 2, ntiles, red, M, S);
    const float* x = logits + q * C;
    float* o = probs + q * C;
    for (int c = threadIdx.x; c < C; c += 256) o[c] = expf(x[c] - M) / S;
}

// ---- COMBINE fusion (few_shot.py:2921-2928, combine_kernel's formula): one workgroup per query (out may alias logits)
__global__ __launch_bounds__(256) void text_combine_kernel(const float* logits, const float* __restrict__ partials,
                                                           const float* __restrict__ visual, float* out, int C, int ntiles, float coff) {
    __shared__ float red[4];
    const size_t q = blockIdx.x;
    float M, S;
    merge_partials(partials + q * ntiles * 2, ntiles, red, M, S);
    const float* v = visual + q * C;
    float mv = -__builtin_inff();
    row_pass4(v, C, [&](float x) { mv = fmaxf(mv, (8.0f + x) / 8.0f); });       // (8 - cum)/8 with cum = -v
    const float Mv = block_max(mv, red);
    float sv = 0.f;
    row_pass4(v, C, [&](float x) { sv += expf((8.0f + x) / 8.0f - Mv); });
    const float Sv = block_sum(sv, red);
    const float* x = logits + q * C;
    float* o = out + q * C;
    for (int c = threadIdx.x; c < C; c += 256) {
        const float p = expf(x[c] - M) / S;
        const float soft = expf((8.0f + v[c]) / 8.0f - Mv) / Sv;
        o[c] = powf(p, coff) * powf(soft, 1.0f - coff);
    }
}

long long workspace_floats(int NQ, int C) { return (long long)NQ * ((C + TILE - 1) / TILE) * 2; }

}  // namespace

extern "C" int cfgt_version(void) { return 100; /* 0.1.0 */ }
extern "C" int cfgt_abi_version(void) { return CFGT_ABI_VERSION; }
extern "C" const char* cfgt_last_error(void) { return g_err; }

extern "C" int cfgt_workspace_floats(int NQ, int C) {
    if (NQ <= 0 || C <= 0) return -1;
    const long long n = workspace_floats(NQ, C);
    return n <= 0x7fffffffLL ? (int)n : -1;
}

extern "C" int cfgt_frame_mean(const float* feats, float* out, int N, int T, int E, cfgt_stream_t stream) {
    SIDE_REQUIRE(feats && out, "cfgt_frame_mean: null pointer");
    SIDE_REQUIRE(N > 0 && T > 0 && T <= MAX_FRAMES && E > 0, "cfgt_frame_mean: bad shape (N=%d T=%d E=%d; 1 <= T <= %d)", N, T, E,
                 MAX_FRAMES);
    hipLaunchKernelGGL(frame_mean_kernel, dim3((unsigned)N), dim3(128), 0, static_cast<hipStream_t>(stream), feats, out, T, E);
    return check_launch("cfgt_frame_mean");
}

extern "C" int cfgt_text_logits(const float* emb, const float* en, const float* text, const float* tn, const float* scale, float* logits,
                                float* partials, int NQ, int C, int E, cfgt_stream_t stream) {
    SIDE_REQUIRE(emb && en && text && tn && scale && logits && partials, "cfgt_text_logits: null pointer");
    SIDE_REQUIRE(NQ > 0 && C > 0 && E >= 4 && E <= 8192 && E % 4 == 0,
                 "cfgt_text_logits: bad shape (NQ=%d C=%d E=%d; E %% 4 == 0, 4 <= E <= 8192)", NQ, C, E);
    SIDE_REQUIRE(((uintptr_t)emb & 15u) == 0 && ((uintptr_t)text & 15u) == 0, "cfgt_text_logits: emb and text must be 16-byte aligned");
    const long long gx = ((long long)C + TILE - 1) / TILE, gy = ((long long)NQ + TILE - 1) / TILE;
    SIDE_REQUIRE(gy <= 65535, "cfgt_text_logits: NQ=%d too large for one launch (at most %d)", NQ, 65535 * TILE);
    SIDE_REQUIRE(workspace_floats(NQ, C) <= 0x7fffffffLL, "cfgt_text_logits: partials workspace beyond 2^31 floats");
    hipLaunchKernelGGL(text_logits_kernel, dim3((unsigned)gx, (unsigned)gy), dim3(256), 0, static_cast<hipStream_t>(stream), emb, en, text,
                       tn, scale, logits, partials, NQ, C, E);
    return check_launch("cfgt_text_logits");
}

extern "C" int cfgt_text_softmax(const float* logits, const float* partials, float* probs, int NQ, int C, cfgt_stream_t stream) {
    SIDE_REQUIRE(logits && partials && probs, "cfgt_text_softmax: null pointer");
    SIDE_REQUIRE(NQ > 0 && C > 0, "cfgt_text_softmax: bad shape (NQ=%d C=%d)", NQ, C);
    SIDE_REQUIRE(workspace_floats(NQ, C) <= 0x7fffffffLL, "cfgt_text_softmax: partials workspace beyond 2^31 floats");
    const int ntiles = (C + TILE - 1) / TILE;
    hipLaunchKernelGGL(text_softmax_kernel, dim3((unsigned)NQ), dim3(256), 0, static_cast<hipStream_t>(stream), logits, partials, probs, C,
                       ntiles);
    return check_launch("cfgt_text_softmax");
}

extern "C" int cfgt_text_combine(const float* logits, const float* partials, const float* visual, float* out, int NQ, int C, float coff,
                                 cfgt_stream_t stream) {
    SIDE_REQUIRE(logits && partials && visual && out, "cfgt_text_combine: null pointer");
    SIDE_REQUIRE(NQ > 0 && C > 0, "cfgt_text_combine: bad shape (NQ=%d C=%d)", NQ, C);
    SIDE_REQUIRE(__builtin_isfinite(coff), "cfgt_text_combine: coff must be finite");
    SIDE_REQUIRE(workspace_floats(NQ, C) <= 0x7fffffffLL, "cfgt_text_combine: partials workspace beyond 2^31 floats");
    const int ntiles = (C + TILE - 1) / TILE;
    hipLaunchKernelGGL(text_combine_kernel, dim3((unsigned)NQ), dim3(256), 0, static_cast<hipStream_t>(stream), logits, partials, visual,
                       out, C, ntiles, coff);
    return check_launch("cfgt_text_combine");
}
