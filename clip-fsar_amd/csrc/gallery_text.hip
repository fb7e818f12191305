// Text half of the support gallery (libclipfsar_gallery_text.so, C ABI in include/clipfsar_gallery_text.h): the EVAL_TEXT / COMBINE eval
// branches (few_shot.py:2835-2930) at any number of classes -- frame means, the zero-shot text logits scale * cos as one exact-fp32 MFMA
// GEMM with per-tile softmax partials in its epilogue, the class-wide softmax and the COMBINE fusion.
// A library of its own: libclipfsar_hip.so and libclipfsar_gallery.so keep their pinned export sets.
#include <stdint.h>

#include "fp32_tile_gemm.h"
#include "side_lib.h"
#include "text_softmax.h"
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
//   Epilogue (text_tile_epilogue, text_softmax.h): logits = scale * (dot / en / tn) into an LDS image of the tile (aliasing the staging buffers); then each wave stores
//   16 of its rows (lane = class column, coalesced) and reduces each row to the softmax partial (tile max, sum of expf(x - max)).
__global__ __launch_bounds__(256) void text_logits_kernel(const float* __restrict__ emb, const float* __restrict__ en,
                                                          const float* __restrict__ text, const float* __restrict__ tn,
                                                          const float* __restrict__ scale, float* __restrict__ logits,
                                                          float* __restrict__ partials, int NQ, int C, int E) {
    __shared__ __attribute__((aligned(16))) float smem[2 * TILE * SLD];
    __shared__ float sen[TILE], stn[TILE];
    float* sA = smem;                                  // [TILE][SLD]
    float* sB = smem + TILE * SLD;                     // [TILE][SLD]
    float* img = smem;                                 // [TILE][ILD], after the K loop
    const int c0 = blockIdx.x * TILE, q0 = blockIdx.y * TILE;
    const int tid = threadIdx.x;
    const int a_rows = min(TILE, NQ - q0), b_rows = min(TILE, C - c0);           // valid rows of each operand
    if (tid < TILE) sen[tid] = tid < a_rows ? en[q0 + tid] : 1.f;
    else if (tid < 2 * TILE) stn[tid - TILE] = tid - TILE < b_rows ? tn[c0 + tid - TILE] : 1.f;

    f32x4 acc[2][2];
    fp32_tile_gemm(emb, (size_t)q0, a_rows, text, (size_t)c0, b_rows, E, sA, sB, acc);   // ends with a barrier: the logit image overwrites the staging buffers
    text_tile_epilogue(acc, img, sen, stn, scale[0], a_rows, b_rows, logits + (size_t)q0 * C + c0, (size_t)C,
                       partials + ((size_t)q0 * gridDim.x + blockIdx.x) * 2, (size_t)gridDim.x * 2);
}

// ---- class-wide softmax: one workgroup per query (probs may alias logits: every element is read and written by the same thread)
__global__ __launch_bounds__(256) void text_softmax_kernel(const float* logits, const float* __restrict__ partials, float* probs, int C,
                                                           int ntiles) {
    __shared__ float red[4];
    const size_t q = blockIdx.x;
    text_softmax_row(logits + q * C, partials + q * ntiles * 2, probs + q * C, C, ntiles, red);
}

// ---- COMBINE fusion (few_shot.py:2921-2928, combine_kernel's formula): one workgroup per query (out may alias logits)
__global__ __launch_bounds__(256) void text_combine_kernel(const float* logits, const float* __restrict__ partials,
                                                           const float* __restrict__ visual, float* out, int C, int ntiles, float coff) {
    __shared__ float red[4];
    const size_t q = blockIdx.x;
    text_combine_row(logits + q * C, partials + q * ntiles * 2, visual + q * C, out + q * C, C, ntiles, coff, red);
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
