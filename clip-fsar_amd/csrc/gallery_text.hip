// Text half of the support gallery (libclipfsar_gallery_text.so, C ABI in include/clipfsar_gallery_text.h): the EVAL_TEXT / COMBINE eval
// branches (few_shot.py:2835-2930) at any number of classes -- frame means, the zero-shot text logits scale * cos as one exact-fp32 MFMA
// GEMM with per-tile softmax partials in its epilogue, the class-wide softmax and the COMBINE fusion.
// A library of its own: libclipfsar_hip.so and libclipfsar_gallery.so keep their pinned export sets.  The GEMM tile loop is a copy of
// otam_gallery_kernel's (gallery.hip), kept here so that the gallery library's code stays exactly as it is.
#include <stdarg.h>
#include <stdint.h>

#include "common.h"
#include "../../include/clipfsar_gallery_text.h"

namespace {

thread_local char g_err[512] = {0};

int fail(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return 1;
}

int check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail("%s: %s", what, hipGetErrorString(e));
    return 0;
}

#define CFGT_REQUIRE(cond, ...)               \
    do {                                      \
        if (!(cond)) return fail(__VA_ARGS__); \
    } while (0)

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
//   GEMM: [NQ, E] x [C, E]^T with v_mfma_f32_16x16x4_f32 (an exact fp32 fmaf chain per k step); both operands staged through LDS in
//   BK-float chunks, the next chunk's global loads in flight while the current one is multiplied; wave w owns the 32 x 32 quarter
//   (w >> 1, w & 1) as 2 x 2 MFMA tiles (otam_gallery_kernel's tile loop, with one row per query / class instead of T).
//   Epilogue: logits = scale * (dot / en / tn) into an LDS image of the tile (aliasing the staging buffers); then each wave stores
//   16 of its rows (lane = class column, coalesced) and reduces each row to the softmax partial (tile max, sum of expf(x - max)).
constexpr int TILE = 64, BK = 32, SLD = BK + 4 /* staging row stride: 16-B aligned rows */, ILD = TILE + 1 /* logit image */;

__device__ __forceinline__ float4 load_row4(const float* __restrict__ X, size_t row, int col, int E, bool ok) {
    return ok ? *reinterpret_cast<const float4*>(X + row * E + col) : make_float4(0.f, 0.f, 0.f, 0.f);
}

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

    // staging: 2 float4 of A and 2 of B per thread and chunk; rows / columns outside the operands are zero (they add +0 to the sums)
    const int sr0 = tid >> 3, sr1 = (tid + 256) >> 3, sc = (tid & 7) * 4;          // staged rows of the two float4s, their column
    float4 ra0, ra1, rb0, rb1;
#define CFGT_LOAD_CHUNK(k0)                                                                                  \
    do {                                                                                                     \
        const int col_ = (k0) + sc;                                                                          \
        ra0 = load_row4(emb, (size_t)q0 + sr0, col_, E, sr0 < a_rows && col_ < E);                           \
        ra1 = load_row4(emb, (size_t)q0 + sr1, col_, E, sr1 < a_rows && col_ < E);                           \
        rb0 = load_row4(text, (size_t)c0 + sr0, col_, E, sr0 < b_rows && col_ < E);                          \
        rb1 = load_row4(text, (size_t)c0 + sr1, col_, E, sr1 < b_rows && col_ < E);                          \
    } while (0)
    f32x4 acc[2][2];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32, fr = lane & 15, fh = lane >> 4;
    CFGT_LOAD_CHUNK(0);
    for (int k0 = 0; k0 < E; k0 += BK) {
        __syncthreads();                                                  // the previous chunk's fragment reads are done
        *reinterpret_cast<float4*>(sA + sr0 * SLD + sc) = ra0;
        *reinterpret_cast<float4*>(sA + sr1 * SLD + sc) = ra1;
        *reinterpret_cast<float4*>(sB + sr0 * SLD + sc) = rb0;
        *reinterpret_cast<float4*>(sB + sr1 * SLD + sc) = rb1;
        __syncthreads();
        if (k0 + BK < E) CFGT_LOAD_CHUNK(k0 + BK);                                   // next chunk in flight during this one's MFMAs
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
#pragma unroll
        for (int s = 0; s < 8; ++s)
#pragma unroll
            for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                for (int ni = 0; ni < 2; ++ni)
                    acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[mi][s >> 2][s & 3], b[ni][s >> 2][s & 3], acc[mi][ni], 0, 0, 0);
    }
#undef CFGT_LOAD_CHUNK
    __syncthreads();                                                      // the logit image overwrites the staging buffers
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
    CFGT_REQUIRE(feats && out, "cfgt_frame_mean: null pointer");
    CFGT_REQUIRE(N > 0 && T > 0 && T <= MAX_FRAMES && E > 0, "cfgt_frame_mean: bad shape (N=%d T=%d E=%d; 1 <= T <= %d)", N, T, E,
                 MAX_FRAMES);
    hipLaunchKernelGGL(frame_mean_kernel, dim3((unsigned)N), dim3(128), 0, static_cast<hipStream_t>(stream), feats, out, T, E);
    return check_launch("cfgt_frame_mean");
}

extern "C" int cfgt_text_logits(const float* emb, const float* en, const float* text, const float* tn, const float* scale, float* logits,
                                float* partials, int NQ, int C, int E, cfgt_stream_t stream) {
    CFGT_REQUIRE(emb && en && text && tn && scale && logits && partials, "cfgt_text_logits: null pointer");
    CFGT_REQUIRE(NQ > 0 && C > 0 && E >= 4 && E <= 8192 && E % 4 == 0,
                 "cfgt_text_logits: bad shape (NQ=%d C=%d E=%d; E %% 4 == 0, 4 <= E <= 8192)", NQ, C, E);
    CFGT_REQUIRE(((uintptr_t)emb & 15u) == 0 && ((uintptr_t)text & 15u) == 0, "cfgt_text_logits: emb and text must be 16-byte aligned");
    const long long gx = ((long long)C + TILE - 1) / TILE, gy = ((long long)NQ + TILE - 1) / TILE;
    CFGT_REQUIRE(gy <= 65535, "cfgt_text_logits: NQ=%d too large for one launch (at most %d)", NQ, 65535 * TILE);
    CFGT_REQUIRE(workspace_floats(NQ, C) <= 0x7fffffffLL, "cfgt_text_logits: partials workspace beyond 2^31 floats");
    hipLaunchKernelGGL(text_logits_kernel, dim3((unsigned)gx, (unsigned)gy), dim3(256), 0, static_cast<hipStream_t>(stream), emb, en, text,
                       tn, scale, logits, partials, NQ, C, E);
    return check_launch("cfgt_text_logits");
}

extern "C" int cfgt_text_softmax(const float* logits, const float* partials, float* probs, int NQ, int C, cfgt_stream_t stream) {
    CFGT_REQUIRE(logits && partials && probs, "cfgt_text_softmax: null pointer");
    CFGT_REQUIRE(NQ > 0 && C > 0, "cfgt_text_softmax: bad shape (NQ=%d C=%d)", NQ, C);
    CFGT_REQUIRE(workspace_floats(NQ, C) <= 0x7fffffffLL, "cfgt_text_softmax: partials workspace beyond 2^31 floats");
    const int ntiles = (C + TILE - 1) / TILE;
    hipLaunchKernelGGL(text_softmax_kernel, dim3((unsigned)NQ), dim3(256), 0, static_cast<hipStream_t>(stream), logits, partials, probs, C,
                       ntiles);
    return check_launch("cfgt_text_softmax");
}

extern "C" int cfgt_text_combine(const float* logits, const float* partials, const float* visual, float* out, int NQ, int C, float coff,
                                 cfgt_stream_t stream) {
    CFGT_REQUIRE(logits && partials && visual && out, "cfgt_text_combine: null pointer");
    CFGT_REQUIRE(NQ > 0 && C > 0, "cfgt_text_combine: bad shape (NQ=%d C=%d)", NQ, C);
    CFGT_REQUIRE(__builtin_isfinite(coff), "cfgt_text_combine: coff must be finite");
    CFGT_REQUIRE(workspace_floats(NQ, C) <= 0x7fffffffLL, "cfgt_text_combine: partials workspace beyond 2^31 floats");
    const int ntiles = (C + TILE - 1) / TILE;
    hipLaunchKernelGGL(text_combine_kernel, dim3((unsigned)NQ), dim3(256), 0, static_cast<hipStream_t>(stream), logits, partials, visual,
                       out, C, ntiles, coff);
    return check_launch("cfgt_text_combine");
}
