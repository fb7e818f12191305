// Support gallery (libclipfsar_gallery.so, C ABI in include/clipfsar_gallery.h): support sequences of any number of videos,
// per-class means over contiguous runs of videos, row norms, top-k, and the hot kernel -- cos_sim + OTAM of every (query, class)
// pair of a gallery (few_shot.py:1115-1124, 2657-2687, 2970-2990) as one exact-fp32 MFMA GEMM with the soft-min DPs in its epilogue.
// A library of its own: libclipfsar_hip.so keeps exactly the entry points of include/clipfsar_hip.h.
#include <stdarg.h>

#include "common.h"
#include "../../include/clipfsar_gallery.h"

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

#define CFSG_REQUIRE(cond, ...)               \
    do {                                      \
        if (!(cond)) return fail(__VA_ARGS__); \
    } while (0)

// ---- support sequences: one workgroup per output row (few_shot.py:2946, :2955)
__global__ __launch_bounds__(128) void support_sequences_kernel(const float* __restrict__ feats, const float* __restrict__ text,
                                                                const int32_t* __restrict__ cls_of_video, float* __restrict__ X,
                                                                int T, int E, int n_cls) {
    const int row = blockIdx.x, tid = threadIdx.x;
    const int v = row / (T + 1), t = row - v * (T + 1);
    const float* src;
    if (t < T) {
        src = feats + ((size_t)v * T + t) * E;
    } else {
        const int cls = cls_of_video[v];
        src = (cls >= 0 && cls < n_cls) ? text + (size_t)cls * E : nullptr;     // out of range: NaN row (validated on the host)
    }
    float* xr = X + (size_t)row * E;
    for (int e = tid; e < E; e += 128) xr[e] = src ? src[e] : __builtin_nanf("");
}

// ---- per-class means over contiguous runs of videos: one workgroup per (class, kept row).  Sum in video order, then * (1 / count),
// the operation order of cfsar_prototypes and of cfsar_build_sequences' merged rows.
__global__ __launch_bounds__(128) void segment_mean_kernel(const float* __restrict__ X, const int32_t* __restrict__ offsets,
                                                           float* __restrict__ out, int Nv, int L, int E, int rows_kept) {
    const int c = blockIdx.x / rows_kept, r = blockIdx.x - c * rows_kept, tid = threadIdx.x;
    const int lo = offsets[c], hi = offsets[c + 1];
    const bool ok = lo >= 0 && lo < hi && hi <= Nv;
    const float inv = ok ? 1.0f / (float)(hi - lo) : __builtin_nanf("");
    float* o = out + ((size_t)c * rows_kept + r) * E;
    for (int e = tid; e < E; e += 128) {
        float a = 0.f;
        if (ok)
            for (int v = lo; v < hi; ++v) a += X[((size_t)v * L + r) * E + e];
        o[e] = ok ? a * inv : __builtin_nanf("");
    }
}

// ---- row L2 norms: one wave per row (the same lane-strided fmaf chain + wave_sum as cos_otam_kernel's query norms)
__global__ __launch_bounds__(256) void row_norms_kernel(const float* __restrict__ X, float* __restrict__ n, int R, int E) {
    const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= R) return;
    const float* x = X + (size_t)r * E;
    float ss = 0.f;
    for (int e = lane; e < E; e += 64) ss = fmaf(x[e], x[e], ss);
    ss = wave_sum(ss);
    if (lane == 0) n[r] = sqrtf(ss);
}

// ---- OTAM soft-min DP: the recurrence of tail.hip's otam_dp (few_shot.py:2657-2687), un-stabilised like the reference, in the same
// operation order, so equal distance blocks give bit-equal results.  The one difference is where the run-time-T rows live: `rstride`
// floats apart in the caller's LDS slot instead of a fixed MAX_T + 2.
constexpr int MAX_T = 32;
template <int TT>
__device__ __forceinline__ float otam_dp(const float* d /*[T][T] row stride rs, col stride cs*/, int rs, int cs, int Trt, float lbda,
                                         float* rows, int rstride) {
    const int T = TT > 0 ? TT : Trt;
    // padded width M = T+2; columns 0 and T+1 are zero padding (few_shot.py:2663)
    float regs[TT > 0 ? 2 * (TT + 2) : 1];
    float* prev = TT > 0 ? regs : rows;
    float* cur = TT > 0 ? regs + (TT + 2) : rows + rstride;
    const float il = 1.0f / lbda;
    prev[0] = 0.f;
#pragma unroll
    for (int m = 1; m <= T + 1; ++m) {                      // first row: running sum (:2668-2671)
        const float dv = (m <= T) ? d[0 * rs + (m - 1) * cs] : 0.f;
        prev[m] = dv + prev[m - 1];
    }
#pragma unroll
    for (int l = 1; l < T; ++l) {
        cur[0] = 0.f;
        {   // first non-zero column (:2675)
            const float dv = d[l * rs + 0 * cs];
            cur[1] = dv - lbda * logf(expf(-prev[0] * il) + expf(-prev[1] * il) + expf(-cur[0] * il));
        }
#pragma unroll
        for (int m = 2; m <= T; ++m) {                      // middle columns (:2678-2679)
            const float dv = d[l * rs + (m - 1) * cs];
            cur[m] = dv - lbda * logf(expf(-prev[m - 1] * il) + expf(-cur[m - 1] * il));
        }
        // last (padding) column (:2683)
        cur[T + 1] = 0.f - lbda * logf(expf(-prev[T] * il) + expf(-prev[T + 1] * il) + expf(-cur[T] * il));
#pragma unroll
        for (int m = 0; m <= T + 1; ++m) prev[m] = cur[m];
    }
    return prev[T + 1];
}

// ---- cos_sim + OTAM of a gallery.  A workgroup (4 waves) owns QB queries x QB classes: a TILE x TILE block of frame rows
// (T = 8: 8 x 8 videos, 64 pairs; T = 16: 4 x 4).
//   GEMM: [QB*T, E] x [QB*T, E]^T with v_mfma_f32_16x16x4_f32 (an exact fp32 fmaf chain per k step); both operands staged through LDS in
//   BK-float chunks, the next chunk's global loads in flight while the current one is multiplied.  Wave w owns the 32 x 32 quarter
//   (w >> 1, w & 1) as 2 x 2 MFMA tiles.  Inside a chunk, MFMA step s of lane half h takes k = 8h + s: every lane reads its k values as
//   two ds_read_b128 per tile (A and B use the same k map, so the products are those of the plain GEMM, summed in another order).
//   Epilogue: d = 1 - dot / (qn pn + 0.01) into an LDS image of the tile (aliasing the staging buffers), then one lane per
//   (pair, direction) runs the DP -- rows in registers for T = 8 / 16, in an LDS slot per thread for run-time T.
constexpr int TILE = 64, BK = 32, SLD = BK + 4 /* staging row stride: 16-B aligned rows */, DLD = TILE + 1 /* distance image */;
constexpr int MAX_PAIRS = 256;

__host__ __device__ inline int tile_videos(int T) { return TILE / T < 16 ? TILE / T : 16; }
__host__ __device__ inline int dp_slots(int T) {
    const int lanes = 2 * tile_videos(T) * tile_videos(T);
    return lanes < 256 ? lanes : 256;
}
// LDS floats: staging (A | B; the distance image reuses it) + norms + DP results (+ run-time-T DP rows)
__host__ __device__ inline int gallery_lds_floats(int T, bool fixed_t) {
    return 2 * TILE * SLD + 2 * TILE + 2 * MAX_PAIRS + (fixed_t ? 0 : dp_slots(T) * 2 * (T + 2));
}

__device__ __forceinline__ float4 load_row4(const float* __restrict__ X, size_t row, int col, int E, bool ok) {
    return ok ? *reinterpret_cast<const float4*>(X + row * E + col) : make_float4(0.f, 0.f, 0.f, 0.f);
}

template <int TT>
__global__ __launch_bounds__(256) void otam_gallery_kernel(const float* __restrict__ Xq, const float* __restrict__ qn,
                                                           const float* __restrict__ P, const float* __restrict__ pn,
                                                           float* __restrict__ logits, float* __restrict__ dists_out, int NQ, int C,
                                                           int Trt, int E, float lbda, int single_direct) {
    static_assert(TILE * DLD <= 2 * TILE * SLD, "the distance image must fit into the staging buffers");
    const int T = TT > 0 ? TT : Trt;
    const int QB = tile_videos(T);
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* sA = smem;                                  // [TILE][SLD]
    float* sB = smem + TILE * SLD;                     // [TILE][SLD]
    float* dist = smem;                                // [TILE][DLD], after the K loop
    float* sqn = smem + 2 * TILE * SLD;                // [TILE]
    float* spn = sqn + TILE;                           // [TILE]
    float* res = spn + TILE;                           // [2 * MAX_PAIRS]
    float* dprows = res + 2 * MAX_PAIRS;               // TT == 0: [dp_slots][2][T + 2]
    const int c0 = blockIdx.x * QB, q0 = blockIdx.y * QB;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t arow0 = (size_t)q0 * T, brow0 = (size_t)c0 * T;
    const int a_rows = min(QB, NQ - q0) * T, b_rows = min(QB, C - c0) * T;        // valid frame rows of each operand
    if (tid < TILE) sqn[tid] = tid < a_rows ? qn[arow0 + tid] : 1.f;
    else if (tid < 2 * TILE) spn[tid - TILE] = tid - TILE < b_rows ? pn[brow0 + tid - TILE] : 1.f;

    // staging: 2 float4 of A and 2 of B per thread and chunk; rows / columns outside the operands are zero (they add +0 to the sums)
    const int sr0 = tid >> 3, sr1 = (tid + 256) >> 3, sc = (tid & 7) * 4;          // staged rows of the two float4s, their column
    float4 ra0, ra1, rb0, rb1;
#define CFSG_LOAD_CHUNK(k0)                                                                                  \
    do {                                                                                                     \
        const int col_ = (k0) + sc;                                                                          \
        ra0 = load_row4(Xq, arow0 + sr0, col_, E, sr0 < a_rows && col_ < E);                                 \
        ra1 = load_row4(Xq, arow0 + sr1, col_, E, sr1 < a_rows && col_ < E);                                 \
        rb0 = load_row4(P, brow0 + sr0, col_, E, sr0 < b_rows && col_ < E);                                  \
        rb1 = load_row4(P, brow0 + sr1, col_, E, sr1 < b_rows && col_ < E);                                  \
    } while (0)
    f32x4 acc[2][2];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32, fr = lane & 15, fh = lane >> 4;
    CFSG_LOAD_CHUNK(0);
    for (int k0 = 0; k0 < E; k0 += BK) {
        __syncthreads();                                                  // the previous chunk's fragment reads are done
        *reinterpret_cast<float4*>(sA + sr0 * SLD + sc) = ra0;
        *reinterpret_cast<float4*>(sA + sr1 * SLD + sc) = ra1;
        *reinterpret_cast<float4*>(sB + sr0 * SLD + sc) = rb0;
        *reinterpret_cast<float4*>(sB + sr1 * SLD + sc) = rb1;
        __syncthreads();
        if (k0 + BK < E) CFSG_LOAD_CHUNK(k0 + BK);                                   // next chunk in flight during this one's MFMAs
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
#undef CFSG_LOAD_CHUNK
    __syncthreads();                                                      // the distance image overwrites the staging buffers
    // C/D map of the 16x16 MFMA: column = lane & 15, row = 4 (lane >> 4) + register
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int row = wm + 16 * mi + 4 * fh + g, col = wn + 16 * ni + fr;
                dist[row * DLD + col] = 1.0f - acc[mi][ni][g] / (sqn[row] * spn[col] + 0.01f);
            }
    __syncthreads();
    const int npairs = QB * QB, TT2 = T * T;
    if (dists_out) {
        for (int i = tid; i < npairs * TT2; i += 256) {
            const int pair = i / TT2, lm = i - pair * TT2, qi = pair / QB, cj = pair - qi * QB, l = lm / T, m = lm - l * T;
            if (q0 + qi < NQ && c0 + cj < C)
                dists_out[((size_t)(q0 + qi) * C + (c0 + cj)) * TT2 + lm] = dist[(qi * T + l) * DLD + cj * T + m];
        }
    }
    for (int p = tid; p < 2 * npairs; p += 256) {
        const int pair = p >> 1, dir = p & 1, qi = pair / QB, cj = pair - qi * QB;
        float v = 0.f;
        if (q0 + qi < NQ && c0 + cj < C && !(dir && single_direct)) {
            const float* d = dist + qi * T * DLD + cj * T;
            // dir 0: rows = query frames; dir 1: the transposed distances (:2982)
            v = otam_dp<TT>(d, dir ? 1 : DLD, dir ? DLD : 1, T, lbda, dprows + tid * 2 * (T + 2), T + 2);
        }
        res[p] = v;
    }
    __syncthreads();
    for (int pair = tid; pair < npairs; pair += 256) {
        const int qi = pair / QB, cj = pair - qi * QB;
        if (q0 + qi < NQ && c0 + cj < C) logits[(size_t)(q0 + qi) * C + (c0 + cj)] = -(res[2 * pair] + res[2 * pair + 1]);
    }
}

// ---- top-k per query: one wave per query.  Each lane keeps the best KMAX of its strided classes (a compare-exchange chain with
// constant indices: registers only), then k rounds of a wave-wide arg-max over the lanes' heads.  Order: larger value first, the
// lower class index on ties (a stable descending sort); NaN logits are never selected.
constexpr int KMAX = 16;
__device__ __forceinline__ bool topk_better(float a, int ia, float b, int ib) { return a > b || (a == b && ia < ib); }

__global__ __launch_bounds__(64) void topk_kernel(const float* __restrict__ logits, float* __restrict__ values,
                                                  int32_t* __restrict__ index, int C, int k) {
    const int q = blockIdx.x, lane = threadIdx.x;
    float v[KMAX];
    int ix[KMAX];
#pragma unroll
    for (int j = 0; j < KMAX; ++j) { v[j] = -__builtin_inff(); ix[j] = 0x7fffffff; }
    const float* row = logits + (size_t)q * C;
    for (int c = lane; c < C; c += 64) {
        float x = row[c];
        int xi = c;
#pragma unroll
        for (int j = 0; j < KMAX; ++j) {
            if (topk_better(x, xi, v[j], ix[j])) {
                const float tv = v[j];
                const int ti = ix[j];
                v[j] = x; ix[j] = xi; x = tv; xi = ti;
            }
        }
    }
    for (int r = 0; r < k; ++r) {
        float bv = v[0];
        int bi = ix[0];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(bv, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (topk_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
        }
        if (lane == 0) {
            values[(size_t)q * k + r] = bv;
            index[(size_t)q * k + r] = bi;
        }
        if (ix[0] == bi) {                                 // the winner's lane pops its head
#pragma unroll
            for (int j = 0; j < KMAX - 1; ++j) { v[j] = v[j + 1]; ix[j] = ix[j + 1]; }
            v[KMAX - 1] = -__builtin_inff();
            ix[KMAX - 1] = 0x7fffffff;
        }
    }
}

}  // namespace

extern "C" int cfsg_version(void) { return 100; /* 0.1.0 */ }
extern "C" int cfsg_abi_version(void) { return CFSG_ABI_VERSION; }
extern "C" const char* cfsg_last_error(void) { return g_err; }

extern "C" int cfsg_support_sequences(const float* feats, const float* text, const int32_t* cls_of_video, float* X, int Nv, int T, int E,
                                      int n_cls, cfsg_stream_t stream) {
    CFSG_REQUIRE(feats && text && cls_of_video && X, "cfsg_support_sequences: null pointer");
    CFSG_REQUIRE(Nv > 0 && T > 0 && E > 0 && n_cls > 0, "cfsg_support_sequences: bad shape (Nv=%d T=%d E=%d n_cls=%d)", Nv, T, E, n_cls);
    const long long rows = (long long)Nv * (T + 1);
    CFSG_REQUIRE(rows <= 0x7fffffffLL, "cfsg_support_sequences: %lld rows", rows);
    hipLaunchKernelGGL(support_sequences_kernel, dim3((unsigned)rows), dim3(128), 0, static_cast<hipStream_t>(stream), feats, text,
                       cls_of_video, X, T, E, n_cls);
    return check_launch("cfsg_support_sequences");
}

extern "C" int cfsg_segment_mean(const float* X, const int32_t* offsets, float* out, int Nv, int L, int E, int C, int rows_kept,
                                 cfsg_stream_t stream) {
    CFSG_REQUIRE(X && offsets && out, "cfsg_segment_mean: null pointer");
    CFSG_REQUIRE(Nv > 0 && L > 0 && E > 0 && C > 0 && rows_kept > 0 && rows_kept <= L,
                 "cfsg_segment_mean: bad shape (Nv=%d L=%d E=%d C=%d rows_kept=%d)", Nv, L, E, C, rows_kept);
    const long long blocks = (long long)C * rows_kept;
    CFSG_REQUIRE(blocks <= 0x7fffffffLL, "cfsg_segment_mean: %lld output rows", blocks);
    hipLaunchKernelGGL(segment_mean_kernel, dim3((unsigned)blocks), dim3(128), 0, static_cast<hipStream_t>(stream), X, offsets, out, Nv, L,
                       E, rows_kept);
    return check_launch("cfsg_segment_mean");
}

extern "C" int cfsg_row_norms(const float* X, float* n, int R, int E, cfsg_stream_t stream) {
    CFSG_REQUIRE(X && n, "cfsg_row_norms: null pointer");
    CFSG_REQUIRE(R > 0 && E > 0, "cfsg_row_norms: bad shape (R=%d E=%d)", R, E);
    hipLaunchKernelGGL(row_norms_kernel, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, static_cast<hipStream_t>(stream), X, n, R, E);
    return check_launch("cfsg_row_norms");
}

extern "C" int cfsg_otam_gallery(const float* Xq, const float* qn, const float* P, const float* pn, float* logits, float* dists_out, int NQ,
                                 int C, int T, int E, float lambda, int single_direct, cfsg_stream_t stream) {
    CFSG_REQUIRE(Xq && qn && P && pn && logits, "cfsg_otam_gallery: null pointer");
    CFSG_REQUIRE(NQ > 0 && C > 0 && T > 0 && T <= MAX_T && E >= 4 && E <= 8192 && E % 4 == 0,
                 "cfsg_otam_gallery: bad shape (NQ=%d C=%d T=%d E=%d; T <= 32, E %% 4 == 0, 4 <= E <= 8192)", NQ, C, T, E);
    CFSG_REQUIRE(lambda > 0.f, "cfsg_otam_gallery: lambda must be > 0");
    const int qb = tile_videos(T);
    const long long gx = ((long long)C + qb - 1) / qb, gy = ((long long)NQ + qb - 1) / qb;
    CFSG_REQUIRE(gy <= 65535, "cfsg_otam_gallery: NQ=%d too large for one launch (at most %d at T=%d)", NQ, 65535 * qb, T);
    const bool fixed_t = T == 8 || T == 16;                   // DP rows in registers; otherwise in an LDS slot per thread
    const int lds = gallery_lds_floats(T, fixed_t) * (int)sizeof(float);
    CFSG_REQUIRE(lds <= 48 * 1024, "cfsg_otam_gallery: LDS %d bytes", lds);
    auto launch = [&](auto kern) -> int {
        hipLaunchKernelGGL(kern, dim3((unsigned)gx, (unsigned)gy), dim3(256), lds, static_cast<hipStream_t>(stream), Xq, qn, P, pn, logits,
                           dists_out, NQ, C, T, E, lambda, single_direct);
        return check_launch("cfsg_otam_gallery");
    };
    if (T == 8) return launch(&otam_gallery_kernel<8>);
    if (T == 16) return launch(&otam_gallery_kernel<16>);
    return launch(&otam_gallery_kernel<0>);
}

extern "C" int cfsg_topk(const float* logits, float* values, int32_t* index, int NQ, int C, int k, cfsg_stream_t stream) {
    CFSG_REQUIRE(logits && values && index, "cfsg_topk: null pointer");
    CFSG_REQUIRE(NQ > 0 && C > 0 && C <= 65535 && k >= 1 && k <= KMAX && k <= C,
                 "cfsg_topk: bad shape (NQ=%d C=%d k=%d; 1 <= k <= 16, k <= C <= 65535)", NQ, C, k);
    hipLaunchKernelGGL(topk_kernel, dim3((unsigned)NQ), dim3(64), 0, static_cast<hipStream_t>(stream), logits, values, index, C, k);
    return check_launch("cfsg_topk");
}
