// Support gallery (libclipfsar_gallery.so, C ABI in include/clipfsar_gallery.h): support sequences of any number of videos,
// per-class means over contiguous runs of videos, row norms, top-k, and the hot kernel -- cos_sim + OTAM of every (query, class)
// pair of a gallery (few_shot.py:1115-1124, 2657-2687, 2970-2990) as one exact-fp32 MFMA GEMM with the soft-min DPs in its epilogue.
// A library of its own: libclipfsar_hip.so keeps exactly the entry points of include/clipfsar_hip.h.
#include "otam_tile.h"
#include "topk_wave.h"
#include "../../include/clipfsar_gallery.h"

namespace {

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

// ---- cos_sim + OTAM of a gallery: otam_tile (otam_tile.h) over dense classes -- tile row r of B is row c0 * T + r of P (the identity map
// of fp32_tile_gemm.h), its norm the same row of pn
struct DenseClasses {
    const float* __restrict__ pn;
    float* __restrict__ dists_out;
    static constexpr bool POISONS = false;
    __device__ __forceinline__ TileRows::Row row(int r, int c0, int b_rows, int T) const { return TileRows{(size_t)c0 * T, b_rows}(r); }
    __device__ __forceinline__ float norm(int r, int c0, int b_rows, int T) const { return r < b_rows ? pn[(size_t)c0 * T + r] : 1.f; }
    __device__ __forceinline__ float* dists() const { return dists_out; }
};

template <int TT>
__global__ __launch_bounds__(256) void otam_gallery_kernel(const float* __restrict__ Xq, const float* __restrict__ qn,
                                                           const float* __restrict__ P, const float* __restrict__ pn,
                                                           float* __restrict__ logits, float* __restrict__ dists_out, int NQ, int C,
                                                           int Trt, int E, float lbda, int single_direct) {
    otam_tile<TT>(Xq, qn, P, DenseClasses{pn, dists_out}, logits, NQ, C, Trt, E, lbda, single_direct);
}

// ---- top-k per query: one wave per query, topk_wave (topk_wave.h)
__global__ __launch_bounds__(64) void topk_kernel(const float* __restrict__ logits, float* __restrict__ values,
                                                  int32_t* __restrict__ index, int C, int k) {
    const size_t q = blockIdx.x;
    topk_wave(logits + q * C, C, k, values + q * k, index + q * k, threadIdx.x);
}

}  // namespace

extern "C" int cfsg_version(void) { return 100; /* 0.1.0 */ }
extern "C" int cfsg_abi_version(void) { return CFSG_ABI_VERSION; }
extern "C" const char* cfsg_last_error(void) { return g_err; }

extern "C" int cfsg_support_sequences(const float* feats, const float* text, const int32_t* cls_of_video, float* X, int Nv, int T, int E,
                                      int n_cls, cfsg_stream_t stream) {
    SIDE_REQUIRE(feats && text && cls_of_video && X, "cfsg_support_sequences: null pointer");
    SIDE_REQUIRE(Nv > 0 && T > 0 && E > 0 && n_cls > 0, "cfsg_support_sequences: bad shape (Nv=%d T=%d E=%d n_cls=%d)", Nv, T, E, n_cls);
    const long long rows = (long long)Nv * (T + 1);
    SIDE_REQUIRE(rows <= 0x7fffffffLL, "cfsg_support_sequences: %lld rows", rows);
    hipLaunchKernelGGL(support_sequences_kernel, dim3((unsigned)rows), dim3(128), 0, static_cast<hipStream_t>(stream), feats, text,
                       cls_of_video, X, T, E, n_cls);
    return check_launch("cfsg_support_sequences");
}

extern "C" int cfsg_segment_mean(const float* X, const int32_t* offsets, float* out, int Nv, int L, int E, int C, int rows_kept,
                                 cfsg_stream_t stream) {
    SIDE_REQUIRE(X && offsets && out, "cfsg_segment_mean: null pointer");
    SIDE_REQUIRE(Nv > 0 && L > 0 && E > 0 && C > 0 && rows_kept > 0 && rows_kept <= L,
                 "cfsg_segment_mean: bad shape (Nv=%d L=%d E=%d C=%d rows_kept=%d)", Nv, L, E, C, rows_kept);
    const long long blocks = (long long)C * rows_kept;
    SIDE_REQUIRE(blocks <= 0x7fffffffLL, "cfsg_segment_mean: %lld output rows", blocks);
    hipLaunchKernelGGL(segment_mean_kernel, dim3((unsigned)blocks), dim3(128), 0, static_cast<hipStream_t>(stream), X, offsets, out, Nv, L,
                       E, rows_kept);
    return check_launch("cfsg_segment_mean");
}

extern "C" int cfsg_row_norms(const float* X, float* n, int R, int E, cfsg_stream_t stream) {
    SIDE_REQUIRE(X && n, "cfsg_row_norms: null pointer");
    SIDE_REQUIRE(R > 0 && E > 0, "cfsg_row_norms: bad shape (R=%d E=%d)", R, E);
    hipLaunchKernelGGL(row_norms_kernel, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, static_cast<hipStream_t>(stream), X, n, R, E);
    return check_launch("cfsg_row_norms");
}

extern "C" int cfsg_otam_gallery(const float* Xq, const float* qn, const float* P, const float* pn, float* logits, float* dists_out, int NQ,
                                 int C, int T, int E, float lambda, int single_direct, cfsg_stream_t stream) {
    SIDE_REQUIRE(Xq && qn && P && pn && logits, "cfsg_otam_gallery: null pointer");
    SIDE_REQUIRE(otam_shape_ok(NQ, C, T, E), "cfsg_otam_gallery: bad shape (NQ=%d C=%d T=%d E=%d; T <= 32, E %% 4 == 0, 4 <= E <= 8192)", NQ, C,
                 T, E);
    return otam_tile_launch("cfsg_otam_gallery", Xq, P, "P", NQ, C, T, lambda, [&](auto tt, dim3 grid, int lds) {
        hipLaunchKernelGGL(otam_gallery_kernel<decltype(tt)::value>, grid, dim3(256), lds, static_cast<hipStream_t>(stream), Xq, qn, P, pn,
                           logits, dists_out, NQ, C, T, E, lambda, single_direct);
    });
}

extern "C" int cfsg_topk(const float* logits, float* values, int32_t* index, int NQ, int C, int k, cfsg_stream_t stream) {
    SIDE_REQUIRE(logits && values && index, "cfsg_topk: null pointer");
    SIDE_REQUIRE(NQ > 0 && C > 0 && C <= 65535 && k >= 1 && k <= TOPK_MAX && k <= C,
                 "cfsg_topk: bad shape (NQ=%d C=%d k=%d; 1 <= k <= 16, k <= C <= 65535)", NQ, C, k);
    hipLaunchKernelGGL(topk_kernel, dim3((unsigned)NQ), dim3(64), 0, static_cast<hipStream_t>(stream), logits, values, index, C, k);
    return check_launch("cfsg_topk");
}
