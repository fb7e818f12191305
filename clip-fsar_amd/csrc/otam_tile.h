// cos_sim + OTAM of one workgroup's tile: the body of otam_gallery_kernel (gallery.hip), otam_indexed_kernel (live.hip) and
// otam_grouped_kernel (groups.hip), and the host checks, grid and T dispatch of their entry points.  A workgroup (4 waves) owns QB queries
// x QB classes: a TILE x TILE block of frame rows (T = 8: 8 x 8 videos, 64 pairs; T = 16: 4 x 4).
//   GEMM: [QB*T, E] x [QB*T, E]^T, fp32_tile_gemm_rows (fp32_tile_gemm.h).
//   Epilogue: d = 1 - dot / (qn pn + 0.01) into an LDS image of the tile (aliasing the staging buffers), then one lane per
//   (pair, direction) runs the DP -- rows in registers for T = 8 / 16, in an LDS slot per thread for run-time T.
// The kernels differ in their B-ROW SOURCE, a struct decided at compile time that says where the classes of a tile are:
//   row(r, c0, b_rows, T)    the fp32_tile_gemm_rows handle of tile row r (the tile's first class is c0, b_rows of its frame rows exist)
//   norm(r, c0, b_rows, T)   that row's norm (1.f for a padding row)
//   POISONS                  a class whose first norm is NaN gets NaN logits
//   dists()                  where to dump the tile's distances ([NQ, C, T, T]), or nullptr
// An output element's fmaf chain does not depend on the source or on its place in a tile: equal rows give equal bits from both kernels.
// The body, otam_tile_at, takes its tile's origin (q0, c0) as arguments: otam_tile reads it from the 2-D blockIdx of one (NQ, C) rectangle,
// otam_grouped_kernel (groups.hip) from a tile scheduler over a ragged list of rectangles, with each rectangle's base pointers and counts.
#pragma once
#include <type_traits>

#include "fp32_tile_gemm.h"
#include "otam_dp.h"
#include "side_lib.h"

constexpr int DLD = TILE + 1 /* distance image */;
constexpr int MAX_PAIRS = 256;

__host__ __device__ inline int tile_videos(int T) { return TILE / T < 16 ? TILE / T : 16; }
__host__ __device__ inline int dp_slots(int T) {
    const int lanes = 2 * tile_videos(T) * tile_videos(T);
    return lanes < 256 ? lanes : 256;
}
// LDS floats: staging (A | B; the distance image reuses it) + norms + DP results (+ run-time-T DP rows)
__host__ __device__ inline int otam_tile_lds_floats(int T, bool fixed_t) {
    return 2 * TILE * SLD + 2 * TILE + 2 * MAX_PAIRS + (fixed_t ? 0 : dp_slots(T) * 2 * (T + 2));
}

// A column list over a prototype store (StoreSlots in live.hip, GroupSlots in groups.hip): the store row of tile row r, or -1 -- r is past
// the tile's classes, or its slot is outside [0, cap) (never dereferenced) -- and that row's norm (NaN for a bad slot, 1.f for padding)
__device__ __forceinline__ long long store_slot_row(const int32_t* __restrict__ cols, int cap, int r, int c0, int b_rows, int T) {
    if (r >= b_rows) return -1;
    const int j = r / T, slot = cols[c0 + j];
    return (unsigned)slot < (unsigned)cap ? (long long)slot * T + (r - j * T) : -1;
}
__device__ __forceinline__ float store_slot_norm(const float* __restrict__ pn, const int32_t* __restrict__ cols, int cap, int r, int c0,
                                                 int b_rows, int T) {
    const long long row = store_slot_row(cols, cap, r, c0, b_rows, T);
    return row >= 0 ? pn[row] : (r < b_rows ? __builtin_nanf("") : 1.f);
}

template <int TT, class BSource>
__device__ __forceinline__ void otam_tile_at(const int q0, const int c0, const float* __restrict__ Xq, const float* __restrict__ qn,
                                             const float* __restrict__ P, const BSource src, float* __restrict__ logits, int NQ, int C,
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
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t arow0 = (size_t)q0 * T;
    const int a_rows = min(QB, NQ - q0) * T, b_rows = min(QB, C - c0) * T;        // valid frame rows of each operand
    if (tid < TILE) sqn[tid] = tid < a_rows ? qn[arow0 + tid] : 1.f;
    else if (tid < 2 * TILE) spn[tid - TILE] = src.norm(tid - TILE, c0, b_rows, T);

    f32x4 acc[2][2];
    // ends with a barrier: the distance image overwrites the staging buffers
    fp32_tile_gemm_rows(Xq, arow0, a_rows, P, [=](int r) { return src.row(r, c0, b_rows, T); }, E, sA, sB, acc);
    const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32, fr = lane & 15, fh = lane >> 4;
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
    if (float* dists_out = src.dists()) {
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
            // dir 0: rows = query frames; dir 1: the transposed distances (few_shot.py:2982)
            v = otam_dp<TT>(d, dir ? 1 : DLD, dir ? DLD : 1, T, lbda, dprows + tid * 2 * (T + 2), T + 2);
        }
        res[p] = v;
    }
    __syncthreads();
    for (int pair = tid; pair < npairs; pair += 256) {
        const int qi = pair / QB, cj = pair - qi * QB;
        if (q0 + qi < NQ && c0 + cj < C) {
            bool poisoned = false;
            if constexpr (BSource::POISONS) poisoned = spn[cj * T] != spn[cj * T];
            logits[(size_t)(q0 + qi) * C + (c0 + cj)] = poisoned ? __builtin_nanf("") : -(res[2 * pair] + res[2 * pair + 1]);
        }
    }
}

// the tile of one (NQ, C) rectangle launched as a 2-D grid: class tiles along x, query tiles along y
template <int TT, class BSource>
__device__ __forceinline__ void otam_tile(const float* __restrict__ Xq, const float* __restrict__ qn, const float* __restrict__ P,
                                          const BSource src, float* __restrict__ logits, int NQ, int C, int Trt, int E, float lbda,
                                          int single_direct) {
    const int QB = tile_videos(TT > 0 ? TT : Trt);
    otam_tile_at<TT>(blockIdx.y * QB, blockIdx.x * QB, Xq, qn, P, src, logits, NQ, C, Trt, E, lbda, single_direct);
}

// ---- host side of the entry points
inline bool otam_shape_ok(int NQ, int C, int T, int E) {
    return NQ > 0 && C > 0 && T > 0 && T <= MAX_T && E >= 4 && E <= 8192 && E % 4 == 0;
}

// The LDS size of an OTAM tile kernel over `grid` and its form for T: launch(tt, grid, lds_bytes) gets
// tt = std::integral_constant<int, 8 / 16 / 0 (run-time T)> and launches its kernel<tt.value> with 256 threads.
template <class Launch>
int otam_tile_forms(const char* who, int T, dim3 grid, Launch launch) {
    const bool fixed_t = T == 8 || T == 16;                   // DP rows in registers; otherwise in an LDS slot per thread
    const int lds = otam_tile_lds_floats(T, fixed_t) * (int)sizeof(float);
    SIDE_REQUIRE(lds <= 48 * 1024, "%s: LDS %d bytes", who, lds);
    if (T == 8) launch(std::integral_constant<int, 8>{}, grid, lds);
    else if (T == 16) launch(std::integral_constant<int, 16>{}, grid, lds);
    else launch(std::integral_constant<int, 0>{}, grid, lds);
    return check_launch(who);
}

// The checks after the shapes of a kernel over one (NQ, C) rectangle, and its 2-D grid; then otam_tile_forms.  Xq and P (named `pname` in
// the message) are the two GEMM operands: fp32_tile_gemm_rows reads them as float4, so both must be 16-byte aligned (with E % 4 == 0 every
// row then is); a pointer that is not is refused here, before any launch.
template <class Launch>
int otam_tile_launch(const char* who, const float* Xq, const float* P, const char* pname, int NQ, int C, int T, float lambda,
                     Launch launch) {
    SIDE_REQUIRE(((uintptr_t)Xq & 15u) == 0 && ((uintptr_t)P & 15u) == 0, "%s: Xq and %s must be 16-byte aligned", who, pname);
    SIDE_REQUIRE(lambda > 0.f, "%s: lambda must be > 0", who);
    const int qb = tile_videos(T);
    const long long gx = ((long long)C + qb - 1) / qb, gy = ((long long)NQ + qb - 1) / qb;
    SIDE_REQUIRE(gy <= 65535, "%s: NQ=%d too large for one launch (at most %d at T=%d)", who, NQ, 65535 * qb, T);
    return otam_tile_forms(who, T, dim3((unsigned)gx, (unsigned)gy), launch);
}
