// Live gallery (libclipfsar_live.so, C ABI in include/clipfsar_live.h): the gallery's cos_sim + OTAM kernel reading its classes through
// a column list over a prototype store of slots, the running per-class sums that take further shots, and the norms of updated slots.
// A library of its own: libclipfsar_gallery.so keeps exactly the entry points of include/clipfsar_gallery.h.
#include <stdint.h>
#include <stdlib.h>

#include "fp32_tile_gemm.h"
#include "otam_dp.h"
#include "side_lib.h"
#include "../../include/clipfsar_live.h"

namespace {

// ---- cos_sim + OTAM over a column list.  otam_gallery_kernel (gallery.hip) with ONE difference: tile row r of the B operand is frame
// r % T of slot cols[c0 + r / T] of the store, and its norm comes from the same place (store_row below; fp32_tile_gemm_rows asks it once
// per staged row, before the K loop).  Tile geometry, K loop, distance image, DP forms and the order of every fmaf chain are the dense
// kernel's, and an output element's chain does not depend on its place in a tile, so the logits are those of the dense kernel on
// P_store[cols], bit for bit.
constexpr int DLD = TILE + 1 /* distance image */;
constexpr int MAX_PAIRS = 256;

__host__ __device__ inline int tile_videos(int T) { return TILE / T < 16 ? TILE / T : 16; }
__host__ __device__ inline int dp_slots(int T) {
    const int lanes = 2 * tile_videos(T) * tile_videos(T);
    return lanes < 256 ? lanes : 256;
}
// LDS floats: staging (A | B; the distance image reuses it) + norms + DP results (+ run-time-T DP rows)
__host__ __device__ inline int indexed_lds_floats(int T, bool fixed_t) {
    return 2 * TILE * SLD + 2 * TILE + 2 * MAX_PAIRS + (fixed_t ? 0 : dp_slots(T) * 2 * (T + 2));
}

// store row of tile row r, or -1: r is past the tile's classes, or its slot is outside [0, cap) (never dereferenced)
__device__ __forceinline__ long long store_row(const int32_t* __restrict__ cols, int c0, int r, int b_rows, int T, int cap) {
    if (r >= b_rows) return -1;
    const int j = r / T, slot = cols[c0 + j];
    return (unsigned)slot < (unsigned)cap ? (long long)slot * T + (r - j * T) : -1;
}

template <int TT>
__global__ __launch_bounds__(256) void otam_indexed_kernel(const float* __restrict__ Xq, const float* __restrict__ qn,
                                                           const float* __restrict__ P, const float* __restrict__ pn,
                                                           const int32_t* __restrict__ cols, float* __restrict__ logits, int NQ, int C,
                                                           int cap, int Trt, int E, float lbda, int single_direct) {
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
    const size_t arow0 = (size_t)q0 * T;
    const int a_rows = min(QB, NQ - q0) * T, b_rows = min(QB, C - c0) * T;        // valid frame rows of each operand
    if (tid < TILE) {
        sqn[tid] = tid < a_rows ? qn[arow0 + tid] : 1.f;
    } else if (tid < 2 * TILE) {
        const int r = tid - TILE;
        const long long row = store_row(cols, c0, r, b_rows, T, cap);
        spn[r] = row >= 0 ? pn[row] : (r < b_rows ? __builtin_nanf("") : 1.f);    // a bad slot: NaN norms poison its column
    }

    f32x4 acc[2][2];
    fp32_tile_gemm_rows(Xq, arow0, a_rows, P, [=](int r) { return LookedUpRow{store_row(cols, c0, r, b_rows, T, cap)}; }, E, sA, sB, acc);
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
    const int npairs = QB * QB;
    for (int p = tid; p < 2 * npairs; p += 256) {
        const int pair = p >> 1, dir = p & 1, qi = pair / QB, cj = pair - qi * QB;
        float v = 0.f;
        if (q0 + qi < NQ && c0 + cj < C && !(dir && single_direct)) {
            const float* d = dist + qi * T * DLD + cj * T;
            // dir 0: rows = query frames; dir 1: the transposed distances
            v = otam_dp<TT>(d, dir ? 1 : DLD, dir ? DLD : 1, T, lbda, dprows + tid * 2 * (T + 2), T + 2);
        }
        res[p] = v;
    }
    __syncthreads();
    for (int pair = tid; pair < npairs; pair += 256) {
        const int qi = pair / QB, cj = pair - qi * QB;
        if (q0 + qi < NQ && c0 + cj < C) {
            const float pn0 = spn[cj * T];
            logits[(size_t)(q0 + qi) * C + (c0 + cj)] = pn0 != pn0 ? __builtin_nanf("") : -(res[2 * pair] + res[2 * pair + 1]);
        }
    }
}

// ---- further videos into the running sums: one workgroup per (table row, kept row).  segment_mean_kernel's (gallery.hip) operation
// order -- sum in video order, then * (1 / count) -- continued from the stored sum.  A row the host would have refused writes nothing.
__global__ __launch_bounds__(128) void accumulate_kernel(const float* __restrict__ X, float* __restrict__ sums, float* __restrict__ means,
                                                         const int32_t* __restrict__ table, int Nv, int L, int E, int cap, int rows_kept,
                                                         int means_by_slot) {
    const int s = blockIdx.x / rows_kept, r = blockIdx.x - s * rows_kept, tid = threadIdx.x;
    const int32_t* row = table + (size_t)s * CFSL_TABLE_COLS;
    const int slot = row[CFSL_SLOT], lo = row[CFSL_OFF], n = row[CFSL_N], prior = row[CFSL_PRIOR];
    if ((unsigned)slot >= (unsigned)cap || lo < 0 || n < 1 || n > Nv - lo || prior < 0) return;
    const int hi = lo + n;
    const float inv = 1.0f / (float)(prior + n);
    float* sm = sums + ((size_t)slot * L + r) * E;
    float* o = means + ((size_t)(means_by_slot ? slot : s) * rows_kept + r) * E;
    for (int e = tid; e < E; e += 128) {
        float a = prior ? sm[e] : 0.f;
        for (int v = lo; v < hi; ++v) a += X[((size_t)v * L + r) * E + e];
        sm[e] = a;
        o[e] = a * inv;
    }
}

// ---- norms of the table's slots: one wave per row, row_norms_kernel's (gallery.hip) lane-strided fmaf chain + wave_sum
__global__ __launch_bounds__(256) void slot_norms_kernel(const float* __restrict__ P, float* __restrict__ pn,
                                                         const int32_t* __restrict__ table, int R, int cap, int T, int E) {
    const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= R) return;
    const int s = r / T, slot = table[(size_t)s * CFSL_TABLE_COLS + CFSL_SLOT];
    if ((unsigned)slot >= (unsigned)cap) return;
    const size_t row = (size_t)slot * T + (r - s * T);
    const float* x = P + row * E;
    float ss = 0.f;
    for (int e = lane; e < E; e += 64) ss = fmaf(x[e], x[e], ss);
    ss = wave_sum(ss);
    if (lane == 0) pn[row] = sqrtf(ss);
}

// the host rows of a table: slots in [0, cap), each at most once
int check_slots(const char* who, const int32_t* t, int S, int cap) {
    SIDE_REQUIRE(S >= 1 && S <= CFSL_MAX_ROWS && S <= cap, "%s: a table of %d rows (1 .. min(%d, cap = %d))", who, S, CFSL_MAX_ROWS, cap);
    uint64_t* seen = static_cast<uint64_t*>(calloc(((size_t)cap + 63) / 64, sizeof(uint64_t)));      // a bit per slot
    SIDE_REQUIRE(seen, "%s: out of host memory for %d slots", who, cap);
    int rc = 0;
    for (int s = 0; s < S && !rc; ++s) {
        const int slot = t[(size_t)s * CFSL_TABLE_COLS + CFSL_SLOT];
        if (slot < 0 || slot >= cap) rc = fail("%s: row %d: slot %d outside [0, %d)", who, s, slot, cap);
        else if (seen[slot >> 6] >> (slot & 63) & 1) rc = fail("%s: row %d: slot %d appears twice in the table", who, s, slot);
        else seen[slot >> 6] |= (uint64_t)1 << (slot & 63);
    }
    free(seen);
    return rc;
}

}  // namespace

extern "C" int cfsl_version(void) { return 100; /* 0.1.0 */ }
extern "C" int cfsl_abi_version(void) { return CFSL_ABI_VERSION; }
extern "C" const char* cfsl_last_error(void) { return g_err; }

extern "C" int cfsl_otam_indexed(const float* Xq, const float* qn, const float* P_store, const float* pn_store, const int32_t* cols,
                                 float* logits, int NQ, int C, int cap, int T, int E, float lambda, int single_direct,
                                 cfsl_stream_t stream) {
    SIDE_REQUIRE(Xq && qn && P_store && pn_store && cols && logits, "cfsl_otam_indexed: null pointer");
    SIDE_REQUIRE(NQ > 0 && C >= 1 && cap >= 1 && T >= 1 && T <= MAX_T && E >= 4 && E <= 8192 && E % 4 == 0,
                 "cfsl_otam_indexed: bad shape (NQ=%d C=%d cap=%d T=%d E=%d; C, cap >= 1, 1 <= T <= 32, E %% 4 == 0, 4 <= E <= 8192)", NQ, C,
                 cap, T, E);
    SIDE_REQUIRE((long long)cap * T <= 0x7fffffffLL && (long long)NQ * T <= 0x7fffffffLL,
                 "cfsl_otam_indexed: cap * T = %lld or NQ * T = %lld rows exceed 32-bit sizes", (long long)cap * T, (long long)NQ * T);
    SIDE_REQUIRE(lambda > 0.f, "cfsl_otam_indexed: lambda must be > 0");
    const int qb = tile_videos(T);
    const long long gx = ((long long)C + qb - 1) / qb, gy = ((long long)NQ + qb - 1) / qb;
    SIDE_REQUIRE(gy <= 65535, "cfsl_otam_indexed: NQ=%d too large for one launch (at most %d at T=%d)", NQ, 65535 * qb, T);
    const bool fixed_t = T == 8 || T == 16;                   // DP rows in registers; otherwise in an LDS slot per thread
    const int lds = indexed_lds_floats(T, fixed_t) * (int)sizeof(float);
    SIDE_REQUIRE(lds <= 48 * 1024, "cfsl_otam_indexed: LDS %d bytes", lds);
    auto launch = [&](auto kern) -> int {
        hipLaunchKernelGGL(kern, dim3((unsigned)gx, (unsigned)gy), dim3(256), lds, static_cast<hipStream_t>(stream), Xq, qn, P_store,
                           pn_store, cols, logits, NQ, C, cap, T, E, lambda, single_direct);
        return check_launch("cfsl_otam_indexed");
    };
    if (T == 8) return launch(&otam_indexed_kernel<8>);
    if (T == 16) return launch(&otam_indexed_kernel<16>);
    return launch(&otam_indexed_kernel<0>);
}

extern "C" int cfsl_accumulate(const float* X, float* sums, float* means, const int32_t* table_host, const int32_t* table_dev, int S, int Nv,
                               int L, int E, int cap, int rows_kept, int means_by_slot, cfsl_stream_t stream) {
    SIDE_REQUIRE(X && sums && means && table_host && table_dev, "cfsl_accumulate: null pointer");
    SIDE_REQUIRE(Nv > 0 && L > 0 && E > 0 && cap >= 1 && rows_kept > 0 && rows_kept <= L,
                 "cfsl_accumulate: bad shape (Nv=%d L=%d E=%d cap=%d rows_kept=%d)", Nv, L, E, cap, rows_kept);
    if (check_slots("cfsl_accumulate", table_host, S, cap)) return 1;
    long long off = 0;
    for (int s = 0; s < S; ++s) {
        const int32_t* row = table_host + (size_t)s * CFSL_TABLE_COLS;
        SIDE_REQUIRE(row[CFSL_N] >= 1, "cfsl_accumulate: row %d: a run of %d videos, at least 1 is needed", s, row[CFSL_N]);
        SIDE_REQUIRE(row[CFSL_PRIOR] >= 0, "cfsl_accumulate: row %d: %d prior videos", s, row[CFSL_PRIOR]);
        SIDE_REQUIRE(row[CFSL_OFF] == off, "cfsl_accumulate: row %d: run offset %d is not the prefix sum %lld of the counts before", s,
                     row[CFSL_OFF], off);
        off += row[CFSL_N];
        SIDE_REQUIRE((long long)row[CFSL_PRIOR] + row[CFSL_N] <= 0x7fffffffLL, "cfsl_accumulate: row %d: the shot count exceeds 32-bit sizes", s);
    }
    SIDE_REQUIRE(off == Nv, "cfsl_accumulate: the runs add up to %lld videos, not to Nv = %d", off, Nv);
    const long long blocks = (long long)S * rows_kept;
    SIDE_REQUIRE(blocks <= 0x7fffffffLL, "cfsl_accumulate: %lld output rows exceed 32-bit sizes", blocks);
    hipLaunchKernelGGL(accumulate_kernel, dim3((unsigned)blocks), dim3(128), 0, static_cast<hipStream_t>(stream), X, sums, means, table_dev,
                       Nv, L, E, cap, rows_kept, means_by_slot);
    return check_launch("cfsl_accumulate");
}

extern "C" int cfsl_slot_norms(const float* P_store, float* pn_store, const int32_t* table_host, const int32_t* table_dev, int S, int cap,
                               int T, int E, cfsl_stream_t stream) {
    SIDE_REQUIRE(P_store && pn_store && table_host && table_dev, "cfsl_slot_norms: null pointer");
    SIDE_REQUIRE(cap >= 1 && T >= 1 && E > 0, "cfsl_slot_norms: bad shape (cap=%d T=%d E=%d)", cap, T, E);
    SIDE_REQUIRE((long long)cap * T <= 0x7fffffffLL, "cfsl_slot_norms: cap * T = %lld rows exceed 32-bit sizes", (long long)cap * T);
    if (check_slots("cfsl_slot_norms", table_host, S, cap)) return 1;
    const int R = S * T;
    hipLaunchKernelGGL(slot_norms_kernel, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, static_cast<hipStream_t>(stream), P_store, pn_store,
                       table_dev, R, cap, T, E);
    return check_launch("cfsl_slot_norms");
}
