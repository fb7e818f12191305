// Live gallery (libclipfsar_live.so, C ABI in include/clipfsar_live.h): the gallery's cos_sim + OTAM kernel reading its classes through
// a column list over a prototype store of slots, the running per-class sums that take further shots, and the norms of updated slots.
// A library of its own: libclipfsar_gallery.so keeps exactly the entry points of include/clipfsar_gallery.h.
#include "otam_tile.h"
#include "../../include/clipfsar_live.h"

namespace {

// ---- cos_sim + OTAM over a column list: otam_tile (otam_tile.h), the body of otam_gallery_kernel (gallery.hip), over the slots of a store
// -- tile row r of the B operand is frame r % T of slot cols[c0 + r / T], and its norm comes from the same place (fp32_tile_gemm_rows
// asks for the row once per staged row, before the K loop).  The logits are those of the dense kernel on P_store[cols], bit for bit.
struct StoreSlots {
    const float* __restrict__ pn;
    const int32_t* __restrict__ cols;
    int cap;
    static constexpr bool POISONS = true;              // a bad slot: NaN norms poison its column
    // store row of tile row r, or -1: r is past the tile's classes, or its slot is outside [0, cap) (store_slot_row, otam_tile.h)
    __device__ __forceinline__ LookedUpRow row(int r, int c0, int b_rows, int T) const {
        return LookedUpRow{store_slot_row(cols, cap, r, c0, b_rows, T)};
    }
    __device__ __forceinline__ float norm(int r, int c0, int b_rows, int T) const {
        return store_slot_norm(pn, cols, cap, r, c0, b_rows, T);
    }
    __device__ __forceinline__ float* dists() const { return nullptr; }
};

template <int TT>
__global__ __launch_bounds__(256) void otam_indexed_kernel(const float* __restrict__ Xq, const float* __restrict__ qn,
                                                           const float* __restrict__ P, const float* __restrict__ pn,
                                                           const int32_t* __restrict__ cols, float* __restrict__ logits, int NQ, int C,
                                                           int cap, int Trt, int E, float lbda, int single_direct) {
    otam_tile<TT>(Xq, qn, P, StoreSlots{pn, cols, cap}, logits, NQ, C, Trt, E, lbda, single_direct);
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
    SlotBits seen(cap);
    SIDE_REQUIRE(seen.ok(), "%s: out of host memory for %d slots", who, cap);
    for (int s = 0; s < S; ++s) {
        const int slot = t[(size_t)s * CFSL_TABLE_COLS + CFSL_SLOT];
        SIDE_REQUIRE(slot >= 0 && slot < cap, "%s: row %d: slot %d outside [0, %d)", who, s, slot, cap);
        SIDE_REQUIRE(!seen.test_and_set(slot), "%s: row %d: slot %d appears twice in the table", who, s, slot);
    }
    return 0;
}

}  // namespace

extern "C" int cfsl_version(void) { return 100; /* 0.1.0 */ }
extern "C" int cfsl_abi_version(void) { return CFSL_ABI_VERSION; }
extern "C" const char* cfsl_last_error(void) { return g_err; }

extern "C" int cfsl_otam_indexed(const float* Xq, const float* qn, const float* P_store, const float* pn_store, const int32_t* cols,
                                 float* logits, int NQ, int C, int cap, int T, int E, float lambda, int single_direct,
                                 cfsl_stream_t stream) {
    SIDE_REQUIRE(Xq && qn && P_store && pn_store && cols && logits, "cfsl_otam_indexed: null pointer");
    SIDE_REQUIRE(otam_shape_ok(NQ, C, T, E) && cap >= 1,
                 "cfsl_otam_indexed: bad shape (NQ=%d C=%d cap=%d T=%d E=%d; C, cap >= 1, 1 <= T <= 32, E %% 4 == 0, 4 <= E <= 8192)", NQ, C,
                 cap, T, E);
    SIDE_REQUIRE((long long)cap * T <= 0x7fffffffLL && (long long)NQ * T <= 0x7fffffffLL,
                 "cfsl_otam_indexed: cap * T = %lld or NQ * T = %lld rows exceed 32-bit sizes", (long long)cap * T, (long long)NQ * T);
    return otam_tile_launch("cfsl_otam_indexed", Xq, P_store, "P_store", NQ, C, T, lambda, [&](auto tt, dim3 grid, int lds) {
        hipLaunchKernelGGL(otam_indexed_kernel<decltype(tt)::value>, grid, dim3(256), lds, static_cast<hipStream_t>(stream), Xq, qn, P_store,
                           pn_store, cols, logits, NQ, C, cap, T, E, lambda, single_direct);
    });
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
