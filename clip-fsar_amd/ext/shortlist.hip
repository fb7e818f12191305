// The coarse stage of two-stage scoring (libclipfsar_shortlist.so, C ABI in include/ext/clipfsar_shortlist.h): one [E] row per sequence
// (the mean of its unit-normalised rows), the coarse scores of every (query, class) pair as one exact-fp32 GEMM, and the selection that
// turns them into per-group slot lists on the device, where cfgr_otam_grouped (groups.hip) reads them.  The pieces are the tree's where
// they exist: the K loop is fp32_tile_gemm_rows with a looked-up B row (fp32_tile_gemm.h), the slot arithmetic is store_slot_row at one
// row per class (otam_tile.h), as live_text.hip uses both.  What is new is select_kernel (its body in select_keys.h): a threshold select
// -- the K-th largest group score by radix passes over order-preserving keys, then a scan that compacts the columns above the threshold
// and the first few equal to it in ascending column order.  A record's place is a prefix sum, never the outcome of a race; the only
// atomics are the histogram counts in LDS, whose sums do not depend on their order.
// A plug-in library (build.py, PLUGIN_LIBS): it lives beside csrc/, whose files and export sets stay as they are.
#include "../csrc/otam_tile.h"
#include "../../include/ext/clipfsar_shortlist.h"
#include "select_keys.h"

#include <math.h>

namespace {

constexpr int COLS = CFSH_TABLE_COLS;
constexpr int WG = SEL_WG, WAVES = SEL_WAVES;
constexpr long long MAX_32 = 0x7fffffffLL;

// ---- the coarse row: one thread per float4 column of a sequence, sequential in t -- adjacent threads on adjacent columns, the norm a
// broadcast load.  A rounded quotient, then a rounded sum: contraction off, and a division cannot fuse into the add anyway.
__global__ __launch_bounds__(WG) void mean_unit_rows_kernel(const float* __restrict__ X, const float* __restrict__ norms,
                                                            const int32_t* __restrict__ slots, float* __restrict__ out, unsigned cap,
                                                            int T, int E) {
#pragma clang fp contract(off)
    const unsigned b = slots ? (unsigned)slots[blockIdx.x] : blockIdx.x;
    const int e = (blockIdx.y * WG + threadIdx.x) * 4;
    if (b >= cap || e >= E) return;                                           // a slot outside the store: never dereferenced
    const float* x = X + (size_t)b * T * E + e;
    const float* n = norms + (size_t)b * T;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int t = 0; t < T; ++t) {
        const float4 v = *reinterpret_cast<const float4*>(x + (size_t)t * E);
        const float d = fmaxf(n[t], CFSH_TINY);
        acc.x = acc.x + __fdiv_rn(v.x, d);
        acc.y = acc.y + __fdiv_rn(v.y, d);
        acc.z = acc.z + __fdiv_rn(v.z, d);
        acc.w = acc.w + __fdiv_rn(v.w, d);
    }
    const float inv = __fdiv_rn(1.0f, (float)T);
    *reinterpret_cast<float4*>(out + (size_t)b * E + e) = make_float4(acc.x * inv, acc.y * inv, acc.z * inv, acc.w * inv);
}

// ---- the coarse scores: a 64 x 64 tile of U x C_store[cols]^T per workgroup, class tiles along x, query tiles along y
struct CoarseSlots {
    const int32_t* __restrict__ cols;
    int cap, c0, b_rows;
    __device__ __forceinline__ LookedUpRow operator()(int r) const { return LookedUpRow{store_slot_row(cols, cap, r, c0, b_rows, 1)}; }
};

__global__ __launch_bounds__(WG) void coarse_scores_kernel(const float* __restrict__ U, const float* __restrict__ C,
                                                           const int32_t* __restrict__ cols, float* __restrict__ S, int NQ, int NC,
                                                           int cap, int E) {
    __shared__ __attribute__((aligned(16))) float smem[2 * TILE * SLD];
    __shared__ int bad[TILE];                                                 // the tile's columns whose slot is outside the store
    const int q0 = blockIdx.y * TILE, c0 = blockIdx.x * TILE;
    const int a_rows = min(TILE, NQ - q0), b_rows = min(TILE, NC - c0);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < TILE) bad[tid] = tid < b_rows && store_slot_row(cols, cap, tid, c0, b_rows, 1) < 0;
    f32x4 acc[2][2];
    fp32_tile_gemm_rows(U, (size_t)q0, a_rows, C, CoarseSlots{cols, cap, c0, b_rows}, E, smem, smem + TILE * SLD, acc);   // ends with a barrier
    const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32, fr = lane & 15, fh = lane >> 4;
    // C/D map of the 16x16 MFMA: column = lane & 15, row = 4 (lane >> 4) + register
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int row = wm + 16 * mi + 4 * fh + g, col = wn + 16 * ni + fr;
                if (row < a_rows && col < b_rows) S[(size_t)(q0 + row) * NC + c0 + col] = bad[col] ? __builtin_nanf("") : acc[mi][ni][g];
            }
}

// ---- the selection: the keys, the radix passes and the compaction are select_keys.h's, shared with pool_select.hip
__global__ __launch_bounds__(WG) void select_kernel(const float* __restrict__ S, const int32_t* __restrict__ cols,
                                                    const int32_t* __restrict__ table, unsigned* __restrict__ work, int NQ, int NC, int K,
                                                    int32_t* __restrict__ sel_cols, int32_t* __restrict__ sel_slots) {
    __shared__ unsigned hist[WAVES * 256];                                    // a histogram per wave
    __shared__ unsigned part[WAVES];
    __shared__ unsigned pick[2];                                              // the pass's digit, and what is left of K below it
    const int tid = threadIdx.x;
    const unsigned g = blockIdx.x;
    int q_first = table[g * COLS + CFSH_Q0], nq = table[g * COLS + CFSH_NQ];
    if (q_first < 0 || nq < 0 || (long long)q_first + nq > NQ) nq = 0;        // a device table that is not the validated host rows
    unsigned* keys = work + (size_t)g * NC;
    // 1. the group scores, as keys: a thread per column, the queries' rows one after the other (coalesced at every q)
    for (int c = tid; c < NC; c += WG) keys[c] = group_score_key(S, q_first, nq, NC, c);
    __syncthreads();
    // 2. the K-th largest key; `left` of the keys equal to it are kept, the lowest columns first.  A threshold of 0 means fewer than K
    // columns are selectable: every key above 0 is kept and nothing else.
    unsigned left;
    const unsigned thr = kth_largest_key(keys, NC, (unsigned)K, hist, pick, [&](unsigned cell) { atomicAdd(&hist[cell], 1u); }, left);
    // 3. compaction in ascending column order, then the padding, at the end
    int32_t* oc = sel_cols + (size_t)g * K;
    int32_t* os = sel_slots + (size_t)g * K;
    const unsigned n_out = compact_selected(keys, NC, (unsigned)K, thr, thr ? left : 0u, part, [&](unsigned at, int c) {
        oc[at] = c;
        os[at] = cols[c];
    });
    for (unsigned r = n_out + tid; r < (unsigned)K; r += WG) {
        oc[r] = CFSH_NONE;
        os[r] = -1;
    }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace

extern "C" int cfsh_version(void) { return 100; /* 0.1.0 */ }
extern "C" int cfsh_abi_version(void) { return CFSH_ABI_VERSION; }
extern "C" const char* cfsh_last_error(void) { return g_err; }

extern "C" int cfsh_mean_unit_rows(const float* X, const float* norms, const int32_t* slots_or_null, float* out, int n, int cap, int T,
                                   int E, cfsh_stream_t stream) {
    const char* who = "cfsh_mean_unit_rows";
    SIDE_REQUIRE(X && norms && out, "%s: null pointer (X, norms or out; slots alone may be null)", who);
    SIDE_REQUIRE(n >= 1, "%s: n=%d sequences, at least 1 is needed", who, n);
    SIDE_REQUIRE(cap >= 1, "%s: cap=%d blocks, at least 1 is needed", who, cap);
    SIDE_REQUIRE(T >= 1 && T <= CFSH_MAX_T, "%s: T=%d outside 1 .. %d", who, T, CFSH_MAX_T);
    SIDE_REQUIRE(E >= 4 && E <= 8192 && E % 4 == 0, "%s: E=%d must be a multiple of 4 in 4 .. 8192", who, E);
    SIDE_REQUIRE((long long)cap * T <= MAX_32, "%s: cap * T = %lld rows exceed 32-bit sizes", who, (long long)cap * T);
    SIDE_REQUIRE(slots_or_null || n <= cap, "%s: n=%d sequences without a slot list, but cap=%d blocks", who, n, cap);
    SIDE_REQUIRE(aligned16(X) && aligned16(out), "%s: X and out must be 16-byte aligned", who);
    hipLaunchKernelGGL(mean_unit_rows_kernel, dim3((unsigned)n, (unsigned)((E / 4 + WG - 1) / WG)), dim3(WG), 0,
                       static_cast<hipStream_t>(stream), X, norms, slots_or_null, out, (unsigned)cap, T, E);
    return check_launch(who);
}

extern "C" int cfsh_coarse_scores(const float* U, const float* C_store, const int32_t* cols, float* S, int NQ, int NC, int cap, int E,
                                  cfsh_stream_t stream) {
    const char* who = "cfsh_coarse_scores";
    SIDE_REQUIRE(U && C_store && cols && S, "%s: null pointer", who);
    SIDE_REQUIRE(NQ >= 1, "%s: NQ=%d queries, at least 1 is needed", who, NQ);
    SIDE_REQUIRE(NC >= 1, "%s: NC=%d columns, at least 1 is needed", who, NC);
    SIDE_REQUIRE(cap >= 1, "%s: cap=%d slots, at least 1 is needed", who, cap);
    SIDE_REQUIRE(E >= 4 && E <= 8192 && E % 4 == 0, "%s: E=%d must be a multiple of 4 in 4 .. 8192", who, E);
    SIDE_REQUIRE((long long)NQ * NC <= MAX_32, "%s: NQ * NC = %lld scores exceed 32-bit sizes", who, (long long)NQ * NC);
    SIDE_REQUIRE(aligned16(U) && aligned16(C_store), "%s: U and C_store must be 16-byte aligned", who);
    const long long gy = ((long long)NQ + TILE - 1) / TILE;
    SIDE_REQUIRE(gy <= 65535, "%s: NQ=%d too large for one launch (at most %d)", who, NQ, 65535 * TILE);
    hipLaunchKernelGGL(coarse_scores_kernel, dim3((unsigned)((NC + TILE - 1) / TILE), (unsigned)gy), dim3(WG), 0,
                       static_cast<hipStream_t>(stream), U, C_store, cols, S, NQ, NC, cap, E);
    return check_launch(who);
}

extern "C" int cfsh_workspace_floats(int G, int NC) {
    if (G < 1 || G > CFSH_MAX_GROUPS || NC < 1 || (long long)G * NC > MAX_32) return -1;
    return G * NC;
}

extern "C" int cfsh_select(const float* S, const int32_t* cols, const int32_t* table_host, const int32_t* table_dev, int G, int NQ, int NC,
                           int keep, int32_t* sel_cols, int32_t* sel_slots, float* work, cfsh_stream_t stream) {
    const char* who = "cfsh_select";
    SIDE_REQUIRE(S && cols && table_host && table_dev && sel_cols && sel_slots && work, "%s: null pointer", who);
    SIDE_REQUIRE(G >= 1 && G <= CFSH_MAX_GROUPS, "%s: a table of G=%d groups (1 .. %d)", who, G, CFSH_MAX_GROUPS);
    SIDE_REQUIRE(NQ >= 1, "%s: NQ=%d queries, at least 1 is needed", who, NQ);
    SIDE_REQUIRE(NC >= 1, "%s: NC=%d columns, at least 1 is needed", who, NC);
    SIDE_REQUIRE(keep >= 1 && keep <= CFSH_MAX_KEEP, "%s: keep=%d outside 1 .. %d", who, keep, CFSH_MAX_KEEP);
    SIDE_REQUIRE((long long)NQ * NC <= MAX_32, "%s: NQ * NC = %lld scores exceed 32-bit sizes", who, (long long)NQ * NC);
    SIDE_REQUIRE((long long)G * NC <= MAX_32, "%s: G * NC = %lld group scores exceed 32-bit sizes", who, (long long)G * NC);
    long long q = 0;
    for (int g = 0; g < G; ++g) {
        const int32_t* d = table_host + (size_t)g * COLS;
        SIDE_REQUIRE(d[CFSH_NQ] >= 0, "%s: group %d has NQ=%d queries, a count cannot be negative", who, g, d[CFSH_NQ]);
        SIDE_REQUIRE(d[CFSH_Q0] == q, "%s: group %d has Q0=%d, the queries of the groups before it add up to %lld", who, g, d[CFSH_Q0], q);
        q += d[CFSH_NQ];
        SIDE_REQUIRE(q <= MAX_32, "%s: the counts up to group %d (%lld queries) exceed 32-bit sizes", who, g, q);
    }
    SIDE_REQUIRE(q == NQ, "%s: the groups add up to %lld queries, not to NQ = %d", who, q, NQ);
    hipLaunchKernelGGL(select_kernel, dim3((unsigned)G), dim3(WG), 0, static_cast<hipStream_t>(stream), S, cols, table_dev,
                       reinterpret_cast<unsigned*>(work), NQ, NC, keep < NC ? keep : NC, sel_cols, sel_slots);
    return check_launch(who);
}
