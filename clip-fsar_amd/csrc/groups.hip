// Grouped scoring (libclipfsar_groups.so, C ABI in include/clipfsar_groups.h): cos_sim + OTAM and top-k of a ragged list of
// (queries x classes) rectangles -- each group of queries against its own list of store slots -- in one launch each.  The tile body is
// otam_tile_at (otam_tile.h), the one of otam_gallery_kernel (gallery.hip) and otam_indexed_kernel (live.hip); what is new here is the
// tile scheduler in front of it: a 1-D grid with one workgroup per tile, which finds its group in the descriptor table by a search over
// the TILE0 column.  The tile number is workgroup-uniform, so the search runs on scalar values (the table loads are scalar loads), as
// find_row of pool.hip.  A library of its own: the other seven keep their pinned export sets and kernel counts.
#include "otam_tile.h"
#include "topk_wave.h"
#include "../../include/clipfsar_groups.h"

namespace {

constexpr int COLS = CFGR_TABLE_COLS;

// the last table row whose prefix offset in column `col` is <= r (offsets start at 0 and never decrease; a group without queries shares
// its offsets with the row after it and is passed over, a trailing one has the totals and is never reached).  Everything is uniform.
__device__ __forceinline__ const int32_t* find_group(const int32_t* __restrict__ table, unsigned G, int col, unsigned r) {
    unsigned lo = 0, hi = G;                   // table[lo][col] <= r; hi == G or table[hi][col] > r
    while (hi - lo > 1) {
        const unsigned mid = (lo + hi) >> 1;
        if ((unsigned)table[mid * COLS + col] <= r) lo = mid;
        else hi = mid;
    }
    return table + lo * COLS;
}

// ---- the B-row source of a group: StoreSlots of live.hip over the group's part of cols
struct GroupSlots {
    const float* __restrict__ pn;
    const int32_t* __restrict__ cols;          // cols + C0 of the group
    int cap;
    static constexpr bool POISONS = true;              // a bad slot: NaN norms poison its column
    __device__ __forceinline__ LookedUpRow row(int r, int c0, int b_rows, int T) const {
        return LookedUpRow{store_slot_row(cols, cap, r, c0, b_rows, T)};
    }
    __device__ __forceinline__ float norm(int r, int c0, int b_rows, int T) const {
        return store_slot_norm(pn, cols, cap, r, c0, b_rows, T);
    }
    __device__ __forceinline__ float* dists() const { return nullptr; }
};

// ---- one workgroup per tile.  Tile `blockIdx.x` belongs to the group whose TILE0 is the last one <= it; inside the group the class tile
// is the fastest index, as blockIdx.x is in the dense kernel's 2-D grid.  The body then sees the group as its whole problem: base
// pointers moved to the group's first query, list and logits block, NQ and C the group's.
template <int TT>
__global__ __launch_bounds__(256) void otam_grouped_kernel(const float* __restrict__ Xq, const float* __restrict__ qn,
                                                           const float* __restrict__ P, const float* __restrict__ pn,
                                                           const int32_t* __restrict__ cols, float* __restrict__ logits,
                                                           const int32_t* __restrict__ table, unsigned G, int cap, int Trt, int E,
                                                           float lbda, int single_direct) {
    const int T = TT > 0 ? TT : Trt, QB = tile_videos(T);
    const unsigned tile = blockIdx.x;
    const int32_t* d = find_group(table, G, CFGR_TILE0, tile);
    const int nq = d[CFGR_NQ], nc = d[CFGR_NC], q_first = d[CFGR_Q0];
    const unsigned local = tile - (unsigned)d[CFGR_TILE0], ctiles = (unsigned)(nc + QB - 1) / QB;
    const unsigned qt = local / ctiles, ct = local - qt * ctiles;
    if (qt * QB >= (unsigned)nq) return;               // not a tile of this group: a device table that is not the validated host rows
    otam_tile_at<TT>((int)(qt * QB), (int)(ct * QB), Xq + (size_t)q_first * T * E, qn + (size_t)q_first * T, P,
                     GroupSlots{pn, cols + d[CFGR_C0], cap}, logits + d[CFGR_OUT0], nq, nc, Trt, E, lbda, single_direct);
}

// ---- top-k: one wave per query row, whose group is the last one with Q0 <= the query
__global__ __launch_bounds__(64) void topk_grouped_kernel(const float* __restrict__ logits, const int32_t* __restrict__ table, unsigned G,
                                                          float* __restrict__ values, int32_t* __restrict__ index, int k) {
    const unsigned q = blockIdx.x;
    const int32_t* d = find_group(table, G, CFGR_Q0, q);
    const int nc = d[CFGR_NC];
    const unsigned i = q - (unsigned)d[CFGR_Q0];
    if (i >= (unsigned)d[CFGR_NQ]) return;             // as above
    topk_wave(logits + d[CFGR_OUT0] + (size_t)i * nc, nc, k, values + (size_t)q * k, index + (size_t)q * k, threadIdx.x);
}

// The host rows, before any device work: counts, and every prefix column equal to the running sum of its counts; the sums end at the
// totals the caller states.  qb = 0: TILE0 is not checked (the top-k call does not know T); NCOLS < 0: that total is not checked.
// -> *tiles: the grid size, *min_nc: the smallest NC of a group with queries
int check_groups(const char* who, const int32_t* t, int G, int NQ, long long NCOLS, int NOUT, int qb, long long* tiles, int* min_nc) {
    SIDE_REQUIRE(G >= 1 && G <= CFGR_MAX_GROUPS, "%s: a table of G=%d groups (1 .. %d)", who, G, CFGR_MAX_GROUPS);
    long long q = 0, c = 0, tl = 0, out = 0;
    *min_nc = 0x7fffffff;
    for (int g = 0; g < G; ++g) {
        const int32_t* d = t + (size_t)g * COLS;
        const long long nq = d[CFGR_NQ], nc = d[CFGR_NC];
        SIDE_REQUIRE(nq >= 0, "%s: group %d has NQ=%lld queries, a count cannot be negative", who, g, nq);
        SIDE_REQUIRE(nc >= 1, "%s: group %d has NC=%lld slots, at least 1 is needed", who, g, nc);
        SIDE_REQUIRE(d[CFGR_Q0] == q && d[CFGR_C0] == c && d[CFGR_OUT0] == out && (qb == 0 || d[CFGR_TILE0] == tl),
                     "%s: group %d has offsets (Q0=%d C0=%d TILE0=%d OUT0=%d), the prefix sums of the counts before it are (%lld, %lld, "
                     "%lld, %lld)", who, g, d[CFGR_Q0], d[CFGR_C0], d[CFGR_TILE0], d[CFGR_OUT0], q, c, tl, out);
        q += nq;
        c += nc;
        out += nq * nc;
        if (qb) tl += ((nq + qb - 1) / qb) * ((nc + qb - 1) / qb);
        if (nq && nc < *min_nc) *min_nc = (int)nc;
        SIDE_REQUIRE(q <= 0x7fffffffLL && c <= 0x7fffffffLL && out <= 0x7fffffffLL && tl <= 0x7fffffffLL,
                     "%s: the counts up to group %d (%lld queries, %lld slots, %lld logits, %lld tiles) exceed 32-bit sizes", who, g, q, c,
                     out, tl);
    }
    SIDE_REQUIRE(q == NQ, "%s: the groups add up to %lld queries, not to NQ = %d", who, q, NQ);
    SIDE_REQUIRE(NCOLS < 0 || c == NCOLS, "%s: the lists add up to %lld slots, not to NCOLS = %lld", who, c, NCOLS);
    SIDE_REQUIRE(out == NOUT, "%s: the blocks add up to %lld logits, not to NOUT = %d", who, out, NOUT);
    *tiles = tl;
    return 0;
}

}  // namespace

extern "C" int cfgr_version(void) { return 100; /* 0.1.0 */ }
extern "C" int cfgr_abi_version(void) { return CFGR_ABI_VERSION; }
extern "C" const char* cfgr_last_error(void) { return g_err; }

extern "C" int cfgr_otam_grouped(const float* Xq, const float* qn, const float* P_store, const float* pn_store, const int32_t* cols,
                                 float* logits, const int32_t* table_host, const int32_t* table_dev, int G, int NQ, int NCOLS, int NOUT,
                                 int cap, int T, int E, float lambda, int single_direct, cfgr_stream_t stream) {
    const char* who = "cfgr_otam_grouped";
    SIDE_REQUIRE(Xq && qn && P_store && pn_store && cols && logits && table_host && table_dev, "%s: null pointer", who);
    SIDE_REQUIRE(otam_shape_ok(NQ, NCOLS, T, E) && NOUT >= 1 && cap >= 1,
                 "%s: bad shape (NQ=%d NCOLS=%d NOUT=%d cap=%d T=%d E=%d; NQ, NCOLS, NOUT, cap >= 1, 1 <= T <= 32, E %% 4 == 0, "
                 "4 <= E <= 8192)", who, NQ, NCOLS, NOUT, cap, T, E);
    SIDE_REQUIRE((long long)cap * T <= 0x7fffffffLL && (long long)NQ * T <= 0x7fffffffLL,
                 "%s: cap * T = %lld or NQ * T = %lld rows exceed 32-bit sizes", who, (long long)cap * T, (long long)NQ * T);
    SIDE_REQUIRE(((uintptr_t)Xq & 15u) == 0 && ((uintptr_t)P_store & 15u) == 0, "%s: Xq and P_store must be 16-byte aligned", who);
    SIDE_REQUIRE(lambda > 0.f, "%s: lambda must be > 0", who);
    long long tiles;
    int min_nc;
    if (check_groups(who, table_host, G, NQ, NCOLS, NOUT, tile_videos(T), &tiles, &min_nc)) return 1;
    // one workgroup per tile (>= 1: NQ >= 1, and every group has a slot)
    return otam_tile_forms(who, T, dim3((unsigned)tiles), [&](auto tt, dim3 grid, int lds) {
        hipLaunchKernelGGL(otam_grouped_kernel<decltype(tt)::value>, grid, dim3(256), lds, static_cast<hipStream_t>(stream), Xq, qn,
                           P_store, pn_store, cols, logits, table_dev, (unsigned)G, cap, T, E, lambda, single_direct);
    });
}

extern "C" int cfgr_topk_grouped(const float* logits, const int32_t* table_host, const int32_t* table_dev, int G, int NQ, int NOUT, int k,
                                 float* values, int32_t* index, cfgr_stream_t stream) {
    const char* who = "cfgr_topk_grouped";
    SIDE_REQUIRE(logits && table_host && table_dev && values && index, "%s: null pointer", who);
    SIDE_REQUIRE(NQ >= 1 && NOUT >= 1, "%s: bad shape (NQ=%d NOUT=%d; both >= 1)", who, NQ, NOUT);
    long long tiles;
    int min_nc;
    if (check_groups(who, table_host, G, NQ, -1, NOUT, 0, &tiles, &min_nc)) return 1;
    SIDE_REQUIRE(k >= 1 && k <= TOPK_MAX && k <= min_nc, "%s: k=%d outside 1 .. min(%d, %d = the smallest NC of a group with queries)", who,
                 k, TOPK_MAX, min_nc);
    for (int g = 0; g < G; ++g) {
        const int32_t* d = table_host + (size_t)g * COLS;
        SIDE_REQUIRE(d[CFGR_NQ] == 0 || d[CFGR_NC] <= 65535, "%s: group %d has NC=%d slots, at most 65535 are ranked", who, g, d[CFGR_NC]);
    }
    hipLaunchKernelGGL(topk_grouped_kernel, dim3((unsigned)NQ), dim3(64), 0, static_cast<hipStream_t>(stream), logits, table_dev,
                       (unsigned)G, values, index, k);
    return check_launch(who);
}
