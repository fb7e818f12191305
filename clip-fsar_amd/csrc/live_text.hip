// Grouped text scoring (libclipfsar_live_text.so, C ABI in include/clipfsar_live_text.h): the EVAL_TEXT / COMBINE eval branches of a
// ragged list of (queries x classes) rectangles -- each group of queries against its own list of slots of a text-row store -- in one
// launch each.  Both branches end in a softmax over the classes, so a subset of the stored classes is no column slice of the dense
// kernels' output (gallery_text.hip): the softmax runs over the list.  The pieces are the tree's: the K loop is fp32_tile_gemm_rows with a
// looked-up B row (fp32_tile_gemm.h), the slot arithmetic is store_slot_row / store_slot_norm at one row per class (otam_tile.h), the
// epilogue, the partials' merge and the two row bodies are gallery_text.hip's own (text_softmax.h), and the tile scheduler in front is
// groups.hip's: a 1-D grid, one workgroup per tile, which finds its group by a search over a prefix column of the descriptor table.  The
// tile number is workgroup-uniform, so the search runs on scalar values.  A library of its own: the other ten keep their pinned export
// sets and kernel counts.
#include "otam_tile.h"
#include "text_softmax.h"
#include "../../include/clipfsar_live_text.h"

namespace {

constexpr int COLS = CFLT_TABLE_COLS;

// the last table row whose prefix offset in column `col` is <= r (find_group of groups.hip over this table's rows: offsets start at 0 and
// never decrease; a group without queries shares its offsets with the row after it and is passed over, a trailing one has the totals and
// is never reached).  Everything is uniform.
__device__ __forceinline__ const int32_t* find_group(const int32_t* __restrict__ table, unsigned G, int col, unsigned r) {
    unsigned lo = 0, hi = G;                   // table[lo][col] <= r; hi == G or table[hi][col] > r
    while (hi - lo > 1) {
        const unsigned mid = (lo + hi) >> 1;
        if ((unsigned)table[mid * COLS + col] <= r) lo = mid;
        else hi = mid;
    }
    return table + lo * COLS;
}

// ---- the B rows of a group's class tile: the text_store row its list names for tile row r, one row per class (store_slot_row at T = 1)
struct TextSlots {
    const int32_t* __restrict__ cols;          // cols + C0 of the group
    int cap, c0, b_rows;
    __device__ __forceinline__ LookedUpRow operator()(int r) const { return LookedUpRow{store_slot_row(cols, cap, r, c0, b_rows, 1)}; }
};

// ---- one workgroup per tile of 64 queries x 64 classes.  Tile `blockIdx.x` belongs to the group whose TILE0 is the last one <= it;
// inside the group the class tile is the fastest index, as blockIdx.x is in text_logits_kernel's 2-D grid.  The body then is that
// kernel's with the group as its whole problem.
__global__ __launch_bounds__(256) void text_logits_grouped_kernel(const float* __restrict__ emb, const float* __restrict__ en,
                                                                  const float* __restrict__ text, const float* __restrict__ tn,
                                                                  const int32_t* __restrict__ cols, const float* __restrict__ scale,
                                                                  float* __restrict__ logits, float* __restrict__ partials,
                                                                  const int32_t* __restrict__ table, unsigned G, int cap, int E) {
    __shared__ __attribute__((aligned(16))) float smem[2 * TILE * SLD];
    __shared__ float sen[TILE], stn[TILE];
    float* sA = smem;                                  // [TILE][SLD]
    float* sB = smem + TILE * SLD;                     // [TILE][SLD]
    float* img = smem;                                 // [TILE][ILD], after the K loop
    const unsigned tile = blockIdx.x;
    const int32_t* d = find_group(table, G, CFLT_TILE0, tile);
    const int nq = d[CFLT_NQ], nc = d[CFLT_NC];
    if (nc < 1) return;                                // as below
    const unsigned local = tile - (unsigned)d[CFLT_TILE0], ctiles = (unsigned)(nc + TILE - 1) / TILE;
    const unsigned qt = local / ctiles, ct = local - qt * ctiles;
    if (qt * TILE >= (unsigned)nq) return;             // not a tile of this group: a device table that is not the validated host rows
    const int q0 = (int)(qt * TILE), c0 = (int)(ct * TILE);
    const size_t q_first = (size_t)d[CFLT_Q0] + q0;    // the tile's first query among all
    const int32_t* gcols = cols + d[CFLT_C0];
    const int tid = threadIdx.x;
    const int a_rows = min(TILE, nq - q0), b_rows = min(TILE, nc - c0);          // valid rows of each operand
    if (tid < TILE) sen[tid] = tid < a_rows ? en[q_first + tid] : 1.f;
    else if (tid < 2 * TILE) stn[tid - TILE] = store_slot_norm(tn, gcols, cap, tid - TILE, c0, b_rows, 1);   // NaN for a bad slot

    f32x4 acc[2][2];
    // ends with a barrier: the logit image overwrites the staging buffers
    fp32_tile_gemm_rows(emb, q_first, a_rows, text, TextSlots{gcols, cap, c0, b_rows}, E, sA, sB, acc);
    text_tile_epilogue(acc, img, sen, stn, scale[0], a_rows, b_rows, logits + (size_t)d[CFLT_OUT0] + (size_t)q0 * nc + c0, (size_t)nc,
                       partials + ((size_t)d[CFLT_PART0] + (size_t)q0 * ctiles + ct) * 2, (size_t)ctiles * 2);
}

// ---- the two row kernels: one workgroup per query row, whose group is the last one with Q0 <= the query (out may alias logits)
struct GroupRow {
    size_t out, part;                          // the row's first logit, its first partial (in floats)
    int nc, ntiles;                            // nc = 0: no row of the table
};
__device__ __forceinline__ GroupRow group_row(const int32_t* __restrict__ table, unsigned G, unsigned q) {
    const int32_t* d = find_group(table, G, CFLT_Q0, q);
    const unsigned i = q - (unsigned)d[CFLT_Q0];
    const int nc = d[CFLT_NC], ntiles = (nc + TILE - 1) / TILE;
    if (i >= (unsigned)d[CFLT_NQ] || nc < 1) return GroupRow{0, 0, 0, 0};        // as above
    return GroupRow{(size_t)d[CFLT_OUT0] + (size_t)i * nc, ((size_t)d[CFLT_PART0] + (size_t)i * ntiles) * 2, nc, ntiles};
}

__global__ __launch_bounds__(256) void text_softmax_grouped_kernel(const float* logits, const float* __restrict__ partials, float* probs,
                                                                   const int32_t* __restrict__ table, unsigned G) {
    __shared__ float red[4];
    const GroupRow r = group_row(table, G, blockIdx.x);
    if (r.nc == 0) return;
    text_softmax_row(logits + r.out, partials + r.part, probs + r.out, r.nc, r.ntiles, red);
}

__global__ __launch_bounds__(256) void text_combine_grouped_kernel(const float* logits, const float* __restrict__ partials,
                                                                   const float* __restrict__ visual, float* out,
                                                                   const int32_t* __restrict__ table, unsigned G, float coff) {
    __shared__ float red[4];
    const GroupRow r = group_row(table, G, blockIdx.x);
    if (r.nc == 0) return;
    text_combine_row(logits + r.out, partials + r.part, visual + r.out, out + r.out, r.nc, r.ntiles, coff, red);
}

// The host rows, before any device work: counts, every prefix column equal to the running sum of its counts, the pad 0; the sums end at
// the totals the caller states (NCOLS < 0: that total is not checked -- the row kernels do not see cols).  -> *tiles: the grid size
int check_groups(const char* who, const int32_t* t, int G, int NQ, long long NCOLS, int NOUT, int NPART, long long* tiles) {
    SIDE_REQUIRE(G >= 1 && G <= CFLT_MAX_GROUPS, "%s: a table of G=%d groups (1 .. %d)", who, G, CFLT_MAX_GROUPS);
    long long q = 0, c = 0, tl = 0, out = 0, part = 0;
    for (int g = 0; g < G; ++g) {
        const int32_t* d = t + (size_t)g * COLS;
        const long long nq = d[CFLT_NQ], nc = d[CFLT_NC];
        SIDE_REQUIRE(nq >= 0, "%s: group %d has NQ=%lld queries, a count cannot be negative", who, g, nq);
        SIDE_REQUIRE(nc >= 1, "%s: group %d has NC=%lld slots, at least 1 is needed", who, g, nc);
        SIDE_REQUIRE(d[CFLT_Q0] == q, "%s: group %d has Q0=%d, the queries of the groups before it add up to %lld", who, g, d[CFLT_Q0], q);
        SIDE_REQUIRE(d[CFLT_C0] == c, "%s: group %d has C0=%d, the lists of the groups before it add up to %lld slots", who, g,
                     d[CFLT_C0], c);
        SIDE_REQUIRE(d[CFLT_TILE0] == tl, "%s: group %d has TILE0=%d, the groups before it own %lld tiles of 64 x 64", who, g,
                     d[CFLT_TILE0], tl);
        SIDE_REQUIRE(d[CFLT_OUT0] == out, "%s: group %d has OUT0=%d, the blocks of the groups before it add up to %lld values", who, g,
                     d[CFLT_OUT0], out);
        SIDE_REQUIRE(d[CFLT_PART0] == part, "%s: group %d has PART0=%d, the groups before it own %lld softmax partials", who, g,
                     d[CFLT_PART0], part);
        SIDE_REQUIRE(d[CFLT_PAD] == 0, "%s: group %d has %d in its last column, which must be 0", who, g, d[CFLT_PAD]);
        const long long ctiles = (nc + TILE - 1) / TILE;
        q += nq;
        c += nc;
        out += nq * nc;
        tl += ((nq + TILE - 1) / TILE) * ctiles;
        part += nq * ctiles;
        SIDE_REQUIRE(q <= 0x7fffffffLL && c <= 0x7fffffffLL && out <= 0x7fffffffLL && tl <= 0x7fffffffLL && 2 * part <= 0x7fffffffLL,
                     "%s: the counts up to group %d (%lld queries, %lld slots, %lld values, %lld tiles, %lld partials) exceed 32-bit sizes",
                     who, g, q, c, out, tl, part);
    }
    SIDE_REQUIRE(q == NQ, "%s: the groups add up to %lld queries, not to NQ = %d", who, q, NQ);
    SIDE_REQUIRE(NCOLS < 0 || c == NCOLS, "%s: the lists add up to %lld slots, not to NCOLS = %lld", who, c, NCOLS);
    SIDE_REQUIRE(out == NOUT, "%s: the blocks add up to %lld values, not to NOUT = %d", who, out, NOUT);
    SIDE_REQUIRE(part == NPART, "%s: the groups own %lld softmax partials, not NPART = %d", who, part, NPART);
    *tiles = tl;
    return 0;
}

}  // namespace

extern "C" int cflt_version(void) { return 100; /* 0.1.0 */ }
extern "C" int cflt_abi_version(void) { return CFLT_ABI_VERSION; }
extern "C" const char* cflt_last_error(void) { return g_err; }

extern "C" int cflt_workspace_floats(const int32_t* table_host, int G) {
    if (!table_host || G < 1 || G > CFLT_MAX_GROUPS) return -1;
    long long part = 0;
    for (int g = 0; g < G; ++g) {
        const long long nq = table_host[(size_t)g * COLS + CFLT_NQ], nc = table_host[(size_t)g * COLS + CFLT_NC];
        if (nq < 0 || nc < 1) return -1;
        part += nq * ((nc + TILE - 1) / TILE);
        if (2 * part > 0x7fffffffLL) return -1;
    }
    return (int)(2 * part);
}

extern "C" int cflt_text_logits_grouped(const float* emb, const float* en, const float* text_store, const float* tn_store,
                                        const int32_t* cols, const float* scale, float* logits, float* partials, const int32_t* table_host,
                                        const int32_t* table_dev, int G, int NQ, int NCOLS, int NOUT, int NPART, int cap, int E,
                                        cflt_stream_t stream) {
    const char* who = "cflt_text_logits_grouped";
    SIDE_REQUIRE(emb && en && text_store && tn_store && cols && scale && logits && partials && table_host && table_dev,
                 "%s: null pointer", who);
    SIDE_REQUIRE(NQ >= 1 && NCOLS >= 1 && NOUT >= 1 && NPART >= 1 && cap >= 1 && E >= 4 && E <= 8192 && E % 4 == 0,
                 "%s: bad shape (NQ=%d NCOLS=%d NOUT=%d NPART=%d cap=%d E=%d; NQ, NCOLS, NOUT, NPART, cap >= 1, E %% 4 == 0, "
                 "4 <= E <= 8192)", who, NQ, NCOLS, NOUT, NPART, cap, E);
    SIDE_REQUIRE(((uintptr_t)emb & 15u) == 0 && ((uintptr_t)text_store & 15u) == 0, "%s: emb and text_store must be 16-byte aligned", who);
    long long tiles;
    if (check_groups(who, table_host, G, NQ, NCOLS, NOUT, NPART, &tiles)) return 1;
    // one workgroup per tile (>= 1: NQ >= 1, and every group has a slot)
    hipLaunchKernelGGL(text_logits_grouped_kernel, dim3((unsigned)tiles), dim3(256), 0, static_cast<hipStream_t>(stream), emb, en,
                       text_store, tn_store, cols, scale, logits, partials, table_dev, (unsigned)G, cap, E);
    return check_launch(who);
}

extern "C" int cflt_text_softmax_grouped(const float* logits, const float* partials, float* probs, const int32_t* table_host,
                                         const int32_t* table_dev, int G, int NQ, int NOUT, int NPART, cflt_stream_t stream) {
    const char* who = "cflt_text_softmax_grouped";
    SIDE_REQUIRE(logits && partials && probs && table_host && table_dev, "%s: null pointer", who);
    SIDE_REQUIRE(NQ >= 1 && NOUT >= 1 && NPART >= 1, "%s: bad shape (NQ=%d NOUT=%d NPART=%d; all >= 1)", who, NQ, NOUT, NPART);
    long long tiles;
    if (check_groups(who, table_host, G, NQ, -1, NOUT, NPART, &tiles)) return 1;
    hipLaunchKernelGGL(text_softmax_grouped_kernel, dim3((unsigned)NQ), dim3(256), 0, static_cast<hipStream_t>(stream), logits, partials,
                       probs, table_dev, (unsigned)G);
    return check_launch(who);
}

extern "C" int cflt_text_combine_grouped(const float* logits, const float* partials, const float* visual, float* out,
                                         const int32_t* table_host, const int32_t* table_dev, int G, int NQ, int NOUT, int NPART,
                                         float coff, cflt_stream_t stream) {
    const char* who = "cflt_text_combine_grouped";
    SIDE_REQUIRE(logits && partials && visual && out && table_host && table_dev, "%s: null pointer", who);
    SIDE_REQUIRE(NQ >= 1 && NOUT >= 1 && NPART >= 1, "%s: bad shape (NQ=%d NOUT=%d NPART=%d; all >= 1)", who, NQ, NOUT, NPART);
    SIDE_REQUIRE(__builtin_isfinite(coff), "%s: coff must be finite", who);
    long long tiles;
    if (check_groups(who, table_host, G, NQ, -1, NOUT, NPART, &tiles)) return 1;
    hipLaunchKernelGGL(text_combine_grouped_kernel, dim3((unsigned)NQ), dim3(256), 0, static_cast<hipStream_t>(stream), logits, partials,
                       visual, out, table_dev, (unsigned)G, coff);
    return check_launch(who);
}
