// The timeline of a stream pool (libclipfsar_timeline.so, C ABI in include/ext/clipfsar_timeline.h): every push's class scores folded
// into coarse buckets of windows -- per (session slot, bucket, class store slot) the peak score, the window of the peak and a count of
// windows at or above a level -- in the push that made the scores, and read back bucket by bucket.  State is keyed as baseline.hip keys
// its own, with the bucket ring as a middle dimension, and a cell is live for a bucket iff its mark is the store slot's current
// generation and its peak's window lies in that bucket.  The fold's descriptor table, key lists and thread mapping are baseline.hip's:
// one workgroup per (table row, chunk of CFTL_CHUNK columns), found in the CHUNK0 column, one thread per column, adjacent threads on
// adjacent columns, sequential in the window with the current cell in registers, so the score reads are coalesced at every window and
// a cell is read and written once per bucket it crosses.  The read has the same mapping over a table of its own, sequential in the
// bucket.  Plain C++ for wave64: a thread alone touches its cells, nothing waits on another workgroup, two runs give identical bytes.
// A plug-in library (build.py, PLUGIN_LIBS): it lives beside csrc/ and includes the shared error plumbing and its own header alone --
// the row search is its own copy, the includers of ext/chunk_row.h stay the ones they were.
#include "../csrc/side_lib.h"
#include "../../include/ext/clipfsar_timeline.h"

#include <math.h>

namespace {

constexpr int CHUNK = CFTL_CHUNK;
constexpr int COLS = CFTL_TABLE_COLS;
constexpr int RCOLS = CFTL_READ_COLS;
constexpr long long MAX_ITEMS = 0x7fffffffLL;  // cells, scores and window numbers are indexed with 32 bits

// the table row whose CHUNK0 is the last one <= g (every row has NC >= 1, so CHUNK0 rises strictly) -> its number.  `cols` values per
// row, CHUNK0 at `chunk0`.  The workgroup number g is uniform, so the search runs on scalar values.
__device__ __forceinline__ unsigned find_row(const int32_t* __restrict__ table, unsigned S, unsigned g, unsigned cols, unsigned chunk0) {
    unsigned lo = 0, hi = S;                   // table[lo][CHUNK0] <= g; hi == S or table[hi][CHUNK0] > g
    for (; hi - lo > 1;) {
        const unsigned mid = (lo + hi) >> 1;
        if ((unsigned)table[mid * cols + chunk0] <= g) lo = mid;
        else hi = mid;
    }
    return lo;
}

// whether a cell whose peak lies at window a belongs to bucket b: a >= 0 and a / span == b, without the division
__device__ __forceinline__ bool in_bucket(int32_t a, unsigned b, unsigned span) {
    const unsigned long long lo = (unsigned long long)b * span;
    return a >= 0 && (unsigned long long)a >= lo && (unsigned long long)a < lo + span;
}

__global__ __launch_bounds__(CHUNK) void timeline_fold_kernel(const float* __restrict__ scores, float* __restrict__ peak,
                                                              int32_t* __restrict__ at, int32_t* __restrict__ above,
                                                              int32_t* __restrict__ marks, const int32_t* __restrict__ gens,
                                                              const int32_t* __restrict__ keys, const int32_t* __restrict__ table,
                                                              const int32_t* __restrict__ first, unsigned S, unsigned B, unsigned cap,
                                                              unsigned span, int has_level, float level) {
    const unsigned row = find_row(table, S, blockIdx.x, COLS, CFTL_CHUNK0);
    const int32_t* t = table + row * COLS;
    const unsigned nW = (unsigned)t[CFTL_NW], NC = (unsigned)t[CFTL_NC];
    const unsigned j = (blockIdx.x - (unsigned)t[CFTL_CHUNK0]) * CHUNK + threadIdx.x;
    if (nW == 0 || j >= NC) return;                                            // no windows: nothing is touched
    const unsigned key = (unsigned)keys[(size_t)t[CFTL_KEY0] + j];
    if (key >= cap) return;                                                    // never dereferenced, no state write
    const int32_t gen = gens[key];
    const size_t base = (size_t)t[CFTL_SLOT] * B * cap + key;                  // the cell of ring position p: base + p * cap
    size_t src = (size_t)t[CFTL_OUT0] + j;
    unsigned w = (unsigned)first[row];
    unsigned b = w / span;
    unsigned left = span - (w - b * span);                                     // windows of bucket b from w on
    unsigned pos = b % B;
    for (unsigned k = 0; k < nW;) {
        const size_t cell = base + (size_t)pos * cap;
        float p = -INFINITY;
        int32_t a = -1, n = 0;
        if (marks[cell] == gen) {
            const int32_t was = at[cell];
            if (in_bucket(was, b, span)) {                                     // this lap's cell: the fold goes on
                p = peak[cell];
                a = was;
                n = above[cell];
            }
        }
        const unsigned stop = k + min(left, nW - k);
        for (; k < stop; ++k, ++w, src += NC) {
            const float s = scores[src];
            if (s == s && s != -INFINITY) {                                    // a candidate: neither NaN nor -inf
                if (a < 0 || s > p) {                                          // strictly: a tie keeps the earlier window
                    p = s;
                    a = (int32_t)w;
                }
                if (!has_level || s >= level) n += 1;
            }
        }
        if (a >= 0) {                                                          // a cell that saw no candidate is not touched
            peak[cell] = p;
            at[cell] = a;
            above[cell] = n;
            marks[cell] = gen;
        }
        b += 1;
        pos = pos + 1 == B ? 0 : pos + 1;
        left = span;
    }
}

__global__ __launch_bounds__(CHUNK) void timeline_read_kernel(const float* __restrict__ peak, const int32_t* __restrict__ at,
                                                              const int32_t* __restrict__ above, const int32_t* __restrict__ marks,
                                                              const int32_t* __restrict__ gens, const int32_t* __restrict__ keys,
                                                              float* __restrict__ out_peak, int32_t* __restrict__ out_at,
                                                              int32_t* __restrict__ out_above, const int32_t* __restrict__ table,
                                                              unsigned S, unsigned B, unsigned cap, unsigned span) {
    const int32_t* t = table + find_row(table, S, blockIdx.x, RCOLS, CFTL_R_CHUNK0) * RCOLS;
    const unsigned NB = (unsigned)t[CFTL_R_NB], NC = (unsigned)t[CFTL_R_NC];
    const unsigned j = (blockIdx.x - (unsigned)t[CFTL_R_CHUNK0]) * CHUNK + threadIdx.x;
    if (NB == 0 || j >= NC) return;
    const unsigned key = (unsigned)keys[(size_t)t[CFTL_R_KEY0] + j];
    size_t dst = (size_t)t[CFTL_R_OUT0] + j;
    if (key >= cap) {                                                          // never dereferenced: a NaN column
        for (unsigned i = 0; i < NB; ++i, dst += NC) {
            out_peak[dst] = __builtin_nanf("");
            out_at[dst] = -1;
            out_above[dst] = 0;
        }
        return;
    }
    const int32_t gen = gens[key];
    const size_t base = (size_t)t[CFTL_R_SLOT] * B * cap + key;
    unsigned b = (unsigned)t[CFTL_R_B0];
    unsigned pos = b % B;
    for (unsigned i = 0; i < NB; ++i, dst += NC) {
        const size_t cell = base + (size_t)pos * cap;
        float p = -INFINITY;
        int32_t a = -1, n = 0;
        if (marks[cell] == gen) {
            const int32_t was = at[cell];
            if (in_bucket(was, b, span)) {
                p = peak[cell];
                a = was;
                n = above[cell];
            }
        }
        out_peak[dst] = p;
        out_at[dst] = a;
        out_above[dst] = n;
        b += 1;
        pos = pos + 1 == B ? 0 : pos + 1;
    }
}

// what both entry points ask of the state's shape
int check_state(const char* what, int max_streams, int B, int cap, int span, int NOUT, int NKEYS) {
    SIDE_REQUIRE(max_streams >= 1 && max_streams <= CFTL_MAX_STREAMS, "%s: max_streams=%d outside 1 .. %d", what, max_streams,
                 CFTL_MAX_STREAMS);
    SIDE_REQUIRE(cap >= 1, "%s: cap=%d must be at least 1", what, cap);
    SIDE_REQUIRE(B >= 1 && B <= CFTL_MAX_BUCKETS, "%s: B=%d buckets outside 1 .. %d", what, B, CFTL_MAX_BUCKETS);
    SIDE_REQUIRE(span >= 1 && span <= CFTL_MAX_SPAN, "%s: span=%d outside 1 .. %d", what, span, CFTL_MAX_SPAN);
    SIDE_REQUIRE((long long)max_streams * B * cap <= MAX_ITEMS, "%s: too large for one launch (max_streams=%d x B=%d x cap=%d cells)",
                 what, max_streams, B, cap);
    SIDE_REQUIRE(NOUT >= 0 && NKEYS >= 1, "%s: bad shape (NOUT=%d NKEYS=%d)", what, NOUT, NKEYS);
    return 0;
}

}  // namespace

extern "C" int cftl_version(void) { return 100; /* 0.1.0 */ }
extern "C" int cftl_abi_version(void) { return CFTL_ABI_VERSION; }
extern "C" const char* cftl_last_error(void) { return g_err; }

extern "C" int cftl_fold(const float* scores, float* peak, int32_t* at, int32_t* above, int32_t* marks, const int32_t* gens,
                         const int32_t* keys, const int32_t* table_host, const int32_t* table_dev, const int32_t* first_host,
                         const int32_t* first_dev, int S, int NOUT, int NKEYS, int max_streams, int B, int cap, int span, int has_level,
                         float level, cftl_stream_t stream) {
    const char* what = "cftl_fold";
    SIDE_REQUIRE(scores && peak && at && above && marks && gens && keys && table_host && table_dev && first_host && first_dev,
                 "%s: null pointer", what);
    SIDE_REQUIRE(!has_level || isfinite(level), "%s: level=%g must be finite", what, (double)level);
    if (check_state(what, max_streams, B, cap, span, NOUT, NKEYS)) return 1;
    SIDE_REQUIRE(S >= 1 && S <= max_streams, "%s: a table of S=%d rows for max_streams=%d", what, S, max_streams);
    SlotBits seen(max_streams);
    SIDE_REQUIRE(seen.ok(), "%s: out of host memory for %d slots", what, max_streams);
    long long n_out = 0, chunks = 0;
    for (int s = 0; s < S; ++s) {
        const int32_t* d = table_host + (size_t)s * COLS;
        const int slot = d[CFTL_SLOT], nW = d[CFTL_NW], NC = d[CFTL_NC], key0 = d[CFTL_KEY0], w0 = first_host[s];
        SIDE_REQUIRE(slot >= 0 && slot < max_streams, "%s: row %d has slot %d outside 0 .. %d", what, s, slot, max_streams - 1);
        SIDE_REQUIRE(!seen.test_and_set(slot), "%s: slot %d appears twice in the table (row %d)", what, slot, s);
        SIDE_REQUIRE(nW >= 0, "%s: row %d has a negative count (nW=%d)", what, s, nW);
        SIDE_REQUIRE(NC >= 1, "%s: row %d has width NC=%d, at least 1 is needed", what, s, NC);
        SIDE_REQUIRE(d[CFTL_OUT0] == n_out && d[CFTL_CHUNK0] == chunks,
                     "%s: row %d has offsets (OUT0=%d, CHUNK0=%d), the prefix sums are (%lld, %lld)", what, s, d[CFTL_OUT0],
                     d[CFTL_CHUNK0], n_out, chunks);
        SIDE_REQUIRE(key0 >= 0 && (long long)key0 + NC <= NKEYS, "%s: row %d has its list at keys[%d .. %lld), outside 0 .. NKEYS=%d", what,
                     s, key0, (long long)key0 + NC, NKEYS);
        SIDE_REQUIRE(w0 >= 0, "%s: row %d has a negative first window (first=%d)", what, s, w0);
        SIDE_REQUIRE((long long)w0 + nW <= MAX_ITEMS, "%s: row %d has its windows at %d .. %lld, window numbers stay below 2^31", what, s, w0,
                     (long long)w0 + nW);
        n_out += (long long)nW * NC;
        chunks += ((long long)NC + CHUNK - 1) / CHUNK;
        SIDE_REQUIRE(n_out <= MAX_ITEMS && chunks <= MAX_ITEMS, "%s: the table's counts are too large for one launch (row %d)", what, s);
    }
    SIDE_REQUIRE(n_out == NOUT, "%s: the table's nW * NC sum to %lld, not to NOUT=%d", what, n_out, NOUT);
    if (NOUT == 0) return 0;                                                   // no session completed a window: nothing to do
    hipLaunchKernelGGL(timeline_fold_kernel, dim3((unsigned)chunks), dim3(CHUNK), 0, static_cast<hipStream_t>(stream), scores, peak, at,
                       above, marks, gens, keys, table_dev, first_dev, (unsigned)S, (unsigned)B, (unsigned)cap, (unsigned)span, has_level,
                       level);
    return check_launch(what);
}

extern "C" int cftl_read(const float* peak, const int32_t* at, const int32_t* above, const int32_t* marks, const int32_t* gens,
                         const int32_t* keys, float* out_peak, int32_t* out_at, int32_t* out_above, const int32_t* table_host,
                         const int32_t* table_dev, int S, int NOUT, int NKEYS, int max_streams, int B, int cap, int span,
                         cftl_stream_t stream) {
    const char* what = "cftl_read";
    SIDE_REQUIRE(peak && at && above && marks && gens && keys && out_peak && out_at && out_above && table_host && table_dev,
                 "%s: null pointer", what);
    if (check_state(what, max_streams, B, cap, span, NOUT, NKEYS)) return 1;
    SIDE_REQUIRE(S >= 1 && S <= CFTL_MAX_STREAMS, "%s: a table of S=%d rows (1 .. %d)", what, S, CFTL_MAX_STREAMS);
    long long n_out = 0, chunks = 0;
    for (int s = 0; s < S; ++s) {
        const int32_t* d = table_host + (size_t)s * RCOLS;
        const int slot = d[CFTL_R_SLOT], b0 = d[CFTL_R_B0], NB = d[CFTL_R_NB], NC = d[CFTL_R_NC], key0 = d[CFTL_R_KEY0];
        SIDE_REQUIRE(slot >= 0 && slot < max_streams, "%s: row %d has slot %d outside 0 .. %d", what, s, slot, max_streams - 1);
        SIDE_REQUIRE(b0 >= 0, "%s: row %d has a negative first bucket (B0=%d)", what, s, b0);
        SIDE_REQUIRE(NB >= 0 && NB <= B, "%s: row %d has NB=%d buckets outside 0 .. B=%d", what, s, NB, B);
        SIDE_REQUIRE(NB == 0 || ((long long)b0 + NB - 1) * span <= MAX_ITEMS,
                     "%s: row %d has its buckets at %d .. %lld, beyond the last one a window number below 2^31 reaches", what, s, b0,
                     (long long)b0 + NB);
        SIDE_REQUIRE(NC >= 1, "%s: row %d has width NC=%d, at least 1 is needed", what, s, NC);
        SIDE_REQUIRE(d[CFTL_R_OUT0] == n_out && d[CFTL_R_CHUNK0] == chunks,
                     "%s: row %d has offsets (OUT0=%d, CHUNK0=%d), the prefix sums are (%lld, %lld)", what, s, d[CFTL_R_OUT0],
                     d[CFTL_R_CHUNK0], n_out, chunks);
        SIDE_REQUIRE(key0 >= 0 && (long long)key0 + NC <= NKEYS, "%s: row %d has its list at keys[%d .. %lld), outside 0 .. NKEYS=%d", what,
                     s, key0, (long long)key0 + NC, NKEYS);
        n_out += (long long)NB * NC;
        chunks += ((long long)NC + CHUNK - 1) / CHUNK;
        SIDE_REQUIRE(n_out <= MAX_ITEMS && chunks <= MAX_ITEMS, "%s: the table's counts are too large for one launch (row %d)", what, s);
    }
    SIDE_REQUIRE(n_out == NOUT, "%s: the table's NB * NC sum to %lld, not to NOUT=%d", what, n_out, NOUT);
    if (NOUT == 0) return 0;                                                   // no bucket is asked for: nothing to do
    hipLaunchKernelGGL(timeline_read_kernel, dim3((unsigned)chunks), dim3(CHUNK), 0, static_cast<hipStream_t>(stream), peak, at, above,
                       marks, gens, keys, out_peak, out_at, out_above, table_dev, (unsigned)S, (unsigned)B, (unsigned)cap,
                       (unsigned)span);
    return check_launch(what);
}
