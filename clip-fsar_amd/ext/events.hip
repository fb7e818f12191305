// Stream events (libclipfsar_events.so, C ABI in include/ext/clipfsar_events.h): a hysteresis detector over every (session, class) pair's
// consecutive windows, run on the device in the push that scores them, emitting a compacted list of onset / offset records in the order
// (table row, column, window).  State is keyed as class_smooth.hip keys its own -- a cell per (session slot, class store slot), valid iff
// its mark is the store slot's current generation -- and the descriptor table, the key lists and the thread mapping are that library's:
// one workgroup per (table row, chunk of CFEV_CHUNK columns), one thread per column, adjacent threads on adjacent columns, sequential in
// the window k, so the score traffic is coalesced at every k.
// Three kernels, none of which waits on another workgroup; a record's position is a prefix sum, never a counter workgroups race for:
//   event_count_kernel  runs the machine without committing anything; work[b] = the workgroup's records, work[n_chunks + b * CHUNK + t] =
//                       the thread's
//   event_scan_kernel   ONE workgroup: work[0 .. n_chunks) becomes its exclusive prefix sums, n_events the total
//   event_emit_kernel   reruns the machine, places the thread's records at work[b] + (in-block exclusive scan of the threads' counts),
//                       drops those at max_events and beyond, commits state and marks
// An add-on library (build.py, ADDON_LIBS): it lives beside csrc/ and class_smooth.hip, whose files and export sets stay as they are.
#include "../csrc/ring_rows.h"
#include "../csrc/side_lib.h"
#include "../../include/ext/clipfsar_events.h"

#include <math.h>

namespace {

constexpr int CHUNK = CFEV_CHUNK;
constexpr int COLS = CFEV_TABLE_COLS;

struct Rule {
    float on, off;
    int32_t min_on, min_off;
};

// the table row whose CHUNK0 is the last one <= b (every row has NC >= 1, so CHUNK0 rises strictly).  Everything here is uniform.
__device__ __forceinline__ const int32_t* find_chunk_row(const int32_t* __restrict__ table, unsigned S, unsigned b, unsigned* row) {
    unsigned lo = 0, hi = S;                   // table[lo][CHUNK0] <= b; hi == S or table[hi][CHUNK0] > b
    while (hi - lo > 1) {
        const unsigned mid = (lo + hi) >> 1;
        if ((unsigned)table[mid * COLS + CFEV_CHUNK0] <= b) lo = mid;
        else hi = mid;
    }
    *row = lo;
    return table + lo * COLS;
}

// What a thread works on: its column of the row's block and its cell; `live` is false for a thread beyond the row's width, of a row
// without windows, or whose key lies outside [0, cap) -- such a thread reads no score, emits nothing and writes no state.
struct Column {
    bool live;
    unsigned row, j, nW, NC;
    size_t at, cell;
    int32_t gen;
};

__device__ __forceinline__ Column find_column(const int32_t* __restrict__ table, const int32_t* __restrict__ keys, const int32_t* __restrict__ gens,
                                              unsigned S, unsigned cap) {
    Column c;
    const int32_t* d = find_chunk_row(table, S, blockIdx.x, &c.row);
    c.nW = (unsigned)d[CFEV_NW];
    c.NC = (unsigned)d[CFEV_NC];
    c.j = (blockIdx.x - (unsigned)d[CFEV_CHUNK0]) * CHUNK + threadIdx.x;
    c.at = (size_t)d[CFEV_OUT0] + c.j;
    c.cell = 0;
    c.gen = 0;
    c.live = c.nW != 0 && c.j < c.NC;
    if (c.live) {
        const unsigned key = (unsigned)keys[(size_t)d[CFEV_KEY0] + c.j];
        c.live = key < cap;
        if (c.live) {
            c.cell = (size_t)d[CFEV_SLOT] * cap + key;
            c.gen = gens[key];
        }
    }
    return c;
}

// One pair's machine over its nW windows, NC floats apart.  put(k, kind, len, s, peak) receives every record in window order; the cell's
// three values are updated in place.  -> the number of records.
template <class Put>
__device__ __forceinline__ int32_t run_machine(const float* __restrict__ x, unsigned nW, unsigned NC, const Rule r, int32_t& streak, int32_t& length,
                                               float& peak, Put put) {
    int32_t n = 0;
    for (unsigned k = 0; k < nW; ++k) {
        const float s = x[(size_t)k * NC];
        if (streak >= 0) {                                                     // idle
            if (s >= r.on) {
                peak = streak == 0 ? s : fmaxf(peak, s);
                streak += 1;
                if (streak == r.min_on) {
                    put(k, CFEV_ONSET, r.min_on, s, peak);
                    ++n;
                    streak = -1;                                               // active, no window below off counted
                    length = r.min_on;
                }
            } else {
                streak = 0;                                                    // s < on, or NaN
            }
        } else {                                                               // active
            length += length != INT32_MAX;
            peak = fmaxf(peak, s);
            const int32_t below = s < r.off ? -streak : 0;                     // (-1 - streak) + 1, or back to 0 (NaN included)
            if (below == r.min_off) {
                put(k, CFEV_OFFSET, length - r.min_off, s, peak);
                ++n;
                streak = 0;
            } else {
                streak = -1 - below;
            }
        }
    }
    return n;
}

// the cell as the machine starts from it: what was stored when the mark is the slot's generation, idle otherwise
__device__ __forceinline__ void load_cell(const Column& c, const int32_t* __restrict__ streak, const int32_t* __restrict__ length,
                                          const float* __restrict__ peak, const int32_t* __restrict__ marks, int32_t& st, int32_t& len, float& pk) {
    st = 0, len = 0, pk = 0.f;
    if (c.live && marks[c.cell] == c.gen) {
        st = streak[c.cell];
        len = length[c.cell];
        pk = peak[c.cell];
    }
}

// exclusive prefix sum of v over the workgroup's CHUNK threads (Hillis-Steele in LDS); *total receives the sum.  Every thread of the
// workgroup calls it.  It ends on a barrier, so it may be called again at once.
__device__ __forceinline__ int32_t block_exclusive_scan(int32_t v, int32_t* total) {
    __shared__ int32_t buf[2][CHUNK];
    const unsigned t = threadIdx.x;
    unsigned p = 0;
    buf[0][t] = v;
    __syncthreads();
#pragma unroll
    for (unsigned d = 1; d < (unsigned)CHUNK; d <<= 1) {
        int32_t x = buf[p][t];
        if (t >= d) x += buf[p][t - d];
        buf[p ^ 1][t] = x;
        p ^= 1;
        __syncthreads();
    }
    const int32_t inclusive = buf[p][t];
    *total = buf[p][CHUNK - 1];
    __syncthreads();
    return inclusive - v;
}

__global__ __launch_bounds__(CHUNK) void event_count_kernel(const float* __restrict__ scores, const int32_t* __restrict__ streak,
                                                            const int32_t* __restrict__ length, const float* __restrict__ peak,
                                                            const int32_t* __restrict__ marks, const int32_t* __restrict__ gens,
                                                            const int32_t* __restrict__ keys, int32_t* __restrict__ work,
                                                            const int32_t* __restrict__ table, unsigned S, unsigned cap, Rule rule) {
    const Column c = find_column(table, keys, gens, S, cap);
    int32_t st, len, n = 0;
    float pk;
    load_cell(c, streak, length, peak, marks, st, len, pk);
    if (c.live) n = run_machine(scores + c.at, c.nW, c.NC, rule, st, len, pk, [](unsigned, int32_t, int32_t, float, float) {});
    work[(size_t)gridDim.x + (size_t)blockIdx.x * CHUNK + threadIdx.x] = n;
    int32_t total;
    block_exclusive_scan(n, &total);
    if (threadIdx.x == 0) work[blockIdx.x] = total;
}

// one workgroup: tiles of CHUNK workgroup totals, a running carry between them
__global__ __launch_bounds__(CHUNK) void event_scan_kernel(int32_t* __restrict__ work, int32_t* __restrict__ n_events, unsigned n_chunks) {
    int32_t carry = 0;
    for (unsigned b0 = 0; b0 < n_chunks; b0 += CHUNK) {
        const unsigned b = b0 + threadIdx.x;
        const int32_t v = b < n_chunks ? work[b] : 0;
        int32_t total;
        const int32_t before = block_exclusive_scan(v, &total);
        if (b < n_chunks) work[b] = carry + before;
        carry += total;
    }
    if (threadIdx.x == 0) *n_events = carry;
}

__global__ __launch_bounds__(CHUNK) void event_emit_kernel(const float* __restrict__ scores, int32_t* __restrict__ streak, int32_t* __restrict__ length,
                                                           float* __restrict__ peak, int32_t* __restrict__ marks, const int32_t* __restrict__ gens,
                                                           const int32_t* __restrict__ keys, int32_t* __restrict__ events, float* __restrict__ values,
                                                           const int32_t* __restrict__ work, const int32_t* __restrict__ table, unsigned S,
                                                           unsigned cap, Rule rule, unsigned max_events) {
    const Column c = find_column(table, keys, gens, S, cap);
    int32_t st, len;
    float pk;
    load_cell(c, streak, length, peak, marks, st, len, pk);
    const int32_t mine = work[(size_t)gridDim.x + (size_t)blockIdx.x * CHUNK + threadIdx.x];
    int32_t total;
    const int32_t before = block_exclusive_scan(mine, &total);
    if (!c.live) return;
    unsigned pos = (unsigned)work[blockIdx.x] + (unsigned)before;              // the thread's first record; its records are consecutive
    run_machine(scores + c.at, c.nW, c.NC, rule, st, len, pk, [&](unsigned k, int32_t kind, int32_t n, float s, float p) {
        if (pos < max_events) {
            int32_t* e = events + (size_t)pos * CFEV_EVENT_COLS;
            e[0] = (int32_t)c.row, e[1] = (int32_t)c.j, e[2] = (int32_t)k, e[3] = kind, e[4] = n;
            values[(size_t)pos * CFEV_VALUE_COLS] = s;
            values[(size_t)pos * CFEV_VALUE_COLS + 1] = p;
        }
        ++pos;
    });
    streak[c.cell] = st;
    length[c.cell] = len;
    peak[c.cell] = pk;
    marks[c.cell] = c.gen;
}

long long workspace_ints(long long n_chunks) { return n_chunks * (CHUNK + 1); }

}  // namespace

extern "C" int cfev_version(void) { return 100; /* 0.1.0 */ }
extern "C" int cfev_abi_version(void) { return CFEV_ABI_VERSION; }
extern "C" const char* cfev_last_error(void) { return g_err; }

extern "C" int cfev_workspace_ints(int n_chunks) {
    if (n_chunks < 1 || workspace_ints(n_chunks) > MAX_ITEMS) return -1;
    return (int)workspace_ints(n_chunks);
}

extern "C" int cfev_detect(const float* scores, int32_t* streak, int32_t* length, float* peak, int32_t* marks, const int32_t* gens,
                           const int32_t* keys, int32_t* events, float* values, int32_t* n_events, int32_t* work,
                           const int32_t* table_host, const int32_t* table_dev, int S, int NOUT, int NKEYS, int max_streams, int cap,
                           float on, float off, int min_on, int min_off, int max_events, cfev_stream_t stream) {
    const char* what = "cfev_detect";
    SIDE_REQUIRE(scores && streak && length && peak && marks && gens && keys && events && values && n_events && work && table_host &&
                     table_dev,
                 "%s: null pointer", what);
    SIDE_REQUIRE(isfinite(on) && isfinite(off), "%s: thresholds on=%g off=%g must be finite", what, (double)on, (double)off);
    SIDE_REQUIRE(off <= on, "%s: thresholds off=%g above on=%g", what, (double)off, (double)on);
    SIDE_REQUIRE(min_on >= 1 && min_off >= 1, "%s: min_on=%d and min_off=%d must be at least 1", what, min_on, min_off);
    SIDE_REQUIRE(max_events >= 1, "%s: max_events=%d must be at least 1", what, max_events);
    SIDE_REQUIRE(max_streams >= 1 && max_streams <= CFEV_MAX_STREAMS, "%s: max_streams=%d outside 1 .. %d", what, max_streams,
                 CFEV_MAX_STREAMS);
    SIDE_REQUIRE(S >= 1 && S <= max_streams, "%s: a table of S=%d rows for max_streams=%d", what, S, max_streams);
    SIDE_REQUIRE(cap >= 1, "%s: cap=%d must be at least 1", what, cap);
    SIDE_REQUIRE((long long)max_streams * cap <= MAX_ITEMS, "%s: too large for one launch (max_streams=%d x cap=%d cells)", what,
                 max_streams, cap);
    SIDE_REQUIRE(NOUT >= 0 && NKEYS >= 1, "%s: bad shape (NOUT=%d NKEYS=%d)", what, NOUT, NKEYS);
    SlotBits seen(max_streams);
    SIDE_REQUIRE(seen.ok(), "%s: out of host memory for %d slots", what, max_streams);
    long long n_out = 0, chunks = 0;
    for (int s = 0; s < S; ++s) {
        const int32_t* d = table_host + (size_t)s * COLS;
        const int slot = d[CFEV_SLOT], nW = d[CFEV_NW], NC = d[CFEV_NC], key0 = d[CFEV_KEY0];
        SIDE_REQUIRE(slot >= 0 && slot < max_streams, "%s: row %d has slot %d outside 0 .. %d", what, s, slot, max_streams - 1);
        SIDE_REQUIRE(!seen.test_and_set(slot), "%s: slot %d appears twice in the table (row %d)", what, slot, s);
        SIDE_REQUIRE(nW >= 0, "%s: row %d has a negative count (nW=%d)", what, s, nW);
        SIDE_REQUIRE(NC >= 1, "%s: row %d has width NC=%d, at least 1 is needed", what, s, NC);
        SIDE_REQUIRE(d[CFEV_OUT0] == n_out && d[CFEV_CHUNK0] == chunks,
                     "%s: row %d has offsets (OUT0=%d, CHUNK0=%d), the prefix sums are (%lld, %lld)", what, s, d[CFEV_OUT0],
                     d[CFEV_CHUNK0], n_out, chunks);
        SIDE_REQUIRE(key0 >= 0 && (long long)key0 + NC <= NKEYS, "%s: row %d has its list at keys[%d .. %lld), outside 0 .. NKEYS=%d", what,
                     s, key0, (long long)key0 + NC, NKEYS);
        n_out += (long long)nW * NC;
        chunks += ((long long)NC + CHUNK - 1) / CHUNK;
        SIDE_REQUIRE(n_out <= MAX_ITEMS && workspace_ints(chunks) <= MAX_ITEMS,
                     "%s: the table's counts are too large for one launch (row %d)", what, s);
    }
    SIDE_REQUIRE(n_out == NOUT, "%s: the table's nW * NC sum to %lld, not to NOUT=%d", what, n_out, NOUT);
    if (NOUT == 0) return 0;                                                   // no session completed a window: nothing to do
    const Rule rule{on, off, min_on, min_off};
    hipStream_t q = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(event_count_kernel, dim3((unsigned)chunks), dim3(CHUNK), 0, q, scores, streak, length, peak, marks, gens, keys, work,
                       table_dev, (unsigned)S, (unsigned)cap, rule);
    hipLaunchKernelGGL(event_scan_kernel, dim3(1), dim3(CHUNK), 0, q, work, n_events, (unsigned)chunks);
    hipLaunchKernelGGL(event_emit_kernel, dim3((unsigned)chunks), dim3(CHUNK), 0, q, scores, streak, length, peak, marks, gens, keys, events,
                       values, work, table_dev, (unsigned)S, (unsigned)cap, rule, (unsigned)max_events);
    return check_launch(what);
}
