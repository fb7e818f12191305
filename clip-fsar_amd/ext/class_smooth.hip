// Per-class smoothing (libclipfsar_class_smooth.so, C ABI in include/ext/clipfsar_class_smooth.h): the smoothing recurrence of a stream
// pool over state keyed by (session slot, class store slot).  pool.hip smooths against state [max_streams, C] by column; here a column of
// a session's block is looked up in its store-slot list and the cell is valid iff its mark is the slot's current generation, so classes
// come and go, and sessions keep lists of their own, without anyone resetting the state.
// One workgroup per (table row, chunk of CFCS_CHUNK columns), found in the CHUNK0 column as pool.hip's find_row and groups.hip's
// find_group find theirs: the workgroup number is uniform, so the search runs on scalar values.  One thread per column; adjacent threads
// take adjacent columns, so the logits traffic is coalesced at every window k.  The recurrence itself is ring_rows.h's smooth_run.
// An extension library (build.py, EXT_LIBS): it lives beside csrc/, whose files and the ten side libraries' export sets stay as they are.
#include "../csrc/ring_rows.h"
#include "../csrc/side_lib.h"
#include "../../include/ext/clipfsar_class_smooth.h"

namespace {

constexpr int CHUNK = CFCS_CHUNK;
constexpr int COLS = CFCS_TABLE_COLS;

// the table row whose CHUNK0 is the last one <= b (every row has NC >= 1, so CHUNK0 rises strictly).  Everything here is uniform.
__device__ __forceinline__ const int32_t* find_chunk_row(const int32_t* __restrict__ table, unsigned S, unsigned b) {
    unsigned lo = 0, hi = S;                   // table[lo][CHUNK0] <= b; hi == S or table[hi][CHUNK0] > b
    while (hi - lo > 1) {
        const unsigned mid = (lo + hi) >> 1;
        if ((unsigned)table[mid * COLS + CFCS_CHUNK0] <= b) lo = mid;
        else hi = mid;
    }
    return table + lo * COLS;
}

// logits and out may be the same buffer: no __restrict__ on them; a thread alone touches its column and its cell
__global__ __launch_bounds__(CHUNK) void class_smooth_kernel(const float* logits, float* __restrict__ state, int32_t* __restrict__ marks,
                                                             const int32_t* __restrict__ gens, const int32_t* __restrict__ keys, float* out,
                                                             const int32_t* __restrict__ table, unsigned S, unsigned cap, float alpha) {
    const int32_t* d = find_chunk_row(table, S, blockIdx.x);
    const unsigned nW = (unsigned)d[CFCS_NW], NC = (unsigned)d[CFCS_NC];
    const unsigned j = (blockIdx.x - (unsigned)d[CFCS_CHUNK0]) * CHUNK + threadIdx.x;
    if (nW == 0 || j >= NC) return;                                            // no windows: state and marks stay as they are
    const size_t at = (size_t)d[CFCS_OUT0] + j;
    const unsigned key = (unsigned)keys[(size_t)d[CFCS_KEY0] + j];
    if (key >= cap) {                                                          // never dereferenced: a NaN column, no state write
        for (unsigned k = 0; k < nW; ++k) out[at + (size_t)k * NC] = __builtin_nanf("");
        return;
    }
    const size_t cell = (size_t)d[CFCS_SLOT] * cap + key;
    const int32_t gen = gens[key];
    smooth_run(logits + at, out + at, state + cell, nW, NC, alpha, __fsub_rn(1.0f, alpha), marks[cell] == gen);
    marks[cell] = gen;
}

}  // namespace

extern "C" int cfcs_version(void) { return 100; /* 0.1.0 */ }
extern "C" int cfcs_abi_version(void) { return CFCS_ABI_VERSION; }
extern "C" const char* cfcs_last_error(void) { return g_err; }

extern "C" int cfcs_smooth_classes(const float* logits, float* state, int32_t* marks, const int32_t* gens, const int32_t* keys, float* out,
                                   const int32_t* table_host, const int32_t* table_dev, int S, int NOUT, int NKEYS, int max_streams,
                                   int cap, float alpha, cfcs_stream_t stream) {
    const char* what = "cfcs_smooth_classes";
    SIDE_REQUIRE(logits && state && marks && gens && keys && out && table_host && table_dev, "%s: null pointer", what);
    SIDE_REQUIRE(alpha >= 0.0f && alpha < 1.0f, "%s: alpha=%g outside [0, 1)", what, (double)alpha);
    SIDE_REQUIRE(max_streams >= 1 && max_streams <= CFCS_MAX_STREAMS, "%s: max_streams=%d outside 1 .. %d", what, max_streams,
                 CFCS_MAX_STREAMS);
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
        const int slot = d[CFCS_SLOT], nW = d[CFCS_NW], NC = d[CFCS_NC], key0 = d[CFCS_KEY0];
        SIDE_REQUIRE(slot >= 0 && slot < max_streams, "%s: row %d has slot %d outside 0 .. %d", what, s, slot, max_streams - 1);
        SIDE_REQUIRE(!seen.test_and_set(slot), "%s: slot %d appears twice in the table (row %d)", what, slot, s);
        SIDE_REQUIRE(nW >= 0, "%s: row %d has a negative count (nW=%d)", what, s, nW);
        SIDE_REQUIRE(NC >= 1, "%s: row %d has width NC=%d, at least 1 is needed", what, s, NC);
        SIDE_REQUIRE(d[CFCS_OUT0] == n_out && d[CFCS_CHUNK0] == chunks,
                     "%s: row %d has offsets (OUT0=%d, CHUNK0=%d), the prefix sums are (%lld, %lld)", what, s, d[CFCS_OUT0],
                     d[CFCS_CHUNK0], n_out, chunks);
        SIDE_REQUIRE(key0 >= 0 && (long long)key0 + NC <= NKEYS, "%s: row %d has its list at keys[%d .. %lld), outside 0 .. NKEYS=%d", what,
                     s, key0, (long long)key0 + NC, NKEYS);
        n_out += (long long)nW * NC;
        chunks += ((long long)NC + CHUNK - 1) / CHUNK;
        SIDE_REQUIRE(n_out <= MAX_ITEMS && chunks <= MAX_ITEMS, "%s: the table's counts are too large for one launch (row %d)", what, s);
    }
    SIDE_REQUIRE(n_out == NOUT, "%s: the table's nW * NC sum to %lld, not to NOUT=%d", what, n_out, NOUT);
    if (NOUT == 0) return 0;                                                   // no session completed a window: nothing to do
    hipLaunchKernelGGL(class_smooth_kernel, dim3((unsigned)chunks), dim3(CHUNK), 0, static_cast<hipStream_t>(stream), logits, state, marks,
                       gens, keys, out, table_dev, (unsigned)S, (unsigned)cap, alpha);
    return check_launch(what);
}
