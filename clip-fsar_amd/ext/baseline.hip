// Adaptive baselines (libclipfsar_baseline.so, C ABI in include/ext/clipfsar_baseline.h): a running mean and mean absolute deviation per
// (session slot, class store slot) of a stream pool, and every score's deviation z = (s - mean) / dev from them, so that one threshold
// means the same on OTAM logits, on COMBINE probabilities and on a class enrolled a minute ago.  State is keyed as class_smooth.hip keys
// its own -- a cell per (session slot, class store slot), valid iff its mark is the store slot's current generation -- and the descriptor
// table, the key lists and the thread mapping are that library's: one workgroup per (table row, chunk of CFBL_CHUNK columns), found in
// the CHUNK0 column (chunk_row.h), one thread per column, adjacent threads on adjacent columns, sequential in the window k with the cell
// in registers, so the score traffic is coalesced at every k and the state is read and written once per launch.
// Every step of the recurrence is one rounded fp32 operation (__fsub_rn, __fmul_rn, __fdiv_rn, and add_rn below for the two sums of
// products, which must not become fused multiply-adds) -- baseline.reference_baseline restates it bit for bit.
// A plug-in library (build.py, PLUGIN_LIBS): it lives beside csrc/, class_smooth.hip and events.hip, whose files and export sets stay as
// they are.
#include "../csrc/ring_rows.h"
#include "../csrc/side_lib.h"
#include "../../include/ext/clipfsar_baseline.h"
#include "chunk_row.h"

#include <math.h>

namespace {

constexpr int CHUNK = CFBL_CHUNK;
constexpr int COLS = CFBL_TABLE_COLS;

struct Params {
    float rate, warm_rate, gate, floor;
    int32_t warmup;
};

// a + b rounded once, and never contracted with a product that feeds it.  __fadd_rn will not do here: the toolchain's header defines it
// as a plain `a + b` compiled with contraction allowed, and after inlining the backend turns __fadd_rn(__fmul_rn(..), __fmul_rn(..)) into
// v_mul_f32 + v_fmac_f32, one rounding short of the recurrence.  An addition compiled under contract(off) is never fused.
__device__ __forceinline__ float add_rn(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}

// fold s into the cell (m, d) at rate r: a = |s - m| with the old m, then both means move; each product is rounded before its sum
__device__ __forceinline__ void fold(float s, float r, float& m, float& d) {
    const float keep = __fsub_rn(1.0f, r);
    const float a = fabsf(__fsub_rn(s, m));
    m = add_rn(__fmul_rn(keep, m), __fmul_rn(r, s));
    d = add_rn(__fmul_rn(keep, d), __fmul_rn(r, a));
}

// scores and out may be the same buffer: no __restrict__ on them; a thread alone touches its column and its cell
__global__ __launch_bounds__(CHUNK) void baseline_kernel(const float* scores, float* __restrict__ mean, float* __restrict__ dev,
                                                         int32_t* __restrict__ count, int32_t* __restrict__ marks,
                                                         const int32_t* __restrict__ gens, const int32_t* __restrict__ keys, float* out,
                                                         const int32_t* __restrict__ table, unsigned S, unsigned cap, Params p) {
    const int32_t* t = table + find_chunk_row(table, S, blockIdx.x, COLS, CFBL_CHUNK0) * COLS;
    const unsigned nW = (unsigned)t[CFBL_NW], NC = (unsigned)t[CFBL_NC];
    const unsigned j = (blockIdx.x - (unsigned)t[CFBL_CHUNK0]) * CHUNK + threadIdx.x;
    if (nW == 0 || j >= NC) return;                                            // no windows: nothing is touched
    const size_t at = (size_t)t[CFBL_OUT0] + j;
    const unsigned key = (unsigned)keys[(size_t)t[CFBL_KEY0] + j];
    const float nan = __builtin_nanf("");
    if (key >= cap) {                                                          // never dereferenced: a NaN column, no state write
        for (unsigned k = 0; k < nW; ++k) out[at + (size_t)k * NC] = nan;
        return;
    }
    const size_t cell = (size_t)t[CFBL_SLOT] * cap + key;
    const int32_t gen = gens[key];
    float m = 0.f, d = 0.f;
    int32_t n = 0;
    if (marks[cell] == gen) {
        m = mean[cell];
        d = dev[cell];
        n = count[cell];
    }
    for (unsigned k = 0; k < nW; ++k) {
        const float s = scores[at + (size_t)k * NC];
        float z = nan;
        if (isfinite(s)) {
            if (n == 0) {
                m = s, d = 0.f, n = 1;
            } else if (n < p.warmup) {
                fold(s, p.warm_rate, m, d);
                n += 1;
            } else {
                z = __fdiv_rn(__fsub_rn(s, m), fmaxf(d, p.floor));
                if (!(z >= p.gate)) fold(s, p.rate, m, d);
            }
        }
        out[at + (size_t)k * NC] = z;
    }
    mean[cell] = m;
    dev[cell] = d;
    count[cell] = n;
    marks[cell] = gen;
}

}  // namespace

extern "C" int cfbl_version(void) { return 100; /* 0.1.0 */ }
extern "C" int cfbl_abi_version(void) { return CFBL_ABI_VERSION; }
extern "C" const char* cfbl_last_error(void) { return g_err; }

extern "C" int cfbl_normalize(const float* scores, float* mean, float* dev, int32_t* count, int32_t* marks, const int32_t* gens,
                              const int32_t* keys, float* out, const int32_t* table_host, const int32_t* table_dev, int S, int NOUT,
                              int NKEYS, int max_streams, int cap, float rate, float warm_rate, int warmup, float gate, float dev_floor,
                              cfbl_stream_t stream) {
    const char* what = "cfbl_normalize";
    SIDE_REQUIRE(scores && mean && dev && count && marks && gens && keys && out && table_host && table_dev, "%s: null pointer", what);
    SIDE_REQUIRE(rate > 0.0f && rate < 1.0f, "%s: rate=%g outside (0, 1)", what, (double)rate);
    SIDE_REQUIRE(warm_rate > 0.0f && warm_rate <= 1.0f, "%s: warm_rate=%g outside (0, 1]", what, (double)warm_rate);
    SIDE_REQUIRE(warmup >= 1 && warmup <= CFBL_MAX_WARMUP, "%s: warmup=%d outside 1 .. %d", what, warmup, CFBL_MAX_WARMUP);
    SIDE_REQUIRE(gate > 0.0f, "%s: gate=%g must be above 0 (+inf: nothing is gated)", what, (double)gate);
    SIDE_REQUIRE(dev_floor > 0.0f && isfinite(dev_floor), "%s: floor=%g must be above 0 and finite", what, (double)dev_floor);
    SIDE_REQUIRE(max_streams >= 1 && max_streams <= CFBL_MAX_STREAMS, "%s: max_streams=%d outside 1 .. %d", what, max_streams,
                 CFBL_MAX_STREAMS);
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
        const int slot = d[CFBL_SLOT], nW = d[CFBL_NW], NC = d[CFBL_NC], key0 = d[CFBL_KEY0];
        SIDE_REQUIRE(slot >= 0 && slot < max_streams, "%s: row %d has slot %d outside 0 .. %d", what, s, slot, max_streams - 1);
        SIDE_REQUIRE(!seen.test_and_set(slot), "%s: slot %d appears twice in the table (row %d)", what, slot, s);
        SIDE_REQUIRE(nW >= 0, "%s: row %d has a negative count (nW=%d)", what, s, nW);
        SIDE_REQUIRE(NC >= 1, "%s: row %d has width NC=%d, at least 1 is needed", what, s, NC);
        SIDE_REQUIRE(d[CFBL_OUT0] == n_out && d[CFBL_CHUNK0] == chunks,
                     "%s: row %d has offsets (OUT0=%d, CHUNK0=%d), the prefix sums are (%lld, %lld)", what, s, d[CFBL_OUT0],
                     d[CFBL_CHUNK0], n_out, chunks);
        SIDE_REQUIRE(key0 >= 0 && (long long)key0 + NC <= NKEYS, "%s: row %d has its list at keys[%d .. %lld), outside 0 .. NKEYS=%d", what,
                     s, key0, (long long)key0 + NC, NKEYS);
        n_out += (long long)nW * NC;
        chunks += ((long long)NC + CHUNK - 1) / CHUNK;
        SIDE_REQUIRE(n_out <= MAX_ITEMS && chunks <= MAX_ITEMS, "%s: the table's counts are too large for one launch (row %d)", what, s);
    }
    SIDE_REQUIRE(n_out == NOUT, "%s: the table's nW * NC sum to %lld, not to NOUT=%d", what, n_out, NOUT);
    if (NOUT == 0) return 0;                                                   // no session completed a window: nothing to do
    const Params p{rate, warm_rate, gate, dev_floor, warmup};
    hipLaunchKernelGGL(baseline_kernel, dim3((unsigned)chunks), dim3(CHUNK), 0, static_cast<hipStream_t>(stream), scores, mean, dev, count,
                       marks, gens, keys, out, table_dev, (unsigned)S, (unsigned)cap, p);
    return check_launch(what);
}
