// The selection of a stream pool with a shortlist (libclipfsar_pool_select.so, C ABI in include/ext/clipfsar_pool_select.h): cfsh_select's
// threshold select over a session's windows, with the columns the pool's state is not done with PINNED into the list, and the commit that
// makes a gap a fresh start -- the marks of a (session slot, store slot) pair that was not scored at the session's previous scoring push
// are zeroed here, ahead of the smoothing, baseline and detector launches that read them.
// One 256-thread workgroup per group (a session): it counts the group's pins, writes the group scores into `work` as keys in which the
// pins are folded -- P <= K: a pin's key is 0xffffffff, above the key of every score, so the K best keys are all pins and the best of the
// rest; P > K: a column that is not pinned has key 0, not selectable, and a pin without a score key 1, below every score -- and runs the
// radix passes and the compaction of select_keys.h, the body shortlist.hip's select_kernel runs.  A kept column's thread writes its place
// and commits its cell; a group's workgroup alone touches its slot's rows of the planes (the host rows are checked for a slot named
// twice), so there is no race, and the only atomics are the histogram counts in LDS.
// A plug-in library (build.py, PLUGIN_LIBS): it lives beside csrc/, whose files and export sets stay as they are.
#include "../csrc/side_lib.h"
#include "../../include/ext/clipfsar_pool_select.h"
#include "select_keys.h"

#include <math.h>

namespace {

constexpr int COLS = CFPS_TABLE_COLS;
constexpr int WG = SEL_WG, WAVES = SEL_WAVES;
constexpr long long MAX_32 = 0x7fffffffLL;
constexpr unsigned PIN_KEY = 0xffffffffu;                                     // above +inf's key, 0xff800000
constexpr unsigned BARE_PIN_KEY = 1u;                                         // below -FLT_MAX's key, 0x00800000

// What decides whether a column of the group is pinned: the group's rows of the planes (`row` = slot * cap) and the rule's numbers.
struct Pins {
    const int32_t* __restrict__ cols;
    const int32_t* __restrict__ gens;
    const int32_t* ev_streak;                                                 // the planes the commit writes carry no __restrict__
    const int32_t* ev_marks;
    const int32_t* seen;
    const int32_t* merit;
    size_t row;
    int cap, tick, hold;
    // the CFPS_PIN_* bits of column c; 0: not pinned.  A key outside [0, cap) is never dereferenced.
    __device__ __forceinline__ unsigned operator()(int c) const {
        const unsigned key = (unsigned)cols[c];
        if (key >= (unsigned)cap) return 0u;
        const size_t cell = row + key;
        if (seen[cell] != tick - 1) return 0u;
        unsigned bits = 0u;
        if (ev_marks && ev_marks[cell] == gens[key] && ev_streak[cell] != 0) bits |= CFPS_PIN_EVENT;
        if (hold > 0) {
            const int32_t m = merit[cell];
            if (m >= 1 && (long long)tick - m <= hold) bits |= CFPS_PIN_HOLD;
        }
        return bits;
    }
};

// the workgroup's sum of v: the waves' sums by shuffles, then through LDS.  Every thread calls it; ends on a barrier.
__device__ __forceinline__ unsigned block_sum(unsigned v, unsigned* part) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_down(v, o, 64);
    if (lane == 0) part[wave] = v;
    __syncthreads();
    unsigned all = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) all += part[w];
    __syncthreads();
    return all;
}

__global__ __launch_bounds__(WG) void select_pinned_kernel(const float* __restrict__ S, const int32_t* __restrict__ cols,
                                                           const int32_t* __restrict__ gens, const int32_t* ev_streak, int32_t* ev_marks,
                                                           int32_t* seen, int32_t* merit, int32_t* smooth_marks, int32_t* base_marks,
                                                           const int32_t* __restrict__ table, unsigned* __restrict__ work, int NQ, int NC, int K,
                                                           int hold, int max_streams, int cap, int32_t* __restrict__ sel_cols,
                                                           int32_t* __restrict__ sel_slots, int32_t* __restrict__ sel_pin,
                                                           int32_t* __restrict__ n_pins) {
    __shared__ unsigned hist[WAVES * 256];                                    // a histogram per wave
    __shared__ unsigned part[WAVES];
    __shared__ unsigned pick[2];
    const int tid = threadIdx.x;
    const unsigned g = blockIdx.x;
    const int32_t* d = table + (size_t)g * COLS;
    int q_first = d[CFPS_Q0], nq = d[CFPS_NQ];
    const int slot = d[CFPS_SLOT], tick = d[CFPS_TICK];
    if (q_first < 0 || nq < 0 || (long long)q_first + nq > NQ || slot < 0 || slot >= max_streams || tick < 1)
        nq = 0;                                                               // a device table that is not the validated host rows
    int32_t* oc = sel_cols + (size_t)g * K;
    int32_t* os = sel_slots + (size_t)g * K;
    int32_t* op = sel_pin + (size_t)g * K;
    unsigned n_out = 0, P = 0;
    if (nq > 0) {                                                             // uniform
        const Pins pins{cols, gens, ev_streak, ev_marks, seen, merit, (size_t)slot * (size_t)cap, cap, tick, hold};
        // 0. the pins, counted: most columns answer with one load (seen)
        unsigned mine = 0;
        for (int c = tid; c < NC; c += WG) mine += pins(c) != 0u;
        P = block_sum(mine, part);
        const bool all_pins_fit = P <= (unsigned)K;
        // 1. the group scores as keys, the pins folded in
        unsigned* keys = work + (size_t)g * NC;
        for (int c = tid; c < NC; c += WG) {
            const unsigned k = group_score_key(S, q_first, nq, NC, c);
            const bool pinned = pins(c) != 0u;
            keys[c] = all_pins_fit ? (pinned ? PIN_KEY : k) : (pinned ? (k ? k : BARE_PIN_KEY) : 0u);
        }
        __syncthreads();
        // 2. the K-th largest key, 3. compaction in ascending column order; a kept column writes its place and commits its cell
        unsigned left;
        const unsigned thr = kth_largest_key(keys, NC, (unsigned)K, hist, pick, [&](unsigned cell) { atomicAdd(&hist[cell], 1u); }, left);
        n_out = compact_selected(keys, NC, (unsigned)K, thr, thr ? left : 0u, part, [&](unsigned at, int c) {
            const unsigned bits = pins(c);                                    // read before this thread's own writes below
            const int32_t key = cols[c];
            oc[at] = c;
            os[at] = key;
            op[at] = (int32_t)bits;
            if ((unsigned)key < (unsigned)cap) {
                const size_t cell = pins.row + (unsigned)key;
                if (seen[cell] != tick - 1) {                                 // new, or back after a gap: every state starts anew
                    if (smooth_marks) smooth_marks[cell] = 0;
                    if (base_marks) base_marks[cell] = 0;
                    if (ev_marks) ev_marks[cell] = 0;
                }
                seen[cell] = tick;
                if (bits == 0u) merit[cell] = tick;
            }
        });
    }
    for (unsigned r = n_out + tid; r < (unsigned)K; r += WG) {                // padding, at the end
        oc[r] = CFPS_NONE;
        os[r] = -1;
        op[r] = 0;
    }
    if (tid == 0) n_pins[g] = (int32_t)P;
}

}  // namespace

extern "C" int cfps_version(void) { return 100; /* 0.1.0 */ }
extern "C" int cfps_abi_version(void) { return CFPS_ABI_VERSION; }
extern "C" const char* cfps_last_error(void) { return g_err; }

extern "C" int cfps_workspace_floats(int G, int NC) {
    if (G < 1 || G > CFPS_MAX_GROUPS || NC < 1 || (long long)G * NC > MAX_32) return -1;
    return G * NC;
}

extern "C" int cfps_select_pinned(const float* S, const int32_t* cols, const int32_t* gens, const int32_t* ev_streak, int32_t* ev_marks,
                                  int32_t* seen, int32_t* merit, int32_t* smooth_marks, int32_t* base_marks, const int32_t* table_host,
                                  const int32_t* table_dev, int G, int NQ, int NC, int keep, int hold, int max_streams, int cap,
                                  int32_t* sel_cols, int32_t* sel_slots, int32_t* sel_pin, int32_t* n_pins, float* work,
                                  cfps_stream_t stream) {
    const char* who = "cfps_select_pinned";
    SIDE_REQUIRE(S && cols && gens && seen && merit && table_host && table_dev && sel_cols && sel_slots && sel_pin && n_pins && work,
                 "%s: null pointer (ev_streak with ev_marks, smooth_marks and base_marks alone may be null)", who);
    SIDE_REQUIRE(!ev_streak == !ev_marks, "%s: ev_streak and ev_marks are both null or both given (ev_streak %s, ev_marks %s)", who,
                 ev_streak ? "given" : "null", ev_marks ? "given" : "null");
    SIDE_REQUIRE(G >= 1 && G <= CFPS_MAX_GROUPS, "%s: a table of G=%d groups (1 .. %d)", who, G, CFPS_MAX_GROUPS);
    SIDE_REQUIRE(NQ >= 1, "%s: NQ=%d queries, at least 1 is needed", who, NQ);
    SIDE_REQUIRE(NC >= 1, "%s: NC=%d columns, at least 1 is needed", who, NC);
    SIDE_REQUIRE(keep >= 1 && keep <= CFPS_MAX_KEEP, "%s: keep=%d outside 1 .. %d", who, keep, CFPS_MAX_KEEP);
    SIDE_REQUIRE(hold >= 0 && hold <= CFPS_MAX_HOLD, "%s: hold=%d outside 0 .. %d", who, hold, CFPS_MAX_HOLD);
    SIDE_REQUIRE(max_streams >= 1 && max_streams <= CFPS_MAX_STREAMS, "%s: max_streams=%d outside 1 .. %d", who, max_streams,
                 CFPS_MAX_STREAMS);
    SIDE_REQUIRE(cap >= 1, "%s: cap=%d slots, at least 1 is needed", who, cap);
    SIDE_REQUIRE((long long)max_streams * cap <= MAX_32, "%s: max_streams * cap = %lld cells exceed 32-bit sizes", who,
                 (long long)max_streams * cap);
    SIDE_REQUIRE(G <= max_streams, "%s: a table of G=%d groups for max_streams=%d", who, G, max_streams);
    SIDE_REQUIRE((long long)NQ * NC <= MAX_32, "%s: NQ * NC = %lld scores exceed 32-bit sizes", who, (long long)NQ * NC);
    SIDE_REQUIRE((long long)G * NC <= MAX_32, "%s: G * NC = %lld group scores exceed 32-bit sizes", who, (long long)G * NC);
    SlotBits named(max_streams);
    SIDE_REQUIRE(named.ok(), "%s: out of host memory for %d slots", who, max_streams);
    long long q = 0;
    for (int g = 0; g < G; ++g) {
        const int32_t* d = table_host + (size_t)g * COLS;
        SIDE_REQUIRE(d[CFPS_NQ] >= 0, "%s: group %d has NQ=%d queries, a count cannot be negative", who, g, d[CFPS_NQ]);
        SIDE_REQUIRE(d[CFPS_Q0] == q, "%s: group %d has Q0=%d, the queries of the groups before it add up to %lld", who, g, d[CFPS_Q0], q);
        q += d[CFPS_NQ];
        SIDE_REQUIRE(q <= MAX_32, "%s: the counts up to group %d (%lld queries) exceed 32-bit sizes", who, g, q);
        SIDE_REQUIRE(d[CFPS_SLOT] >= 0 && d[CFPS_SLOT] < max_streams, "%s: group %d has SLOT=%d outside 0 .. %d", who, g, d[CFPS_SLOT],
                     max_streams - 1);
        SIDE_REQUIRE(!named.test_and_set(d[CFPS_SLOT]), "%s: SLOT=%d appears twice in the table (group %d)", who, d[CFPS_SLOT], g);
        SIDE_REQUIRE(d[CFPS_TICK] >= 1, "%s: group %d has TICK=%d, a session's scoring pushes count from 1", who, g, d[CFPS_TICK]);
    }
    SIDE_REQUIRE(q == NQ, "%s: the groups add up to %lld queries, not to NQ = %d", who, q, NQ);
    hipLaunchKernelGGL(select_pinned_kernel, dim3((unsigned)G), dim3(WG), 0, static_cast<hipStream_t>(stream), S, cols, gens, ev_streak,
                       ev_marks, seen, merit, smooth_marks, base_marks, table_dev, reinterpret_cast<unsigned*>(work), NQ, NC,
                       keep < NC ? keep : NC, hold, max_streams, cap, sel_cols, sel_slots, sel_pin, n_pins);
    return check_launch(who);
}
