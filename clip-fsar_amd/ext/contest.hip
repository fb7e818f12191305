// The contest of a stream pool with an event rule (libclipfsar_contest.so, C ABI in include/ext/clipfsar_contest.h): one stage between
// the judged scores of a push and cfev_detect that ranks every window's row and demotes the losers to -inf.  The table, the key lists and
// the flat score layout are the detector's (events.hip) and class_smooth.hip's.  The selection is the threshold select of select_keys.h,
// which shortlist.hip's select_kernel and pool_select.hip run: the row's scores as order-preserving keys, the R-th largest key by four
// radix passes over per-wave histograms in LDS, then a scan that compacts the columns above the threshold and the first few equal to it
// in ascending column order.  It is RESTATED here, not included: the build's staleness matrix pins select_keys.h to exactly those two
// libraries (tests/test_pool_select_abi.py), and a third includer would change what an edit of that header rebuilds.  The key, the tie
// rule and the order are the header's, and tests/test_gpu_contest.py holds this copy to clip_fsar_amd.contest.reference_contest bit for
// bit.  What is new is the row it runs on -- one window of one session, not a group's maximum over queries -- the row maximum that turns
// a margin into a second threshold, and what a selected column writes: its own score back over the -inf that the demoted plane gave it.
// One 256-thread workgroup per (table row, window); a column is handled by the same thread in every step, so the plane needs nothing
// beyond program order and the barriers the steps end on.  No workgroup waits on another, a leader's place is a prefix sum, and the one
// atomic is the histogram count in LDS, whose sums do not depend on their order.  The contest keeps no state.
// A plug-in library (build.py, PLUGIN_LIBS): it lives beside csrc/, whose files and export sets stay as they are.
#include "../csrc/side_lib.h"
#include "../../include/ext/clipfsar_contest.h"

#include <math.h>

namespace {

constexpr int COLS = CFCT_TABLE_COLS;
constexpr int WG = 256, WAVES = WG / 64;
constexpr long long MAX_32 = 0x7fffffffLL;
constexpr unsigned MAX_GRID_Y = 65535;

// a score as a key that orders as the floats do: larger float, larger key; -0.0 folded into +0.0; 0 = no candidate (not `valid`, NaN, or
// -inf, whose key would be 0x007fffff: every candidate's key is at least 0x00800000, that of -FLT_MAX, and at most 0xff800000, +inf's)
__device__ __forceinline__ unsigned score_key(float v, bool valid) {
    if (!valid || !(v > -__builtin_inff())) return 0u;
    const unsigned u = v == 0.0f ? 0u : __float_as_uint(v);                   // both zeros: the bits of +0.0
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// exclusive prefix of a flag over the workgroup's threads in thread order, and the workgroup's total: a ballot per wave, the waves'
// counts through LDS.  Every thread calls it; `part` is WAVES words, free to be rewritten after the call's second barrier.
__device__ __forceinline__ unsigned block_prefix(bool flag, unsigned* part, unsigned& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long m = __ballot(flag);
    if (lane == 0) part[wave] = (unsigned)__popcll(m);
    __syncthreads();
    unsigned before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
        const unsigned n = part[w];
        before += w < wave ? n : 0u;
        all += n;
    }
    __syncthreads();
    total = all;
    return before + (unsigned)__popcll(m & ((1ull << lane) - 1ull));
}

// The K-th largest of keys[0 .. NC), 1 <= K <= the number of keys above 0, a byte per pass from the top: of the keys that share the bytes
// found so far, count the next byte's values (a histogram per wave, the one atomic), then walk the counts from 255 down until `left` of
// them are covered.  hist: WAVES * 256 counters in LDS; pick: 2 words in LDS.  -> the key; `left` of the keys equal to it are kept.
// The keys must be visible to the workgroup (a barrier behind their writes); the call ends on a barrier.
__device__ __forceinline__ unsigned kth_largest_key(const unsigned* keys, int NC, unsigned K, unsigned* hist, unsigned* pick, unsigned& left) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned prefix = 0;
    left = K;
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        const unsigned mask = pass ? 0xffffffffu << (shift + 8) : 0u;
        for (int i = tid; i < WAVES * 256; i += WG) hist[i] = 0;
        __syncthreads();
        for (int c = tid; c < NC; c += WG) {
            const unsigned k = keys[c];
            if ((k & mask) == prefix) atomicAdd(&hist[wave * 256 + ((k >> shift) & 255u)], 1u);
        }
        __syncthreads();
        if (wave == 0) {                                                      // lane l owns the values 4 l .. 4 l + 3
            unsigned s[4], mine = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                s[j] = 0;
#pragma unroll
                for (int w = 0; w < WAVES; ++w) s[j] += hist[w * 256 + 4 * lane + j];
                mine += s[j];
            }
            unsigned suffix = mine;                                           // -> the count over this lane's values and all above
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const unsigned v = __shfl_down(suffix, o, 64);
                if (lane + o < 64) suffix += v;
            }
            unsigned above = suffix - mine;
#pragma unroll
            for (int j = 3; j >= 0; --j) {
                const unsigned incl = above + s[j];
                if (above < left && incl >= left) {                           // exactly one (lane, j): left >= 1, and K candidates exist
                    pick[0] = (unsigned)(4 * lane + j);
                    pick[1] = left - above;
                }
                above = incl;
            }
        }
        __syncthreads();
        prefix |= pick[0] << shift;
        left = pick[1];
    }
    return prefix;
}

// Compaction in ascending column order, WG columns at a time: the columns whose key is above thr, and the first need_eq of those equal to
// it.  put(place, column) is called once per kept column, place < K, by the column's thread.  -> the number of places filled (uniform).
template <class Put>
__device__ __forceinline__ unsigned compact_selected(const unsigned* keys, int NC, unsigned K, unsigned thr, unsigned need_eq, unsigned* part,
                                                     Put put) {
    const int tid = threadIdx.x;
    unsigned n_eq = 0, n_out = 0;                                             // equal keys seen, places written: uniform
    for (int c0 = 0; c0 < NC; c0 += WG) {
        const int c = c0 + tid;
        const unsigned k = c < NC ? keys[c] : 0u;
        const bool gt = k > thr, eq = k == thr;                               // (thr >= 0x007fffff here: a key of 0 is neither)
        unsigned eq_total, take_total;
        const unsigned eq_rank = n_eq + block_prefix(eq, part, eq_total);
        const bool take = gt || (eq && eq_rank < need_eq);
        const unsigned at = n_out + block_prefix(take, part, take_total);
        if (take && at < K) put(at, c);
        n_eq += eq_total;
        n_out += take_total;
    }
    return n_out < K ? n_out : K;
}

// the float behind a key of score_key (key != 0); both zeros come back as +0.0
__device__ __forceinline__ float key_score(unsigned key) { return __uint_as_float((key & 0x80000000u) ? (key & 0x7fffffffu) : ~key); }

// maximum of mx and sum of n over the workgroup, to every thread: the waves' lanes by shuffles, the waves through LDS.  Every thread calls
// it; `red` is 2 * WAVES words.  It ends on a barrier, so it may be called again at once.
__device__ __forceinline__ void block_max_sum(unsigned& mx, unsigned& n, unsigned* red) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {                                        // lane 0 ends with the wave's: lane l < o takes lane l + o
        mx = max(mx, (unsigned)__shfl_down(mx, o, 64));
        n += (unsigned)__shfl_down(n, o, 64);
    }
    if (lane == 0) {
        red[wave] = mx;
        red[WAVES + wave] = n;
    }
    __syncthreads();
    mx = 0, n = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
        mx = max(mx, red[w]);
        n += red[WAVES + w];
    }
    __syncthreads();
}

struct Margin {
    int has;
    float value;
};

__global__ __launch_bounds__(WG) void contest_kernel(const float* __restrict__ scores, const int32_t* __restrict__ keys, float* __restrict__ out,
                                                     int32_t* __restrict__ leaders, int32_t* __restrict__ n_leaders, unsigned* __restrict__ work,
                                                     const int32_t* __restrict__ table, unsigned NOUT, unsigned NKEYS, unsigned n_rows,
                                                     unsigned cap, unsigned top, Margin margin) {
    __shared__ unsigned hist[WAVES * 256];                                    // a histogram per wave
    __shared__ unsigned part[WAVES];
    __shared__ unsigned pick[2];                                              // the pass's digit, and what is left of R below it
    __shared__ unsigned red[2 * WAVES];
    const int tid = threadIdx.x;
    const int32_t* d = table + (size_t)blockIdx.x * COLS;
    const long long nW = d[CFCT_NW], NC = d[CFCT_NC], out0 = d[CFCT_OUT0], key0 = d[CFCT_KEY0];
    // a device table that is not the validated host rows: the row touches nothing
    if (nW <= 0 || NC < 1 || out0 < 0 || out0 + nW * NC > (long long)NOUT) return;
    if (keys && (key0 < 0 || key0 + NC > (long long)NKEYS)) return;
    if (blockIdx.y >= nW) return;                                             // the grid is as high as the longest row (everything above is uniform)
    // the ordinal of the row's first window among the table's windows: the NW of the rows before it, at most 65536 adds a workgroup
    unsigned first = 0, unused = 0;
    if (leaders) {
        for (unsigned r = tid; r < blockIdx.x; r += WG) first += (unsigned)max(table[(size_t)r * COLS + CFCT_NW], 0);
        block_max_sum(unused, first, red);
    }
    const int32_t* kk = keys ? keys + key0 : nullptr;
    const int nc = (int)NC;
    for (long long k = blockIdx.y; k < nW; k += gridDim.y) {
        const size_t at = (size_t)out0 + (size_t)k * nc;
        const float* x = scores + at;
        float* o = out + at;
        unsigned* rk = work + at;
        // 1. the row's scores as keys, their maximum and the number of candidates (key != 0)
        unsigned best = 0, n_cand = 0;
        for (int c = tid; c < nc; c += WG) {
            const unsigned key = score_key(x[c], !kk || (unsigned)kk[c] < cap);
            rk[c] = key;
            best = max(best, key);
            n_cand += key != 0u;
        }
        block_max_sum(best, n_cand, red);                                     // (its barriers make the keys visible to the workgroup)
        // 2. the R-th largest key, R = min(top, candidates); `left` of the keys equal to it are kept, the lowest columns first.  A margin's
        // floor above that key is the threshold instead, and every key at or above it is kept.
        const unsigned R = min(top, n_cand);
        unsigned thr = 0xffffffffu, need_eq = 0;                              // no candidate: nothing to select
        if (R) {
            thr = kth_largest_key(rk, nc, R, hist, pick, need_eq);
            if (margin.has) {
                const unsigned floor_key = score_key(key_score(best) - margin.value, true);
                if (floor_key > thr) thr = floor_key - 1u, need_eq = 0;
            }
        }
        // 3. the demoted plane: a candidate becomes -inf, everything else keeps its bits
        for (int c = tid; c < nc; c += WG) {
            const float v = x[c];
            o[c] = rk[c] ? -__builtin_inff() : v;
        }
        // 4. the leaders in ascending column order: each takes its score back (the column's own thread wrote the -inf) and its place
        unsigned n_lead = 0;
        const size_t ord = (size_t)first + (size_t)k;
        int32_t* lead = leaders && ord < n_rows ? leaders + ord * top : nullptr;
        if (R)
            n_lead = compact_selected(rk, nc, R, thr, need_eq, part, [&](unsigned place, int c) {
                o[c] = x[c];
                if (lead) lead[place] = c;
            });
        if (lead) {
            for (unsigned r = n_lead + tid; r < top; r += WG) lead[r] = CFCT_NONE;
            if (tid == 0) n_leaders[ord] = (int32_t)n_lead;
        }
    }
}

}  // namespace

extern "C" int cfct_version(void) { return 100; /* 0.1.0 */ }
extern "C" int cfct_abi_version(void) { return CFCT_ABI_VERSION; }
extern "C" const char* cfct_last_error(void) { return g_err; }

extern "C" int cfct_workspace_words(int NOUT) { return NOUT < 0 ? -1 : NOUT; }

extern "C" int cfct_contest(const float* scores, const int32_t* keys, float* out, int32_t* leaders, int32_t* n_leaders, uint32_t* work,
                            const int32_t* table_host, const int32_t* table_dev, int S, int NOUT, int NKEYS, int cap, int top,
                            int has_margin, float margin, cfct_stream_t stream) {
    const char* what = "cfct_contest";
    SIDE_REQUIRE(scores && out && work && table_host && table_dev, "%s: null pointer (scores, out, work, table_host or table_dev)", what);
    SIDE_REQUIRE(!leaders == !n_leaders, "%s: leaders and n_leaders go together, %s alone is given", what, leaders ? "leaders" : "n_leaders");
    SIDE_REQUIRE(S >= 1 && S <= CFCT_MAX_STREAMS, "%s: a table of S=%d rows (1 .. %d)", what, S, CFCT_MAX_STREAMS);
    SIDE_REQUIRE(NOUT >= 0, "%s: bad shape (NOUT=%d)", what, NOUT);
    SIDE_REQUIRE(top >= 1, "%s: top=%d must be at least 1", what, top);
    if (keys) {
        SIDE_REQUIRE(NKEYS >= 1, "%s: bad shape (NKEYS=%d with a key list)", what, NKEYS);
        SIDE_REQUIRE(cap >= 1, "%s: cap=%d must be at least 1", what, cap);
    }
    SIDE_REQUIRE(!has_margin || (isfinite(margin) && margin >= 0.0f), "%s: margin=%g must be finite and at least 0", what, (double)margin);
    long long n_out = 0, n_rows = 0, longest = 0;
    for (int s = 0; s < S; ++s) {
        const int32_t* d = table_host + (size_t)s * COLS;
        const int nW = d[CFCT_NW], NC = d[CFCT_NC], key0 = d[CFCT_KEY0];
        SIDE_REQUIRE(nW >= 0, "%s: row %d has a negative count (nW=%d)", what, s, nW);
        SIDE_REQUIRE(NC >= 1, "%s: row %d has width NC=%d, at least 1 is needed", what, s, NC);
        SIDE_REQUIRE(d[CFCT_OUT0] == n_out, "%s: row %d has OUT0=%d, the nW * NC of the rows before it add up to %lld", what, s, d[CFCT_OUT0],
                     n_out);
        SIDE_REQUIRE(!keys || (key0 >= 0 && (long long)key0 + NC <= NKEYS), "%s: row %d has its list at keys[%d .. %lld), outside 0 .. NKEYS=%d",
                     what, s, key0, (long long)key0 + NC, NKEYS);
        n_out += (long long)nW * NC;
        n_rows += nW;
        longest = nW > longest ? nW : longest;
        SIDE_REQUIRE(n_out <= MAX_32, "%s: the table's counts are too large for one launch (row %d)", what, s);
    }
    SIDE_REQUIRE(n_out == NOUT, "%s: the table's nW * NC sum to %lld, not to NOUT=%d", what, n_out, NOUT);
    if (NOUT == 0) return 0;                                                   // no session completed a window: nothing to do
    const uintptr_t a = (uintptr_t)scores, b = (uintptr_t)out, bytes = (uintptr_t)NOUT * sizeof(float);
    SIDE_REQUIRE(a + bytes <= b || b + bytes <= a, "%s: out overlaps scores (the plane would be read as it is written)", what);
    const unsigned gy = (unsigned)(longest < MAX_GRID_Y ? longest : MAX_GRID_Y);     // a longer row: its workgroups take several windows
    hipLaunchKernelGGL(contest_kernel, dim3((unsigned)S, gy), dim3(WG), 0, static_cast<hipStream_t>(stream), scores, keys, out, leaders,
                       n_leaders, work, table_dev, (unsigned)NOUT, (unsigned)(keys ? NKEYS : 0), (unsigned)n_rows, (unsigned)(keys ? cap : 0),
                       (unsigned)top, Margin{has_margin != 0, margin});
    return check_launch(what);
}
