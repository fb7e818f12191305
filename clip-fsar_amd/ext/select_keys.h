// The threshold select that shortlist.hip (select_kernel) and pool_select.hip (select_pinned_kernel) share, one copy: a group's scores as
// order-preserving 32-bit keys, the K-th largest key by four radix passes over per-wave histograms in LDS, and the scan that compacts the
// columns above the threshold and the first few equal to it in ascending column order.  One 256-thread workgroup per group calls these,
// every thread of it; nothing here waits on another workgroup, and a place is a prefix sum, never the outcome of a race.
// What a kernel brings of its own: where the keys lie (`keys`, NC of them), how a histogram cell is bumped (`count`: the one atomic, on
// LDS, whose sums do not depend on their order) and what a selected column writes (`put`).
#pragma once
#include <stdint.h>

namespace {

constexpr int SEL_WG = 256, SEL_WAVES = SEL_WG / 64;

// a group score as a key that orders as the floats do: larger float, larger key; -0.0 folded into +0.0; 0 = not selectable (no score,
// or -inf, whose key would be 0x007fffff: every selectable key is at least 0x00800000, that of -FLT_MAX, and at most 0xff800000, +inf's)
__device__ __forceinline__ unsigned score_key(float v, bool any) {
    if (!any || !(v > -__builtin_inff())) return 0u;
    const unsigned u = v == 0.0f ? 0u : __float_as_uint(v);                   // both zeros: the bits of +0.0
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// the key of column c of a group: the maximum of S[q, c] over the group's nq queries from q_first on, NaN ignored (coalesced at every q
// when adjacent threads take adjacent columns)
__device__ __forceinline__ unsigned group_score_key(const float* __restrict__ S, int q_first, int nq, int NC, int c) {
    float best = -__builtin_inff();
    bool any = false;
    for (int q = 0; q < nq; ++q) {
        const float v = S[(size_t)(q_first + q) * NC + c];
        if (v == v) {
            best = any ? fmaxf(best, v) : v;
            any = true;
        }
    }
    return score_key(best, any);
}

// exclusive prefix of a flag over the workgroup's threads in thread order, and the workgroup's total: a ballot per wave, the waves'
// counts through LDS.  Every thread calls it; `part` is SEL_WAVES ints, free to be rewritten after the call's second barrier.
__device__ __forceinline__ unsigned block_prefix(bool flag, unsigned* part, unsigned& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long m = __ballot(flag);
    if (lane == 0) part[wave] = (unsigned)__popcll(m);
    __syncthreads();
    unsigned before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < SEL_WAVES; ++w) {
        const unsigned n = part[w];
        before += w < wave ? n : 0u;
        all += n;
    }
    __syncthreads();
    total = all;
    return before + (unsigned)__popcll(m & ((1ull << lane) - 1ull));
}

// The K-th largest of keys[0 .. NC), 1 <= K <= NC, a byte per pass from the top: of the keys that share the bytes found so far, count the
// next byte's values, then walk the counts from 255 down until `left` of them are covered.  hist: SEL_WAVES * 256 counters in LDS, a
// histogram per wave; pick: 2 words in LDS; count(cell) adds one to hist[cell].  -> the key; `left` of the keys equal to it are kept.
// The keys must be visible to the workgroup (a barrier behind their writes); the call ends on a barrier.
template <class Count>
__device__ __forceinline__ unsigned kth_largest_key(const unsigned* keys, int NC, unsigned K, unsigned* hist, unsigned* pick, Count count,
                                                    unsigned& left) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned prefix = 0;
    left = K;
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        const unsigned mask = pass ? 0xffffffffu << (shift + 8) : 0u;
        for (int i = tid; i < SEL_WAVES * 256; i += SEL_WG) hist[i] = 0;
        __syncthreads();
        for (int c = tid; c < NC; c += SEL_WG) {
            const unsigned k = keys[c];
            if ((k & mask) == prefix) count(wave * 256 + ((k >> shift) & 255u));
        }
        __syncthreads();
        if (wave == 0) {                                                      // lane l owns the values 4 l .. 4 l + 3
            unsigned s[4], mine = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                s[j] = 0;
#pragma unroll
                for (int w = 0; w < SEL_WAVES; ++w) s[j] += hist[w * 256 + 4 * lane + j];
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
                if (above < left && incl >= left) {                           // exactly one (lane, j): left >= 1, and K <= NC keys exist
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

// Compaction in ascending column order, SEL_WG columns at a time: the columns whose key is above thr, and the first need_eq of those equal
// to it (thr = 0 keeps nothing equal: 0 is "not selectable").  put(place, column) is called once per kept column, place < K, by the
// column's thread.  -> the number of places filled (uniform); the caller pads the rest.
template <class Put>
__device__ __forceinline__ unsigned compact_selected(const unsigned* keys, int NC, unsigned K, unsigned thr, unsigned need_eq, unsigned* part,
                                                     Put put) {
    const int tid = threadIdx.x;
    unsigned n_eq = 0, n_out = 0;                                             // equal keys seen, places written: uniform
    for (int c0 = 0; c0 < NC; c0 += SEL_WG) {
        const int c = c0 + tid;
        const unsigned k = c < NC ? keys[c] : 0u;
        const bool gt = k > thr, eq = thr && k == thr;
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

}  // namespace
