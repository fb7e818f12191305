// The peak search of a stream pool with a history (libclipfsar_history.so, C ABI in include/ext/clipfsar_history.h): a score plane
// [windows, classes] over the windows a history store still holds -> per class the best occurrences that do not overlap.  The table is
// the pool's (pool.hip), the very rows the gather of those windows was given; only NW and WIN_OFF are read.
// history_peaks_kernel is a local-maximum filter per (session row, class): a tile of 256 windows plus `separation` windows of halo on
// each side, clipped to the row, staged in LDS as order-preserving keys; a window is a peak when no staged neighbour within the
// distance beats it -- a higher key, or an equal key at a lower window.  It writes the peak's key, or 0, TRANSPOSED: work[k, n], so
// that history_hits_kernel, one workgroup per class, reads its class contiguously.  That kernel is the threshold select of
// select_keys.h, which shortlist.hip, pool_select.hip and (restated) contest.hip run: the top-th largest key by four radix passes
// over per-wave histograms in LDS, then a scan that compacts the rows above the threshold and the first few equal to it in ascending
// row order.  It is RESTATED here, not included: the build's staleness matrix pins select_keys.h to exactly two libraries
// (tests/test_pool_select_abi.py), and a further includer would change what an edit of that header rebuilds.  The key, the tie rule
// and the order are the header's; tests/test_history_abi.py holds the working lines to the header's line for line, and
// tests/test_gpu_history.py holds both kernels to clip_fsar_amd.history.reference_search bit for bit.
// No workgroup waits on another, a hit's place is a prefix sum, and the one atomic is the histogram count in LDS, whose sums do not
// depend on their order.  The search keeps no state.
// A plug-in library (build.py, PLUGIN_LIBS): it lives beside csrc/, whose files and export sets stay as they are.
#include "../csrc/side_lib.h"
#include "../../include/ext/clipfsar_history.h"

#include <math.h>

namespace {

constexpr int COLS = CFHS_TABLE_COLS;
constexpr int SEL_WG = 256, SEL_WAVES = SEL_WG / 64;
constexpr int TILE = SEL_WG;
constexpr long long MAX_PLANE = 1LL << 30;          // scores of a plane: the kernels' 32-bit window loops step past its end by less than 2^30
constexpr unsigned MAX_GRID_Y = 65535;

// a score as a key that orders as the floats do: larger float, larger key; -0.0 folded into +0.0; 0 = no candidate (not `any`, NaN, or
// -inf, whose key would be 0x007fffff: every candidate's key is at least 0x00800000, that of -FLT_MAX, and at most 0xff800000, +inf's)
__device__ __forceinline__ unsigned score_key(float v, bool any) {
    if (!any || !(v > -__builtin_inff())) return 0u;
    const unsigned u = v == 0.0f ? 0u : __float_as_uint(v);                   // both zeros: the bits of +0.0
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// exclusive prefix of a flag over the workgroup's threads in thread order, and the workgroup's total: a ballot per wave, the waves'
// counts through LDS.  Every thread calls it; `part` is SEL_WAVES words, free to be rewritten after the call's second barrier.
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

// The K-th largest of keys[0 .. NC), 1 <= K <= the number of keys above 0, a byte per pass from the top: of the keys that share the bytes
// found so far, count the next byte's values (a histogram per wave, the one atomic), then walk the counts from 255 down until `left` of
// them are covered.  hist: SEL_WAVES * 256 counters in LDS; pick: 2 words in LDS.  -> the key; `left` of the keys equal to it are kept.
// The keys must be visible to the workgroup (a launch or a barrier behind their writes); the call ends on a barrier.
__device__ __forceinline__ unsigned kth_largest_key(const unsigned* keys, int NC, unsigned K, unsigned* hist, unsigned* pick, unsigned& left) {
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
            if ((k & mask) == prefix) atomicAdd(&hist[wave * 256 + ((k >> shift) & 255u)], 1u);
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
                if (above < left && incl >= left) {                           // exactly one (lane, j): left >= 1, and K peaks exist
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

// Compaction in ascending row order, SEL_WG rows at a time: the rows whose key is above thr, and the first need_eq of those equal to
// it (thr = 0 keeps nothing equal: 0 is "no peak").  put(place, row) is called once per kept row, place < K, by the row's thread.
// -> the number of places filled (uniform); the caller pads the rest.
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

// sum of n over the workgroup, to every thread: the waves' lanes by shuffles, the waves through LDS.  Every thread calls it; `red` is
// SEL_WAVES words.  It ends on a barrier.
__device__ __forceinline__ unsigned block_sum(unsigned n, unsigned* red) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) n += (unsigned)__shfl_down(n, o, 64);    // lane 0 ends with the wave's: lane l < o takes lane l + o
    if (lane == 0) red[wave] = n;
    __syncthreads();
    n = 0;
#pragma unroll
    for (int w = 0; w < SEL_WAVES; ++w) n += red[w];
    __syncthreads();
    return n;
}

struct MinScore {
    int has;
    float value;
};

// One workgroup per (table row, tile of TILE windows, class): blockIdx.x the row, blockIdx.y the row's tiles (a longer row: its
// workgroups take several), blockIdx.z the class.
__global__ __launch_bounds__(SEL_WG) void history_peaks_kernel(const float* __restrict__ scores, unsigned* __restrict__ work,
                                                              const int32_t* __restrict__ table, unsigned NW, unsigned K, int sep,
                                                              MinScore ms) {
    extern __shared__ unsigned tile[];                                        // TILE + 2 sep keys: the windows lo .. hi - 1 of the row
    const int tid = threadIdx.x;
    const int32_t* d = table + (size_t)blockIdx.x * COLS;
    const long long nW = d[CFHS_NW], off = d[CFHS_WIN_OFF];
    // a device table that is not the validated host rows: the row touches nothing
    if (nW <= 0 || off < 0 || off + nW > (long long)NW) return;
    const unsigned k = blockIdx.z;
    const int n = (int)nW;
    for (int j0 = (int)blockIdx.y * TILE; j0 < n; j0 += (int)gridDim.y * TILE) {        // (uniform: every thread meets the barriers)
        const int lo = max(j0 - sep, 0), hi = (int)min((long long)j0 + TILE + sep, nW);
        for (int v = lo + tid; v < hi; v += SEL_WG) {
            const float s = scores[((size_t)off + (size_t)v) * K + k];
            tile[v - lo] = score_key(s, !ms.has || s >= ms.value);
        }
        __syncthreads();
        const int j = j0 + tid;
        if (j < n) {
            const unsigned mine = tile[j - lo];
            bool peak = mine != 0u;
            const int a = max(j - sep, 0), b = min(j + sep, n - 1);         // lo <= a and b < hi: the halo covers them
            for (int v = a; v < j && peak; ++v) peak = tile[v - lo] < mine;   // an earlier window beats it with an equal key too
            for (int v = j + 1; v <= b && peak; ++v) peak = tile[v - lo] <= mine;
            work[(size_t)k * NW + (size_t)off + (size_t)j] = peak ? mine : 0u;
        }
        __syncthreads();                                                      // the tile is rewritten by the next round
    }
}

// One workgroup per class: keys = work[k, 0 .. NW), written by the launch before this one.
__global__ __launch_bounds__(SEL_WG) void history_hits_kernel(const float* __restrict__ scores, const unsigned* __restrict__ work,
                                                             int32_t* __restrict__ hit_rows, float* __restrict__ hit_scores,
                                                             int32_t* __restrict__ n_hits, int32_t* __restrict__ n_peaks, unsigned NW,
                                                             unsigned K, unsigned top) {
    __shared__ unsigned hist[SEL_WAVES * 256];                                // a histogram per wave
    __shared__ unsigned part[SEL_WAVES];
    __shared__ unsigned pick[2];                                              // the pass's digit, and what is left of R below it
    __shared__ unsigned red[SEL_WAVES];
    const int tid = threadIdx.x;
    const unsigned k = blockIdx.x;
    const unsigned* keys = work + (size_t)k * NW;
    const int nc = (int)NW;
    unsigned mine = 0;
    for (int c = tid; c < nc; c += SEL_WG) mine += keys[c] != 0u;
    const unsigned peaks = block_sum(mine, red);
    const unsigned R = min(top, peaks);
    int32_t* rows = hit_rows + (size_t)k * top;
    float* vals = hit_scores + (size_t)k * top;
    unsigned n_out = 0;
    if (R) {
        unsigned need_eq = 0;
        const unsigned thr = kth_largest_key(keys, nc, R, hist, pick, need_eq);
        n_out = compact_selected(keys, nc, R, thr, need_eq, part, [&](unsigned place, int c) {
            rows[place] = c;
            vals[place] = scores[(size_t)c * K + k];                          // the plane's bits, not the key's: -0.0 stays -0.0
        });
    }
    for (unsigned r = n_out + tid; r < top; r += SEL_WG) {
        rows[r] = CFHS_NONE;
        vals[r] = 0.0f;
    }
    if (tid == 0) {
        n_hits[k] = (int32_t)n_out;
        n_peaks[k] = (int32_t)peaks;
    }
}

bool overlap(const void* a, long long a_bytes, const void* b, long long b_bytes) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return !(x + (uintptr_t)a_bytes <= y || y + (uintptr_t)b_bytes <= x);
}

}  // namespace

extern "C" int cfhs_version(void) { return 100; /* 0.1.0 */ }
extern "C" int cfhs_abi_version(void) { return CFHS_ABI_VERSION; }
extern "C" const char* cfhs_last_error(void) { return g_err; }

extern "C" int cfhs_workspace_words(int NW, int K) {
    if (NW < 0 || K < 1 || (long long)NW * K > MAX_PLANE) return -1;
    return (int)((long long)NW * K);
}

extern "C" int cfhs_peaks(const float* scores, uint32_t* work, int32_t* hit_rows, float* hit_scores, int32_t* n_hits, int32_t* n_peaks,
                          const int32_t* table_host, const int32_t* table_dev, int S, int NW, int K, int separation, int has_min,
                          float min_score, int top, cfhs_stream_t stream) {
    const char* what = "cfhs_peaks";
    SIDE_REQUIRE(scores && work && hit_rows && hit_scores && n_hits && n_peaks && table_host && table_dev,
                 "%s: null pointer (scores, work, hit_rows, hit_scores, n_hits, n_peaks, table_host or table_dev)", what);
    SIDE_REQUIRE(S >= 1 && S <= CFHS_MAX_STREAMS, "%s: a table of S=%d rows (1 .. %d)", what, S, CFHS_MAX_STREAMS);
    SIDE_REQUIRE(NW >= 0, "%s: bad shape (NW=%d)", what, NW);
    SIDE_REQUIRE(K >= 1 && K <= CFHS_MAX_CLASSES, "%s: K=%d classes (1 .. %d)", what, K, CFHS_MAX_CLASSES);
    SIDE_REQUIRE((long long)NW * K <= MAX_PLANE, "%s: a plane of NW=%d x K=%d scores is too large for one launch (2^30 at most)", what, NW, K);
    SIDE_REQUIRE(top >= 1 && top <= CFHS_MAX_TOP, "%s: top=%d outside 1 .. %d", what, top, CFHS_MAX_TOP);
    SIDE_REQUIRE(separation >= 0 && separation <= CFHS_MAX_SEPARATION, "%s: separation=%d outside 0 .. %d", what, separation,
                 CFHS_MAX_SEPARATION);
    SIDE_REQUIRE(!has_min || !isnan(min_score), "%s: min_score is NaN (no score is at least NaN)", what);
    long long win = 0, longest = 0;
    for (int s = 0; s < S; ++s) {
        const int32_t* d = table_host + (size_t)s * COLS;
        const int nW = d[CFHS_NW];
        SIDE_REQUIRE(nW >= 0, "%s: row %d has a negative count (nW=%d)", what, s, nW);
        SIDE_REQUIRE(d[CFHS_WIN_OFF] == win, "%s: row %d has WIN_OFF=%d, the nW of the rows before it add up to %lld", what, s,
                     d[CFHS_WIN_OFF], win);
        win += nW;
        longest = nW > longest ? nW : longest;
        SIDE_REQUIRE(win <= MAX_PLANE, "%s: the table's counts are too large for one launch (row %d)", what, s);
    }
    SIDE_REQUIRE(win == NW, "%s: the table's nW sum to %lld, not to NW=%d", what, win, NW);
    if (NW == 0) return 0;                                                     // no held window: nothing to do
    const long long plane = (long long)NW * K * 4, hits = (long long)K * top * 4, per_class = (long long)K * 4;
    SIDE_REQUIRE(!overlap(work, plane, scores, plane), "%s: work overlaps scores (the plane would be overwritten as it is read)", what);
    SIDE_REQUIRE(!overlap(work, plane, hit_rows, hits) && !overlap(work, plane, hit_scores, hits) &&
                     !overlap(work, plane, n_hits, per_class) && !overlap(work, plane, n_peaks, per_class),
                 "%s: work overlaps an output (hit_rows, hit_scores, n_hits or n_peaks)", what);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t lds = (size_t)(TILE + 2 * separation) * sizeof(unsigned);   // at most 33 KB, separation <= 4096
    const long long tiles = (longest + TILE - 1) / TILE;
    const unsigned gy = (unsigned)(tiles < MAX_GRID_Y ? tiles : MAX_GRID_Y);   // a longer row: its workgroups take several tiles
    hipLaunchKernelGGL(history_peaks_kernel, dim3((unsigned)S, gy, (unsigned)K), dim3(SEL_WG), lds, st, scores, work, table_dev, (unsigned)NW,
                       (unsigned)K, separation, MinScore{has_min != 0, min_score});
    if (check_launch(what)) return 1;
    hipLaunchKernelGGL(history_hits_kernel, dim3((unsigned)K), dim3(SEL_WG), 0, st, scores, work, hit_rows, hit_scores, n_hits, n_peaks,
                       (unsigned)NW, (unsigned)K, (unsigned)top);
    return check_launch(what);
}
