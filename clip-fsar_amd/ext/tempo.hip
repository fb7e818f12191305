// Tempo windows of a stream pool (libclipfsar_tempo.so, C ABI in include/ext/clipfsar_tempo.h): every window of a push read at R frame
// rates out of the pool's ring, and the reduction of the R scores of a (window, class) cell to their maximum and the tempo that gave it.
// The gather has the shape of pool.hip's window gather: one WAVE per destination row, the row's session found by a wave-uniform binary
// search over the table's WIN_OFF prefix offsets (scalar loads), the lanes striding over the row's 16-byte pieces.  The rates travel by
// value in the kernel arguments (a struct of CFTP_MAX_RATES ints): there is no device list to upload or to keep alive.
// The reduction is one thread per four consecutive classes of a window (one class when the row width or a base does not allow 16-byte
// accesses): R row loads into registers, a compare chain, one store of the score and one of the tempo.  Memory-bound by construction.
// Both kernels are plain C++, every cell has exactly one writer (two runs write identical bytes), no workgroup waits on another.
// find_row and check_table live in pool.hip's anonymous namespace; csrc/ takes no new file and ring_rows.h must not learn the pool's
// header, so both are RESTATED here -- same search, same checks, same wording after the function's name.
// A plug-in library (build.py, PLUGIN_LIBS): it lives beside csrc/, whose files and export sets stay as they are.
#include "../csrc/ring_rows.h"
#include "../csrc/side_lib.h"
#include "../../include/clipfsar_pool.h"
#include "../../include/ext/clipfsar_tempo.h"

namespace {

constexpr int THREADS = 256;
constexpr int WAVE = 64;
constexpr int WAVES = THREADS / WAVE;
constexpr int COLS = CFSP_TABLE_COLS;

struct Rates {
    int r[CFTP_MAX_RATES];
};

// pool.hip's find_row, restated: the last table row whose prefix offset in column `col` is <= r (offsets start at 0 and never decrease;
// rows with a count of 0 share their offset with the row after them and are passed over).  Everything here is wave-uniform.
__device__ __forceinline__ const int* find_row(const int* __restrict__ table, unsigned S, int col, unsigned r) {
    unsigned lo = 0, hi = S;                   // table[lo][col] <= r; hi == S or table[hi][col] > r
    while (hi - lo > 1) {
        const unsigned mid = (lo + hi) >> 1;
        if ((unsigned)table[mid * COLS + col] <= r) lo = mid;
        else hi = mid;
    }
    return table + lo * COLS;
}

__device__ __forceinline__ unsigned wave_id() { return __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE); }

// rates.r[i], i wave-uniform and below R <= 8: a select chain over the by-value struct, so that nothing is indexed in memory
__device__ __forceinline__ unsigned rate_of(const Rates& rates, unsigned i) {
    unsigned v = (unsigned)rates.r[0];
#pragma unroll
    for (int k = 1; k < CFTP_MAX_RATES; ++k) v = i == (unsigned)k ? (unsigned)rates.r[k] : v;
    return v;
}

// ---- tempo gather.  Row r of X is frame j of tempo i of window g = w0 + r / (R T) of the packed window list; g belongs to the session
// whose win_off is the last one <= g, as its window w = g - win_off: ring position
// (win_pos + w * stride + (T - 1) * (rmax - rate_i) + j * rate_i) mod cap.  The host checked that w * stride + (T - 1) * rmax < cap for
// every window of a row and that win_pos < cap, and (T - 1) * (rmax - rate_i) + j * rate_i <= (T - 1) * rmax: the sum stays below 2 cap.
template <bool VEC>
__global__ __launch_bounds__(THREADS) void tempo_gather_kernel(const float* __restrict__ ring, float* __restrict__ X,
                                                               const int* __restrict__ table, unsigned S, unsigned rows, unsigned w0,
                                                               unsigned T, unsigned R, unsigned pieces, unsigned cap, unsigned stride,
                                                               unsigned rmax, Rates rates) {
    typedef typename Piece<VEC>::type P;
    const unsigned lane = threadIdx.x % WAVE;
    for (unsigned r = blockIdx.x * WAVES + wave_id(); r < rows; r += gridDim.x * WAVES) {
        const unsigned gt = r / T, j = r - gt * T;             // (window, tempo) pair and frame
        const unsigned gw = gt / R, i = gt - gw * R, g = w0 + gw;
        const unsigned rate = rate_of(rates, i);
        const int* d = find_row(table, S, CFSP_WIN_OFF, g);
        const unsigned pos = ((unsigned)d[CFSP_WIN_POS] + (g - (unsigned)d[CFSP_WIN_OFF]) * stride + (T - 1) * (rmax - rate) + j * rate) % cap;
        const P* src = reinterpret_cast<const P*>(ring) + ((size_t)d[CFSP_SLOT] * cap + pos) * pieces;
        P* dst = reinterpret_cast<P*>(X) + (size_t)r * pieces;
        for (unsigned p = lane; p < pieces; p += WAVE) dst[p] = src[p];
    }
}

// ---- tempo reduction.  One cell: `best` starts as tempo 0's score; a later score replaces it when it is larger, or when it is a NaN,
// and nothing replaces a NaN -- so the first NaN wins, otherwise the largest score at its lowest index.  Selection only: `best` is one
// of the inputs bit for bit.
__device__ __forceinline__ void take(float v, int i, float& best, int& at) {
    const bool held = best != best;                            // a NaN is kept
    const bool better = !held && (v > best || v != v);
    best = better ? v : best;
    at = better ? i : at;
}

// VEC: item = (window w, class quad q) of C / 4 quads; otherwise (window w, class c).  `cols` = quads or classes per row.
template <bool VEC>
__global__ __launch_bounds__(THREADS) void tempo_reduce_kernel(const float* __restrict__ scores, float* __restrict__ out,
                                                               int* __restrict__ tempo, unsigned items, unsigned R, unsigned cols) {
    typedef typename Piece<VEC>::type P;
    for (unsigned idx = blockIdx.x * THREADS + threadIdx.x; idx < items; idx += gridDim.x * THREADS) {
        const unsigned w = idx / cols, c = idx - w * cols;
        const P* src = reinterpret_cast<const P*>(scores) + (size_t)w * R * cols + c;
        P v[CFTP_MAX_RATES];
#pragma unroll
        for (int i = 0; i < CFTP_MAX_RATES; ++i)               // the R row loads, all issued before the first compare
            if ((unsigned)i < R) v[i] = src[(size_t)i * cols];
        if constexpr (VEC) {
            float4 best = v[0];
            int4 at = make_int4(0, 0, 0, 0);
#pragma unroll
            for (int i = 1; i < CFTP_MAX_RATES; ++i)
                if ((unsigned)i < R) {
                    take(v[i].x, i, best.x, at.x);
                    take(v[i].y, i, best.y, at.y);
                    take(v[i].z, i, best.z, at.z);
                    take(v[i].w, i, best.w, at.w);
                }
            reinterpret_cast<float4*>(out)[idx] = best;
            reinterpret_cast<int4*>(tempo)[idx] = at;
        } else {
            float best = v[0];
            int at = 0;
#pragma unroll
            for (int i = 1; i < CFTP_MAX_RATES; ++i)
                if ((unsigned)i < R) take(v[i], i, best, at);
            out[idx] = best;
            tempo[idx] = at;
        }
    }
}

// pool.hip's check_table, restated: the host copy of the table, before any device work.  N / NW < 0: that total is not checked.
int check_table(const char* what, const int32_t* t, int S, int max_streams, int cap, long long N, long long NW) {
    SIDE_REQUIRE(max_streams >= 1 && max_streams <= CFSP_MAX_STREAMS, "%s: max_streams=%d outside 1 .. %d", what, max_streams,
                 CFSP_MAX_STREAMS);
    SIDE_REQUIRE(S >= 1 && S <= max_streams, "%s: a table of S=%d rows for max_streams=%d", what, S, max_streams);
    SlotBits seen(max_streams);
    SIDE_REQUIRE(seen.ok(), "%s: out of host memory for %d slots", what, max_streams);
    long long feat = 0, win = 0;
    for (int s = 0; s < S; ++s) {
        const int32_t* d = t + (size_t)s * COLS;
        const int slot = d[CFSP_SLOT];
        SIDE_REQUIRE(slot >= 0 && slot < max_streams, "%s: row %d has slot %d outside 0 .. %d", what, s, slot, max_streams - 1);
        SIDE_REQUIRE(!seen.test_and_set(slot), "%s: slot %d appears twice in the table (row %d)", what, slot, s);
        SIDE_REQUIRE(d[CFSP_N] >= 0 && d[CFSP_NW] >= 0, "%s: row %d has a negative count (n=%d nW=%d)", what, s, d[CFSP_N], d[CFSP_NW]);
        SIDE_REQUIRE(d[CFSP_PUT_POS] >= 0 && d[CFSP_WIN_POS] >= 0 && (cap == 0 || (d[CFSP_PUT_POS] < cap && d[CFSP_WIN_POS] < cap)),
                     "%s: row %d has a ring position outside 0 .. cap-1 (put_pos=%d win_pos=%d cap=%d)", what, s, d[CFSP_PUT_POS],
                     d[CFSP_WIN_POS], cap);
        SIDE_REQUIRE(cap == 0 || d[CFSP_N] <= cap, "%s: row %d: n=%d frames do not fit a ring of cap=%d", what, s, d[CFSP_N], cap);
        SIDE_REQUIRE(d[CFSP_FEAT_OFF] == feat && d[CFSP_WIN_OFF] == win,
                     "%s: row %d has offsets (%d, %d), the prefix sums of the counts are (%lld, %lld)", what, s, d[CFSP_FEAT_OFF],
                     d[CFSP_WIN_OFF], feat, win);
        SIDE_REQUIRE(d[CFSP_HAS_STATE] == 0 || d[CFSP_HAS_STATE] == 1, "%s: row %d has has_state=%d, not 0 or 1", what, s, d[CFSP_HAS_STATE]);
        feat += d[CFSP_N];
        win += d[CFSP_NW];
        SIDE_REQUIRE(feat <= MAX_ITEMS && win <= MAX_ITEMS, "%s: the table's counts are too large for one launch (row %d)", what, s);
    }
    SIDE_REQUIRE(N < 0 || feat == N, "%s: the table's n sum to %lld, not to N=%lld", what, feat, N);
    SIDE_REQUIRE(NW < 0 || win == NW, "%s: the table's nW sum to %lld, not to NW=%lld", what, win, NW);
    return 0;
}

// do the byte ranges [a, a + na) and [b, b + nb) share a byte?
bool overlap(const void* a, long long na, const void* b, long long nb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + (uintptr_t)nb && b0 < a0 + (uintptr_t)na;
}

}  // namespace

extern "C" int cftp_version(void) { return 100; /* 0.1.0 */ }
extern "C" int cftp_abi_version(void) { return CFTP_ABI_VERSION; }
extern "C" const char* cftp_last_error(void) { return g_err; }

extern "C" int cftp_window_sequences(const float* ring, float* X, const int32_t* table_host, const int32_t* table_dev, int S, int NW, int w0,
                                     int w1, int T, int E, int max_streams, int cap, int stride, const int32_t* rates_host, int R,
                                     cftp_stream_t stream) {
    SIDE_REQUIRE(ring && X && table_host && table_dev && rates_host, "cftp_window_sequences: null pointer");
    SIDE_REQUIRE(NW > 0 && E > 0 && cap > 0, "cftp_window_sequences: bad shape (NW=%d E=%d cap=%d)", NW, E, cap);
    SIDE_REQUIRE(T >= 1 && T <= CFSP_MAX_T, "cftp_window_sequences: T=%d outside 1 .. %d", T, CFSP_MAX_T);
    SIDE_REQUIRE(stride >= 1, "cftp_window_sequences: stride=%d must be at least 1", stride);
    SIDE_REQUIRE(R >= 1 && R <= CFTP_MAX_RATES, "cftp_window_sequences: R=%d rates outside 1 .. %d", R, CFTP_MAX_RATES);
    Rates rates;
    for (int i = 0; i < CFTP_MAX_RATES; ++i) rates.r[i] = i < R ? rates_host[i] : 0;
    SIDE_REQUIRE(rates.r[0] >= 1, "cftp_window_sequences: rates[0]=%d must be at least 1", rates.r[0]);
    for (int i = 1; i < R; ++i)
        SIDE_REQUIRE(rates.r[i] > rates.r[i - 1], "cftp_window_sequences: rates[%d]=%d after rates[%d]=%d, the rates must be strictly ascending",
                     i, rates.r[i], i - 1, rates.r[i - 1]);
    const int rmax = rates.r[R - 1];
    SIDE_REQUIRE(0 <= w0 && w0 < w1 && w1 <= NW, "cftp_window_sequences: window range [%d, %d) outside 0 .. NW=%d", w0, w1, NW);
    if (check_table("cftp_window_sequences", table_host, S, max_streams, cap, -1, NW)) return 1;
    for (int s = 0; s < S; ++s) {
        const int nW = table_host[(size_t)s * COLS + CFSP_NW];
        const long long span = (long long)(nW - 1) * stride + (long long)(T - 1) * rmax + 1;
        SIDE_REQUIRE(nW == 0 || span <= cap, "cftp_window_sequences: row %d: the %lld frames of nW=%d windows do not fit a ring of cap=%d", s,
                     span, nW, cap);
    }
    const bool vec = vec_ok(ring, X, E);
    const long long pieces = vec ? E / 4 : E;
    const long long rows = (long long)(w1 - w0) * R * T;
    SIDE_REQUIRE(rows * pieces <= MAX_ITEMS && (long long)max_streams * cap * pieces <= MAX_ITEMS,
                 "cftp_window_sequences: too large for one launch (windows=%d R=%d T=%d E=%d max_streams=%d cap=%d)", w1 - w0, R, T, E,
                 max_streams, cap);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (vec)
        hipLaunchKernelGGL(tempo_gather_kernel<true>, dim3(blocks_for(rows, WAVES)), dim3(THREADS), 0, s, ring, X, table_dev, (unsigned)S,
                           (unsigned)rows, (unsigned)w0, (unsigned)T, (unsigned)R, (unsigned)pieces, (unsigned)cap, (unsigned)stride,
                           (unsigned)rmax, rates);
    else
        hipLaunchKernelGGL(tempo_gather_kernel<false>, dim3(blocks_for(rows, WAVES)), dim3(THREADS), 0, s, ring, X, table_dev, (unsigned)S,
                           (unsigned)rows, (unsigned)w0, (unsigned)T, (unsigned)R, (unsigned)pieces, (unsigned)cap, (unsigned)stride,
                           (unsigned)rmax, rates);
    return check_launch("cftp_window_sequences");
}

extern "C" int cftp_reduce(const float* scores, float* out, int32_t* tempo, int NW, int R, int C, cftp_stream_t stream) {
    SIDE_REQUIRE(scores && out && tempo, "cftp_reduce: null pointer");
    SIDE_REQUIRE(NW > 0 && C > 0, "cftp_reduce: bad shape (NW=%d C=%d)", NW, C);
    SIDE_REQUIRE(R >= 1 && R <= CFTP_MAX_RATES, "cftp_reduce: R=%d rates outside 1 .. %d", R, CFTP_MAX_RATES);
    const long long cells = (long long)NW * C;
    SIDE_REQUIRE(cells * R <= MAX_ITEMS, "cftp_reduce: too large for one launch (NW=%d R=%d C=%d)", NW, R, C);
    SIDE_REQUIRE(!overlap(scores, cells * R * 4, out, cells * 4), "cftp_reduce: out overlaps scores -- the reduction is not done in place, give it a buffer of its own");
    SIDE_REQUIRE(!overlap(scores, cells * R * 4, tempo, cells * 4) && !overlap(out, cells * 4, tempo, cells * 4),
                 "cftp_reduce: tempo overlaps scores or out -- give it a buffer of its own");
    const bool vec = C % 4 == 0 && (((uintptr_t)scores | (uintptr_t)out | (uintptr_t)tempo) & 15u) == 0;
    const long long cols = vec ? C / 4 : C, items = (long long)NW * cols;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (vec)
        hipLaunchKernelGGL(tempo_reduce_kernel<true>, dim3(blocks_for(items, THREADS)), dim3(THREADS), 0, s, scores, out, tempo,
                           (unsigned)items, (unsigned)R, (unsigned)cols);
    else
        hipLaunchKernelGGL(tempo_reduce_kernel<false>, dim3(blocks_for(items, THREADS)), dim3(THREADS), 0, s, scores, out, tempo,
                           (unsigned)items, (unsigned)R, (unsigned)cols);
    return check_launch("cftp_reduce");
}
