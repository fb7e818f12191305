// Stream pool (libclipfsar_pool.so, C ABI in include/clipfsar_pool.h): the ring write, the window gather and the smoothing recurrence of
// window-stream sessions that join, leave and push unevenly.  stream.hip serves B lockstep streams from one (B, n, first_frame) triple;
// here a push is a descriptor table with one int32 row per session, and the kernels find a row's session in it.
// Copy kernels: one WAVE per destination row.  The row number is wave-uniform, so the search over the table's prefix offsets runs once
// per row on scalar values (the table loads are scalar loads) and the lanes then stride over the row's 16-byte pieces.
// A library of its own: the other four keep their pinned export sets.
#include "ring_rows.h"
#include "side_lib.h"
#include "../../include/clipfsar_pool.h"

namespace {

constexpr int THREADS = 256;
constexpr int WAVE = 64;
constexpr int WAVES = THREADS / WAVE;
constexpr int COLS = CFSP_TABLE_COLS;

// the last table row whose prefix offset in column `col` is <= r (offsets start at 0 and never decrease; rows with a count of 0 share
// their offset with the row after them and are passed over).  Everything here is wave-uniform.
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

// ---- ring write.  Packed row r belongs to the session whose feat_off is the last one <= r; its ring position is put_pos + (r - feat_off),
// wrapped once (n <= cap)
template <bool VEC>
__global__ __launch_bounds__(THREADS) void pool_ring_put_kernel(const float* __restrict__ feats, float* __restrict__ ring,
                                                                const int* __restrict__ table, unsigned S, unsigned N, unsigned pieces,
                                                                unsigned cap) {
    typedef typename Piece<VEC>::type P;
    const unsigned lane = threadIdx.x % WAVE;
    for (unsigned r = blockIdx.x * WAVES + wave_id(); r < N; r += gridDim.x * WAVES) {
        const int* d = find_row(table, S, CFSP_FEAT_OFF, r);
        unsigned pos = (unsigned)d[CFSP_PUT_POS] + (r - (unsigned)d[CFSP_FEAT_OFF]);          // < 2 cap
        if (pos >= cap) pos -= cap;
        const P* src = reinterpret_cast<const P*>(feats) + (size_t)r * pieces;
        P* dst = reinterpret_cast<P*>(ring) + ((size_t)d[CFSP_SLOT] * cap + pos) * pieces;
        for (unsigned p = lane; p < pieces; p += WAVE) dst[p] = src[p];
    }
}

// ---- window gather.  Row r of X is frame j = r mod T of window g = w0 + r / T of the packed window list; g belongs to the session whose
// win_off is the last one <= g, as its window w = g - win_off: ring position (win_pos + w * stride + j * rate) mod cap (the host checked
// that a row's windows span at most cap positions, so the sum stays below 2 cap)
template <bool VEC>
__global__ __launch_bounds__(THREADS) void pool_window_sequences_kernel(const float* __restrict__ ring, float* __restrict__ X,
                                                                        const int* __restrict__ table, unsigned S, unsigned rows, unsigned w0,
                                                                        unsigned T, unsigned pieces, unsigned cap, unsigned stride,
                                                                        unsigned rate) {
    typedef typename Piece<VEC>::type P;
    const unsigned lane = threadIdx.x % WAVE;
    for (unsigned r = blockIdx.x * WAVES + wave_id(); r < rows; r += gridDim.x * WAVES) {
        const unsigned gw = r / T, j = r - gw * T, g = w0 + gw;
        const int* d = find_row(table, S, CFSP_WIN_OFF, g);
        const unsigned pos = ((unsigned)d[CFSP_WIN_POS] + (g - (unsigned)d[CFSP_WIN_OFF]) * stride + j * rate) % cap;
        const P* src = reinterpret_cast<const P*>(ring) + ((size_t)d[CFSP_SLOT] * cap + pos) * pieces;
        P* dst = reinterpret_cast<P*>(X) + (size_t)r * pieces;
        for (unsigned p = lane; p < pieces; p += WAVE) dst[p] = src[p];
    }
}

// ---- smoothing.  One thread per (table row, c): smooth_run (ring_rows.h), as stream.hip's smooth_logits_kernel
__global__ __launch_bounds__(THREADS) void pool_smooth_logits_kernel(const float* logits, float* __restrict__ state, float* out,
                                                                     const int* __restrict__ table, unsigned SC, unsigned C, float alpha) {
    const float om = __fsub_rn(1.0f, alpha);
    for (unsigned idx = blockIdx.x * THREADS + threadIdx.x; idx < SC; idx += gridDim.x * THREADS) {
        const unsigned s = idx / C, c = idx - s * C;
        const int* d = table + s * COLS;
        const unsigned nW = (unsigned)d[CFSP_NW];
        if (nW == 0) continue;                                                 // the session's state stays as it is
        const size_t at = (size_t)d[CFSP_WIN_OFF] * C + c;
        smooth_run(logits + at, out + at, state + (size_t)d[CFSP_SLOT] * C + c, nW, C, alpha, om, d[CFSP_HAS_STATE] != 0);
    }
}

// The host copy of the table, before any device work.  cap == 0: ring positions are only required to be non-negative (the smoothing call
// has no ring); N / NW < 0: that total is not checked.
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

}  // namespace

extern "C" int cfsp_version(void) { return 100; /* 0.1.0 */ }
extern "C" int cfsp_abi_version(void) { return CFSP_ABI_VERSION; }
extern "C" const char* cfsp_last_error(void) { return g_err; }

extern "C" int cfsp_ring_put(const float* feats, float* ring, const int32_t* table_host, const int32_t* table_dev, int S, int N, int E,
                             int max_streams, int cap, cfsp_stream_t stream) {
    SIDE_REQUIRE(feats && ring && table_host && table_dev, "cfsp_ring_put: null pointer");
    SIDE_REQUIRE(N > 0 && E > 0 && cap > 0, "cfsp_ring_put: bad shape (N=%d E=%d cap=%d)", N, E, cap);
    if (check_table("cfsp_ring_put", table_host, S, max_streams, cap, N, -1)) return 1;
    const bool vec = vec_ok(feats, ring, E);
    const long long pieces = vec ? E / 4 : E;
    SIDE_REQUIRE((long long)max_streams * cap * pieces <= MAX_ITEMS && (long long)N * pieces <= MAX_ITEMS,
                 "cfsp_ring_put: too large for one launch (max_streams=%d cap=%d N=%d E=%d)", max_streams, cap, N, E);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (vec)
        hipLaunchKernelGGL(pool_ring_put_kernel<true>, dim3(blocks_for(N, WAVES)), dim3(THREADS), 0, s, feats, ring, table_dev, (unsigned)S,
                           (unsigned)N, (unsigned)pieces, (unsigned)cap);
    else
        hipLaunchKernelGGL(pool_ring_put_kernel<false>, dim3(blocks_for(N, WAVES)), dim3(THREADS), 0, s, feats, ring, table_dev, (unsigned)S,
                           (unsigned)N, (unsigned)pieces, (unsigned)cap);
    return check_launch("cfsp_ring_put");
}

extern "C" int cfsp_window_sequences(const float* ring, float* X, const int32_t* table_host, const int32_t* table_dev, int S, int NW, int w0,
                                     int w1, int T, int E, int max_streams, int cap, int stride, int rate, cfsp_stream_t stream) {
    SIDE_REQUIRE(ring && X && table_host && table_dev, "cfsp_window_sequences: null pointer");
    SIDE_REQUIRE(NW > 0 && E > 0 && cap > 0, "cfsp_window_sequences: bad shape (NW=%d E=%d cap=%d)", NW, E, cap);
    SIDE_REQUIRE(T >= 1 && T <= CFSP_MAX_T, "cfsp_window_sequences: T=%d outside 1 .. %d", T, CFSP_MAX_T);
    SIDE_REQUIRE(stride >= 1, "cfsp_window_sequences: stride=%d must be at least 1", stride);
    SIDE_REQUIRE(rate >= 1, "cfsp_window_sequences: rate=%d must be at least 1", rate);
    SIDE_REQUIRE(0 <= w0 && w0 < w1 && w1 <= NW, "cfsp_window_sequences: window range [%d, %d) outside 0 .. NW=%d", w0, w1, NW);
    if (check_table("cfsp_window_sequences", table_host, S, max_streams, cap, -1, NW)) return 1;
    for (int s = 0; s < S; ++s) {
        const int nW = table_host[(size_t)s * COLS + CFSP_NW];
        const long long span = (long long)(nW - 1) * stride + (long long)(T - 1) * rate + 1;
        SIDE_REQUIRE(nW == 0 || span <= cap, "cfsp_window_sequences: row %d: the %lld frames of nW=%d windows do not fit a ring of cap=%d", s,
                     span, nW, cap);
    }
    const bool vec = vec_ok(ring, X, E);
    const long long pieces = vec ? E / 4 : E;
    const long long rows = (long long)(w1 - w0) * T;
    SIDE_REQUIRE(rows * pieces <= MAX_ITEMS && (long long)max_streams * cap * pieces <= MAX_ITEMS,
                 "cfsp_window_sequences: too large for one launch (windows=%d T=%d E=%d max_streams=%d cap=%d)", w1 - w0, T, E, max_streams, cap);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (vec)
        hipLaunchKernelGGL(pool_window_sequences_kernel<true>, dim3(blocks_for(rows, WAVES)), dim3(THREADS), 0, s, ring, X, table_dev,
                           (unsigned)S, (unsigned)rows, (unsigned)w0, (unsigned)T, (unsigned)pieces, (unsigned)cap, (unsigned)stride,
                           (unsigned)rate);
    else
        hipLaunchKernelGGL(pool_window_sequences_kernel<false>, dim3(blocks_for(rows, WAVES)), dim3(THREADS), 0, s, ring, X, table_dev,
                           (unsigned)S, (unsigned)rows, (unsigned)w0, (unsigned)T, (unsigned)pieces, (unsigned)cap, (unsigned)stride,
                           (unsigned)rate);
    return check_launch("cfsp_window_sequences");
}

extern "C" int cfsp_smooth_logits(const float* logits, float* state, float* out, const int32_t* table_host, const int32_t* table_dev, int S,
                                  int NW, int C, int max_streams, float alpha, cfsp_stream_t stream) {
    SIDE_REQUIRE(logits && state && out && table_host && table_dev, "cfsp_smooth_logits: null pointer");
    SIDE_REQUIRE(NW > 0 && C > 0, "cfsp_smooth_logits: bad shape (NW=%d C=%d)", NW, C);
    SIDE_REQUIRE(alpha >= 0.0f && alpha < 1.0f, "cfsp_smooth_logits: alpha=%g outside [0, 1)", (double)alpha);
    if (check_table("cfsp_smooth_logits", table_host, S, max_streams, 0, -1, NW)) return 1;
    SIDE_REQUIRE((long long)max_streams * C <= MAX_ITEMS && (long long)NW * C <= MAX_ITEMS,
                 "cfsp_smooth_logits: too large for one launch (max_streams=%d NW=%d C=%d)", max_streams, NW, C);
    hipLaunchKernelGGL(pool_smooth_logits_kernel, dim3(blocks_for((long long)S * C, THREADS)), dim3(THREADS), 0,
                       static_cast<hipStream_t>(stream), logits, state, out, table_dev, (unsigned)S * (unsigned)C, (unsigned)C, alpha);
    return check_launch("cfsp_smooth_logits");
}
