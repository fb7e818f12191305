// Enrolment (libclipfsar_enroll.so, C ABI in include/clipfsar_enroll.h): the support sequences of windows that lie in a stream pool's ring
// -- T ring rows and the class's text row each -- for StreamPool.enroll / enroll_windows, which teach a class from what a session has
// just seen without running the tower again.
// A copy kernel in the style of pool.hip: one WAVE per destination row.  The table has a row per output SEQUENCE, so a destination row's
// table row is row / (T + 1): wave-uniform, loaded with scalar loads, no search.  The lanes then stride over the row's 16-byte pieces.
// A library of its own: the other nine keep their pinned export sets.
#include "ring_rows.h"
#include "side_lib.h"
#include "../../include/clipfsar_enroll.h"

namespace {

constexpr int THREADS = 256;
constexpr int WAVE = 64;
constexpr int WAVES = THREADS / WAVE;
constexpr int COLS = CFEN_TABLE_COLS;

__device__ __forceinline__ unsigned wave_id() { return __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE); }

template <bool VEC> __device__ __forceinline__ typename Piece<VEC>::type nan_piece() { return __builtin_nanf(""); }
template <> __device__ __forceinline__ float4 nan_piece<true>() {
    const float q = __builtin_nanf("");
    return make_float4(q, q, q, q);
}

// vec_ok (ring_rows.h) over the three pointers of this library's one call
inline bool vec_ok3(const void* a, const void* b, const void* c, int E) {
    return E % 4 == 0 && (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15u) == 0;
}

// ---- row r of X0 is row j = r mod (T + 1) of sequence i = r / (T + 1).  j < T: ring[slot_i, (pos_i + j * rate) mod cap] (pos < cap and
// j * rate < cap, the host checked the span: the sum stays below 2 cap); j == T: text[cls_i].  The table row is read from the DEVICE copy
// and checked again: out of range there, the whole sequence is NaN and neither the ring nor the text is read for it.
template <bool VEC>
__global__ __launch_bounds__(THREADS) void ring_sequences_kernel(const float* __restrict__ ring, const float* __restrict__ text,
                                                                 float* __restrict__ X0, const int* __restrict__ table, unsigned rows,
                                                                 unsigned T, unsigned pieces, unsigned max_streams, unsigned cap,
                                                                 unsigned rate, unsigned n_cls) {
    typedef typename Piece<VEC>::type P;
    const unsigned lane = threadIdx.x % WAVE;
    for (unsigned r = blockIdx.x * WAVES + wave_id(); r < rows; r += gridDim.x * WAVES) {
        const unsigned i = r / (T + 1), j = r - i * (T + 1);
        const int* d = table + (size_t)i * COLS;
        const unsigned slot = (unsigned)d[CFEN_SLOT], pos0 = (unsigned)d[CFEN_POS], cls = (unsigned)d[CFEN_CLS];      // negative: huge
        P* dst = reinterpret_cast<P*>(X0) + (size_t)r * pieces;
        if (slot >= max_streams || pos0 >= cap || cls >= n_cls) {
            for (unsigned p = lane; p < pieces; p += WAVE) dst[p] = nan_piece<VEC>();
            continue;
        }
        const P* src;
        if (j < T) {
            unsigned pos = pos0 + j * rate;
            if (pos >= cap) pos -= cap;
            src = reinterpret_cast<const P*>(ring) + ((size_t)slot * cap + pos) * pieces;
        } else {
            src = reinterpret_cast<const P*>(text) + (size_t)cls * pieces;
        }
        for (unsigned p = lane; p < pieces; p += WAVE) dst[p] = src[p];
    }
}

}  // namespace

extern "C" int cfen_version(void) { return 100; /* 0.1.0 */ }
extern "C" int cfen_abi_version(void) { return CFEN_ABI_VERSION; }
extern "C" const char* cfen_last_error(void) { return g_err; }

extern "C" int cfen_ring_sequences(const float* ring, const float* text, const int32_t* table_host, const int32_t* table_dev, int n, int T,
                                   int E, int max_streams, int cap, int rate, int n_cls, float* X0, cfen_stream_t stream) {
    SIDE_REQUIRE(ring && text && table_host && table_dev && X0, "cfen_ring_sequences: null pointer");
    SIDE_REQUIRE(n >= 1 && E >= 1 && max_streams >= 1 && cap >= 1 && n_cls >= 1,
                 "cfen_ring_sequences: bad shape (n=%d E=%d max_streams=%d cap=%d n_cls=%d)", n, E, max_streams, cap, n_cls);
    SIDE_REQUIRE(T >= 1 && T <= CFSP_MAX_T, "cfen_ring_sequences: T=%d outside 1 .. %d", T, CFSP_MAX_T);
    SIDE_REQUIRE(rate >= 1, "cfen_ring_sequences: rate=%d must be at least 1", rate);
    SIDE_REQUIRE((long long)(T - 1) * rate + 1 <= cap, "cfen_ring_sequences: the %lld frames of a window do not fit a ring of cap=%d",
                 (long long)(T - 1) * rate + 1, cap);
    for (int i = 0; i < n; ++i) {
        const int32_t* d = table_host + (size_t)i * COLS;
        SIDE_REQUIRE(d[CFEN_SLOT] >= 0 && d[CFEN_SLOT] < max_streams, "cfen_ring_sequences: row %d has slot %d outside 0 .. %d", i,
                     d[CFEN_SLOT], max_streams - 1);
        SIDE_REQUIRE(d[CFEN_POS] >= 0 && d[CFEN_POS] < cap, "cfen_ring_sequences: row %d has ring position %d outside 0 .. cap-1 (cap=%d)", i,
                     d[CFEN_POS], cap);
        SIDE_REQUIRE(d[CFEN_CLS] >= 0 && d[CFEN_CLS] < n_cls, "cfen_ring_sequences: row %d has class %d outside 0 .. %d", i, d[CFEN_CLS],
                     n_cls - 1);
    }
    const bool vec = vec_ok3(ring, text, X0, E);
    const long long pieces = vec ? E / 4 : E;
    const long long rows = (long long)n * (T + 1);
    SIDE_REQUIRE(rows * pieces <= MAX_ITEMS && (long long)max_streams * cap * pieces <= MAX_ITEMS && (long long)n_cls * pieces <= MAX_ITEMS &&
                     (long long)n * COLS <= MAX_ITEMS,
                 "cfen_ring_sequences: too large for one launch (n=%d T=%d E=%d max_streams=%d cap=%d n_cls=%d)", n, T, E, max_streams, cap,
                 n_cls);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (vec)
        hipLaunchKernelGGL(ring_sequences_kernel<true>, dim3(blocks_for(rows, WAVES)), dim3(THREADS), 0, s, ring, text, X0, table_dev,
                           (unsigned)rows, (unsigned)T, (unsigned)pieces, (unsigned)max_streams, (unsigned)cap, (unsigned)rate,
                           (unsigned)n_cls);
    else
        hipLaunchKernelGGL(ring_sequences_kernel<false>, dim3(blocks_for(rows, WAVES)), dim3(THREADS), 0, s, ring, text, X0, table_dev,
                           (unsigned)rows, (unsigned)T, (unsigned)pieces, (unsigned)max_streams, (unsigned)cap, (unsigned)rate,
                           (unsigned)n_cls);
    return check_launch("cfen_ring_sequences");
}
