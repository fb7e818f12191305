// Window streams (libclipfsar_stream.so, C ABI in include/clipfsar_stream.h): the ring of per-frame tower features of B lockstep streams,
// the gather of sliding windows out of it into context2's input, and the smoothing recurrence over consecutive windows.
// Copy and stream kernels: HBM- and latency-bound, one launch per call, 16-byte accesses where the rows allow them.
// A library of its own: libclipfsar_hip.so, libclipfsar_gallery.so and libclipfsar_gallery_text.so keep their pinned export sets.
#include "ring_rows.h"
#include "side_lib.h"
#include "../../include/clipfsar_stream.h"

namespace {

constexpr int THREADS = 256;

// ---- ring write.  One thread per row piece: idx -> (b, i, piece); the slot of frame i is first_slot + i, wrapped once (n <= cap)
template <bool VEC>
__global__ __launch_bounds__(THREADS) void ring_put_kernel(const float* __restrict__ feats, float* __restrict__ ring, unsigned total,
                                                           unsigned n, unsigned pieces, unsigned cap, unsigned first_slot) {
    typedef typename Piece<VEC>::type P;
    const P* src = reinterpret_cast<const P*>(feats);
    P* dst = reinterpret_cast<P*>(ring);
    for (unsigned idx = blockIdx.x * THREADS + threadIdx.x; idx < total; idx += gridDim.x * THREADS) {
        const unsigned row = idx / pieces, p = idx - row * pieces;
        const unsigned b = row / n, i = row - b * n;
        unsigned slot = first_slot + i;                                    // < 2 cap
        if (slot >= cap) slot -= cap;
        dst[((size_t)b * cap + slot) * pieces + p] = src[idx];
    }
}

// ---- window gather.  One thread per piece of X: idx -> (b, w, j, piece); frame = (first_window + w) * stride + j * rate, its slot is
// (base_slot + w * stride + j * rate) mod cap with base_slot = first_window * stride mod cap from the host
template <bool VEC>
__global__ __launch_bounds__(THREADS) void window_sequences_kernel(const float* __restrict__ ring, float* __restrict__ X, unsigned total,
                                                                   unsigned nW, unsigned T, unsigned pieces, unsigned cap, unsigned stride,
                                                                   unsigned rate, unsigned base_slot) {
    typedef typename Piece<VEC>::type P;
    const P* src = reinterpret_cast<const P*>(ring);
    P* dst = reinterpret_cast<P*>(X);
    for (unsigned idx = blockIdx.x * THREADS + threadIdx.x; idx < total; idx += gridDim.x * THREADS) {
        const unsigned row = idx / pieces, p = idx - row * pieces;
        const unsigned bw = row / T, j = row - bw * T;
        const unsigned b = bw / nW, w = bw - b * nW;
        const unsigned slot = (base_slot + w * stride + j * rate) % cap;   // the host checked that the sum stays below 2^31
        dst[idx] = src[((size_t)b * cap + slot) * pieces + p];
    }
}

// ---- smoothing.  One thread per (b, c): smooth_run (ring_rows.h)
__global__ __launch_bounds__(THREADS) void smooth_logits_kernel(const float* logits, float* __restrict__ state, float* out, unsigned BC,
                                                                unsigned nW, unsigned C, float alpha, int have_state) {
    const float om = __fsub_rn(1.0f, alpha);
    for (unsigned idx = blockIdx.x * THREADS + threadIdx.x; idx < BC; idx += gridDim.x * THREADS) {
        const unsigned b = idx / C, c = idx - b * C;
        const size_t at = (size_t)b * nW * C + c;
        smooth_run(logits + at, out + at, state + idx, nW, C, alpha, om, have_state);
    }
}

}  // namespace

extern "C" int cfss_version(void) { return 100; /* 0.1.0 */ }
extern "C" int cfss_abi_version(void) { return CFSS_ABI_VERSION; }
extern "C" const char* cfss_last_error(void) { return g_err; }

extern "C" int cfss_ring_put(const float* feats, float* ring, int B, int n, int E, int cap, int64_t first_frame, cfss_stream_t stream) {
    SIDE_REQUIRE(feats && ring, "cfss_ring_put: null pointer");
    SIDE_REQUIRE(B > 0 && n > 0 && E > 0 && cap > 0, "cfss_ring_put: bad shape (B=%d n=%d E=%d cap=%d)", B, n, E, cap);
    SIDE_REQUIRE(n <= cap, "cfss_ring_put: n=%d frames do not fit a ring of cap=%d", n, cap);
    SIDE_REQUIRE(first_frame >= 0, "cfss_ring_put: first_frame=%lld is negative", (long long)first_frame);
    const bool vec = vec_ok(feats, ring, E);
    const long long pieces = vec ? E / 4 : E;
    SIDE_REQUIRE((long long)B * cap * pieces <= MAX_ITEMS, "cfss_ring_put: ring too large for one launch (B=%d cap=%d E=%d)", B, cap, E);
    const long long total = (long long)B * n * pieces;
    const unsigned first_slot = (unsigned)(first_frame % cap);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (vec)
        hipLaunchKernelGGL(ring_put_kernel<true>, dim3(blocks_for(total, THREADS)), dim3(THREADS), 0, s, feats, ring, (unsigned)total,
                           (unsigned)n, (unsigned)pieces, (unsigned)cap, first_slot);
    else
        hipLaunchKernelGGL(ring_put_kernel<false>, dim3(blocks_for(total, THREADS)), dim3(THREADS), 0, s, feats, ring, (unsigned)total,
                           (unsigned)n, (unsigned)pieces, (unsigned)cap, first_slot);
    return check_launch("cfss_ring_put");
}

extern "C" int cfss_window_sequences(const float* ring, float* X, int B, int nW, int T, int E, int cap, int stride, int rate,
                                     int64_t first_window, int64_t frames_pushed, cfss_stream_t stream) {
    SIDE_REQUIRE(ring && X, "cfss_window_sequences: null pointer");
    SIDE_REQUIRE(B > 0 && nW > 0 && E > 0 && cap > 0, "cfss_window_sequences: bad shape (B=%d nW=%d E=%d cap=%d)", B, nW, E, cap);
    SIDE_REQUIRE(T >= 1 && T <= CFSS_MAX_T, "cfss_window_sequences: T=%d outside 1 .. %d", T, CFSS_MAX_T);
    SIDE_REQUIRE(stride >= 1, "cfss_window_sequences: stride=%d must be at least 1", stride);
    SIDE_REQUIRE(rate >= 1, "cfss_window_sequences: rate=%d must be at least 1", rate);
    SIDE_REQUIRE(first_window >= 0 && frames_pushed >= 0, "cfss_window_sequences: first_window=%lld / frames_pushed=%lld is negative",
                 (long long)first_window, (long long)frames_pushed);
    const long long span = (long long)(nW - 1) * stride + (long long)(T - 1) * rate;       // last frame offset inside the request
    SIDE_REQUIRE(span + cap <= MAX_ITEMS && first_window <= (INT64_MAX - span) / stride,
                 "cfss_window_sequences: window range too large (nW=%d stride=%d rate=%d first_window=%lld)", nW, stride, rate,
                 (long long)first_window);
    const int64_t lo = first_window * stride, hi = lo + span;
    SIDE_REQUIRE(hi < frames_pushed, "cfss_window_sequences: frame %lld is not pushed yet (%lld frames pushed)", (long long)hi,
                 (long long)frames_pushed);
    SIDE_REQUIRE(lo >= frames_pushed - cap, "cfss_window_sequences: frame %lld is already overwritten (%lld frames pushed, cap=%d)",
                 (long long)lo, (long long)frames_pushed, cap);
    const bool vec = vec_ok(ring, X, E);
    const long long pieces = vec ? E / 4 : E;
    const long long total = (long long)B * nW * T * pieces;
    SIDE_REQUIRE(total <= MAX_ITEMS && (long long)B * cap * pieces <= MAX_ITEMS,
                 "cfss_window_sequences: too large for one launch (B=%d nW=%d T=%d E=%d cap=%d)", B, nW, T, E, cap);
    const unsigned base_slot = (unsigned)(lo % cap);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (vec)
        hipLaunchKernelGGL(window_sequences_kernel<true>, dim3(blocks_for(total, THREADS)), dim3(THREADS), 0, s, ring, X, (unsigned)total,
                           (unsigned)nW, (unsigned)T, (unsigned)pieces, (unsigned)cap, (unsigned)stride, (unsigned)rate, base_slot);
    else
        hipLaunchKernelGGL(window_sequences_kernel<false>, dim3(blocks_for(total, THREADS)), dim3(THREADS), 0, s, ring, X, (unsigned)total,
                           (unsigned)nW, (unsigned)T, (unsigned)pieces, (unsigned)cap, (unsigned)stride, (unsigned)rate, base_slot);
    return check_launch("cfss_window_sequences");
}

extern "C" int cfss_smooth_logits(const float* logits, float* state, float* out, int B, int nW, int C, float alpha, int64_t windows_seen,
                                  cfss_stream_t stream) {
    SIDE_REQUIRE(logits && state && out, "cfss_smooth_logits: null pointer");
    SIDE_REQUIRE(B > 0 && nW > 0 && C > 0, "cfss_smooth_logits: bad shape (B=%d nW=%d C=%d)", B, nW, C);
    SIDE_REQUIRE(alpha >= 0.0f && alpha < 1.0f, "cfss_smooth_logits: alpha=%g outside [0, 1)", (double)alpha);
    SIDE_REQUIRE(windows_seen >= 0, "cfss_smooth_logits: windows_seen=%lld is negative", (long long)windows_seen);
    SIDE_REQUIRE((long long)B * C <= MAX_ITEMS, "cfss_smooth_logits: too large for one launch (B=%d C=%d)", B, C);
    hipLaunchKernelGGL(smooth_logits_kernel, dim3(blocks_for((long long)B * C, THREADS)), dim3(THREADS), 0,
                       static_cast<hipStream_t>(stream), logits, state, out, (unsigned)B * (unsigned)C, (unsigned)nW, (unsigned)C, alpha,
                       windows_seen > 0 ? 1 : 0);
    return check_launch("cfss_smooth_logits");
}
