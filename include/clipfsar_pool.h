/*
 * clipfsar_pool.h -- C ABI of libclipfsar_pool.so: the device side of a pool of window streams whose sessions join, leave and push
 * unevenly (clip_fsar_amd.pool.StreamPool) for CLIP-FSAR (gfx950 / CDNA4).
 *
 * include/clipfsar_stream.h serves B lockstep streams described by one (B, n, first_frame) triple.  Here every session owns one slot
 * of ring [max_streams, cap, E] and numbers its own frames; a push is described by a DESCRIPTOR TABLE with one row of CFSP_TABLE_COLS
 * int32 per session in the push (O(sessions), never O(frames)):
 *
 *   [CFSP_SLOT]      ring slot of the session, 0 <= slot < max_streams, at most once per table
 *   [CFSP_PUT_POS]   ring position of the first frame written: frames_before mod cap
 *   [CFSP_N]         frames the session writes, 0 <= n <= cap
 *   [CFSP_FEAT_OFF]  row of the session's first frame in the packed features: the sum of n over the rows before
 *   [CFSP_WIN_POS]   ring position of the first frame of the session's first window: (first_window * stride) mod cap
 *   [CFSP_NW]        windows the session completes, >= 0
 *   [CFSP_WIN_OFF]   index of the session's first window in the packed window list: the sum of nW over the rows before
 *   [CFSP_HAS_STATE] 1 when state[slot] holds y of the session's window before its first one here, else 0
 *
 * 64-bit frame and window numbers stay on the host: the device sees positions below cap.  Window w of a row holds the ring positions
 * (win_pos + w * stride + j * rate) mod cap, j = 0 .. T-1.
 *
 * Conventions (as include/clipfsar_stream.h): the library allocates no memory and owns no stream, all work is enqueued on `stream` (a
 * hipStream_t) of the CURRENT device; return 0 = success, non-zero = error with the message in cfsp_last_error() (thread-local).  All
 * tensors are fp32 row-major.  Every pointer is a DEVICE pointer owned by the caller, WITH ONE EXCEPTION: the table is passed twice --
 * `table_host`, a HOST pointer to the S rows, which the entry point reads and validates before it touches the device, and `table_dev`,
 * the device copy of the same rows that the caller uploaded on `stream` before the call, which the kernel reads.  The host rows need to
 * stay valid only for the duration of the call.  Each call is one launch at any number of sessions.  Rows are moved with 16-byte
 * accesses when E % 4 == 0 and both pointers are 16-byte aligned, with 4-byte accesses otherwise.
 */
#ifndef CLIPFSAR_POOL_H
#define CLIPFSAR_POOL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* Built with -fvisibility=hidden: exactly the entry points declared between this push and the pop are exported
 * (tests/test_pool_abi.py compares `nm -D` with this file). */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

typedef void* cfsp_stream_t;

/* library version (major*10000 + minor*100 + patch), ABI revision (bumped whenever an exported signature or the table layout changes)
 * and the last error text of the calling thread */
#define CFSP_ABI_VERSION 1
#define CFSP_MAX_T 32
#define CFSP_MAX_STREAMS 65536
#define CFSP_TABLE_COLS 8
#define CFSP_SLOT 0
#define CFSP_PUT_POS 1
#define CFSP_N 2
#define CFSP_FEAT_OFF 3
#define CFSP_WIN_POS 4
#define CFSP_NW 5
#define CFSP_WIN_OFF 6
#define CFSP_HAS_STATE 7
int cfsp_version(void);
int cfsp_abi_version(void);
const char* cfsp_last_error(void);

/* ---- ring write: ring[slot_s, (put_pos_s + i) mod cap] = feats[feat_off_s + i], i = 0 .. n_s - 1, for every row s of the table.
 * feats [N, E] packed session-major, ring [max_streams, cap, E]; N = the sum of n over the table, N >= 1. */
int cfsp_ring_put(const float* feats, float* ring, const int32_t* table_host, const int32_t* table_dev, int S, int N, int E,
                  int max_streams, int cap, cfsp_stream_t stream);

/* ---- window gather: the windows g = w0 .. w1 - 1 of the packed window list (NW = the sum of nW over the table; g = win_off_s + w) into
 * X [w1 - w0, T, E], context2's input: X[g - w0, j] = ring[slot_s, (win_pos_s + w * stride + j * rate) mod cap].  0 <= w0 < w1 <= NW: a
 * range may start and end inside sessions.  1 <= T <= 32, stride >= 1, rate >= 1.  Fails when the frames of a row's windows,
 * (nW - 1) * stride + (T - 1) * rate + 1 of them, cannot lie in a ring of cap positions at once. */
int cfsp_window_sequences(const float* ring, float* X, const int32_t* table_host, const int32_t* table_dev, int S, int NW, int w0, int w1,
                          int T, int E, int max_streams, int cap, int stride, int rate, cfsp_stream_t stream);

/* ---- smoothing over the consecutive windows of every session: y_0 = x_0, y_k = fmaf(alpha, y_{k-1}, (1 - alpha) * x_k), with 1 - alpha
 * and the product rounded to fp32 -- the recurrence and the bits of cfss_smooth_logits.  logits [NW, C] packed as the window list,
 * state [max_streams, C] indexed by slot: read when has_state is 1, receives y of the session's last window when nW > 0 and is left
 * alone otherwise; out [NW, C] receives every y (out may be logits).  Sequential in a session's k.  0 <= alpha < 1. */
int cfsp_smooth_logits(const float* logits, float* state, float* out, const int32_t* table_host, const int32_t* table_dev, int S, int NW,
                       int C, int max_streams, float alpha, cfsp_stream_t stream);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* CLIPFSAR_POOL_H */
