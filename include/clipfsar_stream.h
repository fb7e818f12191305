/*
 * clipfsar_stream.h -- C ABI of libclipfsar_stream.so: the device side of sliding-window classification of frame streams
 * (clip_fsar_amd.stream.WindowStream) for CLIP-FSAR (gfx950 / CDNA4).
 *
 * In the eval branch the image tower is per frame (few_shot.py:971-999, get_feats): nothing mixes frames before context2.  A stream
 * therefore keeps the tower features of its last frames in a ring, and a window's context2 input is a gather of T ring rows.  This
 * library holds the ring write, the window gather and the smoothing recurrence over consecutive windows; the tower and context2 run
 * on libclipfsar_hip.so, the scores on libclipfsar_gallery.so / libclipfsar_gallery_text.so.
 *
 * Streams advance in lockstep.  Frames of a stream are numbered t = 0, 1, ... ; frame t lives in ring slot t mod cap.  Window k holds
 * frames k * stride + j * rate, j = 0 .. T-1.
 *
 * Conventions (as include/clipfsar_gallery.h): every pointer is a DEVICE pointer owned by the caller, the library allocates no device
 * memory and owns no stream, all work is enqueued on `stream` (a hipStream_t) of the CURRENT device; return 0 = success, non-zero =
 * error with the message in cfss_last_error() (thread-local).  Every entry point validates its arguments before it touches the device.
 * All tensors are fp32 row-major.  Each call is one launch at any B, n, nW.  Rows are moved with 16-byte accesses when E % 4 == 0 and
 * both pointers are 16-byte aligned, with 4-byte accesses otherwise.
 */
#ifndef CLIPFSAR_STREAM_H
#define CLIPFSAR_STREAM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* Built with -fvisibility=hidden: exactly the entry points declared between this push and the pop are exported
 * (tests/test_stream_abi.py compares `nm -D` with this file). */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

typedef void* cfss_stream_t;

/* library version (major*10000 + minor*100 + patch), ABI revision (bumped whenever an exported signature changes or is added) and the
 * last error text of the calling thread */
#define CFSS_ABI_VERSION 1
#define CFSS_MAX_T 32
int cfss_version(void);
int cfss_abi_version(void);
const char* cfss_last_error(void);

/* ---- ring write: ring[b, (first_frame + i) mod cap] = feats[b, i], i = 0 .. n-1.
 * feats [B, n, E], ring [B, cap, E]; first_frame >= 0 the absolute number of feats[:, 0]; 1 <= n <= cap. */
int cfss_ring_put(const float* feats, float* ring, int B, int n, int E, int cap, int64_t first_frame, cfss_stream_t stream);

/* ---- window gather: X[b * nW + w, j] = ring[b, ((first_window + w) * stride + j * rate) mod cap], w = 0 .. nW-1, j = 0 .. T-1.
 * ring [B, cap, E], X [B * nW, T, E] (the context2 input: one sequence of T rows per window).  1 <= T <= 32, stride >= 1, rate >= 1.
 * frames_pushed = frames written to the ring so far (per stream).  Fails on the host, before any launch, when a requested frame is
 * not pushed yet (>= frames_pushed) or already overwritten (< frames_pushed - cap). */
int cfss_window_sequences(const float* ring, float* X, int B, int nW, int T, int E, int cap, int stride, int rate, int64_t first_window,
                          int64_t frames_pushed, cfss_stream_t stream);

/* ---- smoothing over the consecutive windows of a stream: y_0 = x_0, y_k = fmaf(alpha, y_{k-1}, (1 - alpha) * x_k), with 1 - alpha and
 * the product rounded to fp32.  logits [B, nW, C] holds x of windows windows_seen .. windows_seen + nW - 1, state [B, C] holds
 * y of window windows_seen - 1 (not read when windows_seen == 0) and receives y of the last window, out [B, nW, C] receives every y
 * (out may be logits).  Sequential in k, one fmaf per step: the bits of y_k do not depend on how the windows were split over calls.
 * 0 <= alpha < 1. */
int cfss_smooth_logits(const float* logits, float* state, float* out, int B, int nW, int C, float alpha, int64_t windows_seen,
                       cfss_stream_t stream);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* CLIPFSAR_STREAM_H */
