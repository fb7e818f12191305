/*
 * clipfsar_tempo.h -- C ABI of libclipfsar_tempo.so: the tempo windows of a stream pool (clip_fsar_amd.pool.StreamPool(rates=...)) for
 * CLIP-FSAR (gfx950 / CDNA4).  A pool with one `rate` sees window k of a session as its frames k * stride + j * rate, j < T.  With a
 * list of R rates, rates[0] < .. < rates[R - 1] = rmax, the pool plans, sizes its ring and numbers its windows as a pool with
 * rate = rmax, and every window is read R times: TEMPO i of window k is the T frames e_k - (T - 1 - j) * rates[i], j < T, where
 * e_k = k * stride + (T - 1) * rmax is the frame that completes the window.  All tempos of a window end on that frame, so all complete
 * in the same push; tempo R - 1 is the window of the rate = rmax pool.  A window's score for a class is the maximum over its tempos.
 *
 * Two entry points: the gather of the R tempo sequences of every window out of the pool's ring, over the pool's own descriptor table
 * (include/clipfsar_pool.h: the CFSP_* columns, CFSP_MAX_T, CFSP_MAX_STREAMS), and the reduction of the [windows * R, C] scores to
 * [windows, C] scores and the index of the tempo that gave each.
 *
 * Conventions (as include/clipfsar_pool.h): the library allocates no memory and owns no stream, all work is enqueued on `stream` (a
 * hipStream_t) of the CURRENT device; return 0 = success, non-zero = error with the message in cftp_last_error() (thread-local).  All
 * tensors are row-major.  Every pointer is a DEVICE pointer owned by the caller, WITH TWO EXCEPTIONS, both read and validated before the
 * device is touched and needed only for the duration of the call: `table_host`, the HOST copy of the descriptor table whose device copy
 * `table_dev` the kernel reads, and `rates_host`, a HOST pointer to the R rates -- the kernel receives them by value, in its arguments.
 */
#ifndef CLIPFSAR_TEMPO_H
#define CLIPFSAR_TEMPO_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* Built with -fvisibility=hidden: exactly the entry points declared between this push and the pop are exported
 * (tests/test_tempo_abi.py compares `nm -D` with this file). */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

typedef void* cftp_stream_t;

/* library version (major*10000 + minor*100 + patch), ABI revision (bumped whenever an exported signature changes) and the last error
 * text of the calling thread */
#define CFTP_ABI_VERSION 1
#define CFTP_MAX_RATES 8
int cftp_version(void);
int cftp_abi_version(void);
const char* cftp_last_error(void);

/* ---- tempo gather: the windows g = w0 .. w1 - 1 of the table's packed window list (NW = the sum of nW over the table; g = win_off_s + w)
 * into X [(w1 - w0) * R, T, E], rows ordered (window, tempo, frame):
 *     X[((g - w0) * R + i) * T + j] = ring[slot_s, (win_pos_s + w * stride + (T - 1) * (rmax - rates[i]) + j * rates[i]) mod cap]
 * with win_pos_s the ring position of the first frame of the session's first window IN ITS rmax FORM, as a pool with rate = rmax writes
 * it.  0 <= w0 < w1 <= NW: a range may start and end inside sessions.  1 <= T <= CFSP_MAX_T, stride >= 1, 1 <= R <= CFTP_MAX_RATES,
 * 1 <= rates[0] < rates[1] < .. < rates[R - 1].  Fails when the frames of a row's windows, (nW - 1) * stride + (T - 1) * rmax + 1 of them,
 * cannot lie in a ring of cap positions at once, and when (w1 - w0) * R * T row pieces exceed 32-bit sizes.  ring [max_streams, cap, E]
 * and X fp32; rows are moved with 16-byte accesses when E % 4 == 0 and both pointers are 16-byte aligned, with 4-byte accesses otherwise.
 * The ring is only read; every row of X has one writer.  One launch. */
int cftp_window_sequences(const float* ring, float* X, const int32_t* table_host, const int32_t* table_dev, int S, int NW, int w0, int w1,
                          int T, int E, int max_streams, int cap, int stride, const int32_t* rates_host, int R, cftp_stream_t stream);

/* ---- tempo reduction: scores [NW * R, C] fp32, rows ordered (window, tempo) -> out [NW, C] fp32 and tempo [NW, C] int32.  Per cell
 * (w, c), over s_i = scores[(w * R + i) * C + c], i < R:
 *     any s_i is NaN:  tempo = the index of the FIRST NaN and out = that NaN -- a NaN never disappears inside a maximum
 *     otherwise:       out = the largest s_i and tempo = the LOWEST index that holds it (-0.0 == +0.0: the lower index)
 * out is always one of the s_i, bit for bit (no arithmetic touches it); every cell has one writer.  R == 1 is a copy and a plane of
 * zeros, through the same kernel.  1 <= R <= CFTP_MAX_RATES, NW >= 1, C >= 1, NW * R * C below 2^31.  out and tempo may not overlap
 * scores or each other: such a call is refused.  One thread reduces four consecutive classes with 16-byte accesses when C % 4 == 0 and
 * the three pointers are 16-byte aligned, one class otherwise.  Memory-bound: (R + 2) * NW * C * 4 bytes move.  One launch. */
int cftp_reduce(const float* scores, float* out, int32_t* tempo, int NW, int R, int C, cftp_stream_t stream);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* CLIPFSAR_TEMPO_H */
