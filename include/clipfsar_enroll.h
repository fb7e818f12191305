/*
 * clipfsar_enroll.h -- C ABI of libclipfsar_enroll.so: support sequences out of a stream pool's ring (clip_fsar_amd.pool.StreamPool.enroll,
 * enroll_windows) for CLIP-FSAR (gfx950 / CDNA4).
 *
 * A support sequence is the T tower rows of a clip plus its class's text row (cfsg_support_sequences of include/clipfsar_gallery.h).  The
 * tower rows of a session's recent frames already lie in the pool's ring [max_streams, cap, E] (include/clipfsar_pool.h), so a window a
 * session has seen becomes a shot of a class without the tower: one copy launch builds the support sequences of an ENROLMENT LIST, in the
 * class-grouped order the gallery's registration takes them in.  The list is a table with one row of CFEN_TABLE_COLS int32 per output
 * sequence:
 *
 *   [CFEN_SLOT]  ring slot of the session, 0 <= slot < max_streams; the same slot may appear in any number of rows
 *   [CFEN_POS]   ring position of the window's first frame, 0 <= pos < cap: (window * stride) mod cap
 *   [CFEN_CLS]   row of `text` that closes the sequence, 0 <= cls < n_cls
 *   [CFEN_PAD]   unused, 0 (a row is 16 bytes)
 *
 * This is not the pool's push table (one row per slot, consecutive windows, prefix offsets, no text row): the rows are independent of
 * each other and in the order of the output.  64-bit frame and window numbers stay on the host; which windows of a session are still in
 * its ring is the caller's knowledge (clip_fsar_amd.pool.plan_enroll).
 *
 * Conventions (as include/clipfsar_pool.h): the library allocates no memory and owns no stream, all work is enqueued on `stream` (a
 * hipStream_t) of the CURRENT device; return 0 = success, non-zero = error with the message in cfen_last_error() (thread-local).  All
 * tensors are fp32 row-major.  Every pointer is a DEVICE pointer owned by the caller, WITH ONE EXCEPTION: the table is passed twice --
 * `table_host`, a HOST pointer to the n rows, which the entry point reads and validates before it touches the device, and `table_dev`,
 * the device copy of the same rows that the caller uploaded on `stream` before the call, which the kernel reads.  The host rows need to
 * stay valid only for the duration of the call.  The kernel checks the device rows once more: a sequence whose slot, position or class
 * is out of range THERE is written as NaN and nothing is read for it.  Rows are moved with 16-byte accesses when E % 4 == 0 and all three
 * pointers are 16-byte aligned, with 4-byte accesses otherwise.
 */
#ifndef CLIPFSAR_ENROLL_H
#define CLIPFSAR_ENROLL_H

#include <stdint.h>

#include "clipfsar_pool.h" /* CFSP_MAX_T: the windows are the pool's */

#ifdef __cplusplus
extern "C" {
#endif
/* Built with -fvisibility=hidden: exactly the entry points declared between this push and the pop are exported
 * (tests/test_enroll_abi.py compares `nm -D` with this file). */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

typedef void* cfen_stream_t;

/* library version (major*10000 + minor*100 + patch), ABI revision (bumped whenever an exported signature or the table layout changes)
 * and the last error text of the calling thread */
#define CFEN_ABI_VERSION 1
#define CFEN_TABLE_COLS 4
#define CFEN_SLOT 0
#define CFEN_POS 1
#define CFEN_CLS 2
#define CFEN_PAD 3
int cfen_version(void);
int cfen_abi_version(void);
const char* cfen_last_error(void);

/* ---- support sequences out of the ring: X0 [n, T + 1, E], for every row i of the table
 *        X0[i, j] = ring[slot_i, (pos_i + j * rate) mod cap],  j = 0 .. T - 1
 *        X0[i, T] = text[cls_i]
 * ring [max_streams, cap, E], text [n_cls, E].  n >= 1, E >= 1, 1 <= T <= CFSP_MAX_T, rate >= 1, (T - 1) * rate + 1 <= cap (a window's
 * frames lie in the ring at once), max_streams >= 1, n_cls >= 1; every element count below 2^31.  One launch at any n. */
int cfen_ring_sequences(const float* ring, const float* text, const int32_t* table_host, const int32_t* table_dev, int n, int T, int E,
                        int max_streams, int cap, int rate, int n_cls, float* X0, cfen_stream_t stream);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* CLIPFSAR_ENROLL_H */
