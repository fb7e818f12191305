/*
 * clipfsar_class_smooth.h -- C ABI of libclipfsar_class_smooth.so: the smoothing recurrence of a stream pool whose state is keyed by
 * (session slot, class store slot) instead of by column (clip_fsar_amd.pool.StreamPool(smooth_by="class")) for CLIP-FSAR (gfx950 / CDNA4).
 *
 * include/clipfsar_pool.h smooths [NW, C] logits against state [max_streams, C]: a state cell belongs to a COLUMN, and a column is only
 * an index into the gallery's class order of the moment.  Here a cell belongs to a class's slot of the live gallery's store, which keeps
 * its number while other classes come and go:
 *
 *   state [max_streams, cap] fp32    y of the pair's last window
 *   marks [max_streams, cap] int32   the generation of the store slot at the time the cell was written; 0: never
 *   gens  [cap] int32                the store slots' current generations, each >= 1 (LiveGallery.slot_generations)
 *   keys  [NKEYS] int32              store-slot lists, one after the other; a session's list is keys[KEY0 .. KEY0 + NC)
 *
 * A cell is VALID iff marks[slot, key] == gens[key].  A valid cell continues the recurrence, any other starts it (y = x); either way
 * the cell receives y of the pair's last window and the mark the slot's generation.  The caller invalidates a session's row of marks
 * (zeroes it) at open() and reset(), and the gallery bumps a slot's generation when the slot is freed or changes owner.
 *
 * A push is described by a DESCRIPTOR TABLE with one row of CFCS_TABLE_COLS int32 per session in the push:
 *
 *   [CFCS_SLOT]    the session's slot, 0 <= slot < max_streams, at most once per table
 *   [CFCS_NW]      its windows in this push, >= 0; a row of 0 windows touches neither state nor marks
 *   [CFCS_OUT0]    offset of its row-major [NW, NC] block in the flat logits: the sum of NW * NC over the rows before
 *   [CFCS_NC]      its width, >= 1
 *   [CFCS_KEY0]    offset of its store-slot list in keys, KEY0 >= 0 and KEY0 + NC <= NKEYS.  Lists may be shared and may overlap: every
 *                  session without a list of its own points at one "every class" list
 *   [CFCS_CHUNK0]  the sum of ceil(NC / CFCS_CHUNK) over the rows before: the row's first workgroup
 *
 * No list may name a store slot twice (the two columns would share a cell); the keys live on the device, so this is the caller's to keep.
 * A key outside [0, cap) is never dereferenced: its column of out is NaN and no state is written.
 *
 * Conventions (as include/clipfsar_pool.h): the library allocates no memory and owns no stream, all work is enqueued on `stream` (a
 * hipStream_t) of the CURRENT device; return 0 = success, non-zero = error with the message in cfcs_last_error() (thread-local).  Every
 * pointer is a DEVICE pointer owned by the caller, WITH ONE EXCEPTION: the table is passed twice -- `table_host`, a HOST pointer to the S
 * rows, which the entry point reads and validates before it touches the device, and `table_dev`, the device copy of the same rows that
 * the caller uploaded on `stream` before the call, which the kernel reads.  The call is one launch at any number of sessions.
 */
#ifndef CLIPFSAR_CLASS_SMOOTH_H
#define CLIPFSAR_CLASS_SMOOTH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* Built with -fvisibility=hidden: exactly the entry points declared between this push and the pop are exported
 * (tests/test_class_smooth_abi.py compares `nm -D` with this file). */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

typedef void* cfcs_stream_t;

/* library version (major*10000 + minor*100 + patch), ABI revision (bumped whenever an exported signature or the table layout changes)
 * and the last error text of the calling thread */
#define CFCS_ABI_VERSION 1
#define CFCS_MAX_STREAMS 65536
#define CFCS_CHUNK 256 /* columns per workgroup: one thread each */
#define CFCS_TABLE_COLS 6
#define CFCS_SLOT 0
#define CFCS_NW 1
#define CFCS_OUT0 2
#define CFCS_NC 3
#define CFCS_KEY0 4
#define CFCS_CHUNK0 5
int cfcs_version(void);
int cfcs_abi_version(void);
const char* cfcs_last_error(void);

/* ---- smoothing per (session, class): for row s and its column j, key = keys[KEY0 + j], over the row's windows k = 0 .. NW - 1
 *   y_0 = x_0 when the cell (slot, key) is not valid, else y_0 = fmaf(alpha, state[slot, key], (1 - alpha) * x_0);
 *   y_k = fmaf(alpha, y_{k-1}, (1 - alpha) * x_k),   x_k = logits[OUT0 + k * NC + j],   out[OUT0 + k * NC + j] = y_k
 * with 1 - alpha and the product rounded to fp32 -- the recurrence and the bits of cfss_smooth_logits and cfsp_smooth_logits on the
 * pair's own windows.  Then state[slot, key] = y_{NW-1} and marks[slot, key] = gens[key].  logits and out are flat, NOUT floats (the
 * sum of NW * NC over the table; 0: nothing is launched); out may be logits.  1 <= S <= max_streams <= 65536, cap >= 1,
 * max_streams * cap < 2^31, NKEYS >= 1, 0 <= alpha < 1. */
int cfcs_smooth_classes(const float* logits, float* state, int32_t* marks, const int32_t* gens, const int32_t* keys, float* out,
                        const int32_t* table_host, const int32_t* table_dev, int S, int NOUT, int NKEYS, int max_streams, int cap,
                        float alpha, cfcs_stream_t stream);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* CLIPFSAR_CLASS_SMOOTH_H */
