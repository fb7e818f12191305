/*
 * clipfsar_baseline.h -- C ABI of libclipfsar_baseline.so: adaptive baselines of a stream pool, a running mean and mean absolute
 * deviation per (session slot, class store slot), and the deviation of every score from them
 * (clip_fsar_amd.pool.StreamPool(baseline=Baseline(...))) for CLIP-FSAR (gfx950 / CDNA4).
 *
 * The scores of a pool share no scale: OTAM logits, COMBINE probabilities around 1 / (classes in the list), a class with five shots
 * against one enrolled from a single window.  A threshold means something on z = (s - mean) / dev of the pair's own scores.  State, keyed
 * and guarded exactly as include/ext/clipfsar_class_smooth.h keys and guards its own:
 *
 *   mean  [max_streams, cap] fp32    the pair's running mean m
 *   dev   [max_streams, cap] fp32    its running mean absolute deviation d
 *   count [max_streams, cap] int32   the windows folded in so far, n, which stays at `warmup` once it is reached
 *   marks [max_streams, cap] int32   the generation of the store slot at the time the cell was written; 0: never
 *   gens  [cap] int32                the store slots' current generations, each >= 1 (LiveGallery.slot_generations)
 *   keys  [NKEYS] int32              store-slot lists, one after the other; a session's list is keys[KEY0 .. KEY0 + NC)
 *
 * A cell is VALID iff marks[slot, key] == gens[key]; any other cell starts with n = 0.  The caller invalidates a session's row of marks
 * (zeroes it) at open() and reset(), and the gallery bumps a slot's generation when the slot is freed or changes owner.
 *
 * A push is described by class_smooth's DESCRIPTOR TABLE, redeclared here, one row of CFBL_TABLE_COLS int32 per session in the push:
 *
 *   [CFBL_SLOT]    the session's slot, 0 <= slot < max_streams, at most once per table
 *   [CFBL_NW]      its windows in this push, >= 0; a row of 0 windows touches nothing
 *   [CFBL_OUT0]    offset of its row-major [NW, NC] block in the flat scores: the sum of NW * NC over the rows before
 *   [CFBL_NC]      its width, >= 1
 *   [CFBL_KEY0]    offset of its store-slot list in keys, KEY0 >= 0 and KEY0 + NC <= NKEYS.  Lists may be shared and may overlap
 *   [CFBL_CHUNK0]  the sum of ceil(NC / CFBL_CHUNK) over the rows before: the row's first workgroup
 *
 * No list may name a store slot twice (the two columns would share a cell); the keys live on the device, so this is the caller's to keep.
 * A key outside [0, cap) is never dereferenced: its column of out is NaN and no state is written.
 *
 * Conventions (as include/ext/clipfsar_class_smooth.h): the library allocates no memory and owns no stream, all work is enqueued on
 * `stream` (a hipStream_t) of the CURRENT device; return 0 = success, non-zero = error with the message in cfbl_last_error()
 * (thread-local).  Every pointer is a DEVICE pointer owned by the caller, WITH ONE EXCEPTION: the table is passed twice -- `table_host`,
 * a HOST pointer to the S rows, which the entry point reads and validates before it touches the device, and `table_dev`, the device copy
 * of the same rows that the caller uploaded on `stream` before the call, which the kernel reads.  The call is one launch at any number
 * of sessions.
 */
#ifndef CLIPFSAR_BASELINE_H
#define CLIPFSAR_BASELINE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* Built with -fvisibility=hidden: exactly the entry points declared between this push and the pop are exported
 * (tests/test_baseline_abi.py compares `nm -D` with this file). */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

typedef void* cfbl_stream_t;

/* library version (major*10000 + minor*100 + patch), ABI revision (bumped whenever an exported signature or the table layout changes)
 * and the last error text of the calling thread */
#define CFBL_ABI_VERSION 1
#define CFBL_MAX_STREAMS 65536
#define CFBL_CHUNK 256 /* columns per workgroup: one thread each */
#define CFBL_TABLE_COLS 6
#define CFBL_SLOT 0
#define CFBL_NW 1
#define CFBL_OUT0 2
#define CFBL_NC 3
#define CFBL_KEY0 4
#define CFBL_CHUNK0 5
#define CFBL_MAX_WARMUP 1048576 /* 2^20 */
int cfbl_version(void);
int cfbl_abi_version(void);
const char* cfbl_last_error(void);

/* ---- the deviation per (session, class): for row r and its column j, key = keys[KEY0 + j], the cell (m, d, n) = (mean, dev,
 * count)[slot, key] when it is valid and n = 0 otherwise; over the row's windows k = 0 .. NW - 1 in order, s = scores[OUT0 + k * NC + j],
 * z = out[OUT0 + k * NC + j]:
 *   s not finite       z = NaN, the cell is untouched
 *   n == 0             m = s, d = 0, n = 1, z = NaN
 *   n < warmup         z = NaN; update with r = warm_rate; n += 1
 *   otherwise          z = (s - m) / fmaxf(d, floor); update with r = rate unless z >= gate (a window that stands out is not folded
 *                      into its own baseline); n stays at warmup
 *   update             keep = 1 - r;  a = |s - m| with the old m;  m = keep * m + r * s;  d = keep * d + r * a
 * Every operation is ONE correctly rounded fp32 operation (both products are rounded before their sum; nothing is fused), so the
 * recurrence restated in IEEE fp32 scalars on the host gives the same bits.  Afterwards mean, dev and count hold the cell and
 * marks[slot, key] = gens[key].  scores and out are flat, NOUT floats (the sum of NW * NC over the table; 0: nothing is launched); out
 * may be scores.  1 <= S <= max_streams <= 65536, cap >= 1, max_streams * cap < 2^31, NKEYS >= 1, 0 < rate < 1, 0 < warm_rate <= 1,
 * 1 <= warmup <= 2^20, gate > 0 (+inf: nothing is gated), 0 < floor < inf. */
int cfbl_normalize(const float* scores, float* mean, float* dev, int32_t* count, int32_t* marks, const int32_t* gens,
                   const int32_t* keys, float* out, const int32_t* table_host, const int32_t* table_dev, int S, int NOUT, int NKEYS,
                   int max_streams, int cap, float rate, float warm_rate, int warmup, float gate, float floor, cfbl_stream_t stream);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* CLIPFSAR_BASELINE_H */
