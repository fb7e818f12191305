/*
 * clipfsar_timeline.h -- C ABI of libclipfsar_timeline.so: the timeline of a stream pool, the class scores of every push folded into
 * coarse buckets of windows that outlive the ring (clip_fsar_amd.pool.StreamPool(timeline=Timeline(...)), StreamPool.timeline,
 * StreamPool.recall) for CLIP-FSAR (gfx950 / CDNA4).
 *
 * Window w of a session lies in BUCKET b = w / span, and bucket b lives at ring position b mod B.  State, keyed and guarded as
 * include/ext/clipfsar_baseline.h keys and guards its own, with the bucket ring as a middle dimension:
 *
 *   peak  [max_streams, B, cap] fp32    the highest candidate score of the (session, bucket, class) cell
 *   at    [max_streams, B, cap] int32   the window that score belongs to
 *   above [max_streams, B, cap] int32   the cell's candidates at or above `level` (every candidate without a level)
 *   marks [max_streams, B, cap] int32   the generation of the store slot at the time the cell was written; 0: never
 *   gens  [cap] int32                   the store slots' current generations, each >= 1 (LiveGallery.slot_generations)
 *   keys  [NKEYS] int32                 store-slot lists, one after the other; a row's list is keys[KEY0 .. KEY0 + NC)
 *
 * The cell of (slot, bucket b, key) is LIVE FOR b iff marks == gens[key], at >= 0 and at / span == b; any other cell stands for the
 * empty one, (peak, at, above) = (-inf, -1, 0).  The peak's own window number says which lap of the ring a cell belongs to, so the
 * cell carries no bucket tag.  The caller zeroes a session's marks at open() and reset(), and the gallery bumps a slot's generation
 * when the slot is freed or changes owner.
 *
 * A CANDIDATE is a score that is neither NaN nor -inf (+inf is one).
 *
 * Conventions (as include/ext/clipfsar_baseline.h): the library allocates no device memory and owns no stream, all work is enqueued
 * on `stream` (a hipStream_t) of the CURRENT device; return 0 = success, non-zero = error with the message in cftl_last_error()
 * (thread-local).  Every pointer is a DEVICE pointer owned by the caller except `table_host` and `first_host`, the HOST copies of the
 * table's S rows and of first[S], which the entry point validates before it touches the device; `table_dev` and `first_dev` are the
 * device copies the caller uploaded on `stream` before the call.  Each call is one launch at any number of sessions; no atomics, no
 * workgroup waits on another, and a thread alone touches its cells: two runs give identical bytes.
 */
#ifndef CLIPFSAR_TIMELINE_H
#define CLIPFSAR_TIMELINE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* Built with -fvisibility=hidden: exactly the entry points declared between this push and the pop are exported
 * (tests/test_timeline_abi.py compares `nm -D` with this file). */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

typedef void* cftl_stream_t;

#define CFTL_ABI_VERSION 1
#define CFTL_MAX_STREAMS 65536
#define CFTL_CHUNK 256 /* columns per workgroup: one thread each */
#define CFTL_MAX_SPAN 1048576 /* 2^20 windows per bucket */
#define CFTL_MAX_BUCKETS 65536
/* the fold's table: class_smooth's, redeclared */
#define CFTL_TABLE_COLS 6
#define CFTL_SLOT 0
#define CFTL_NW 1
#define CFTL_OUT0 2
#define CFTL_NC 3
#define CFTL_KEY0 4
#define CFTL_CHUNK0 5
/* the read's table */
#define CFTL_READ_COLS 7
#define CFTL_R_SLOT 0
#define CFTL_R_B0 1
#define CFTL_R_NB 2
#define CFTL_R_NC 3
#define CFTL_R_KEY0 4
#define CFTL_R_OUT0 5
#define CFTL_R_CHUNK0 6
int cftl_version(void);
int cftl_abi_version(void);
const char* cftl_last_error(void);

/* ---- the fold.  The table is the push's: a row of CFTL_TABLE_COLS int32 per session -- SLOT (0 <= slot < max_streams, at most once
 * per table), NW (its windows in this push, >= 0), OUT0 (offset of its row-major [NW, NC] block in the flat scores: the sum of NW * NC
 * over the rows before), NC (>= 1), KEY0 (KEY0 >= 0, KEY0 + NC <= NKEYS; lists may be shared and may overlap, none names a store slot
 * twice), CHUNK0 (the sum of ceil(NC / CFTL_CHUNK) over the rows before) -- and first[r] is the window number of row r's first
 * window: window k of the row is w = first[r] + k.  One workgroup per (row, chunk of CFTL_CHUNK columns), one thread per column j,
 * key = keys[KEY0 + j], over the row's windows in ascending order with the current cell in registers:
 *   entering bucket b    the cell at [slot, b mod B, key] when it is live for b, the empty cell otherwise
 *   candidate s at w     peak = s, at = w when the cell is empty (at < 0) or s > peak -- strictly, so a tie keeps the earlier window and
 *                        of -0.0 and +0.0 the first one's bits stay;  above += 1 when !has_level or s >= level
 *   leaving the bucket   (at a bucket change and at the row's end) iff at >= 0: peak, at, above are written and marks = gens[key]
 * A cell that saw no candidate is not touched; NW may exceed span * B (a full lap inside one call); a key outside [0, cap) touches
 * nothing; a row of NW = 0 touches nothing.  scores is flat, NOUT floats (0: nothing is launched) and only read.
 * 1 <= S <= max_streams <= 65536, cap >= 1, 1 <= B <= 65536, max_streams * B * cap < 2^31, 1 <= span <= 2^20, NKEYS >= 1,
 * first[r] >= 0 and first[r] + NW < 2^31; with has_level: level is finite. */
int cftl_fold(const float* scores, float* peak, int32_t* at, int32_t* above, int32_t* marks, const int32_t* gens, const int32_t* keys,
              const int32_t* table_host, const int32_t* table_dev, const int32_t* first_host, const int32_t* first_dev, int S, int NOUT,
              int NKEYS, int max_streams, int B, int cap, int span, int has_level, float level, cftl_stream_t stream);

/* ---- the read.  The table is its own: a row of CFTL_READ_COLS int32 -- SLOT (0 <= slot < max_streams; a slot may appear in several
 * rows), B0 (the first bucket, >= 0), NB (0 <= NB <= B, and (B0 + NB - 1) * span < 2^31), NC (>= 1), KEY0 (as above), OUT0 (the sum
 * of NB * NC over the rows before), CHUNK0 (the sum of ceil(NC / CFTL_CHUNK) over the rows before).  Row r writes a row-major
 * [NB, NC] block at OUT0 of each of out_peak, out_at and out_above (NOUT elements each): bucket B0 + i, column j holds the cell's
 * (peak, at, above) when it is live for that bucket, (-inf, -1, 0) when it is not, and (NaN, -1, 0) when keys[KEY0 + j] lies outside
 * [0, cap).  The state is only read.  1 <= S <= 65536; the other bounds are the fold's. */
int cftl_read(const float* peak, const int32_t* at, const int32_t* above, const int32_t* marks, const int32_t* gens, const int32_t* keys,
              float* out_peak, int32_t* out_at, int32_t* out_above, const int32_t* table_host, const int32_t* table_dev, int S, int NOUT,
              int NKEYS, int max_streams, int B, int cap, int span, cftl_stream_t stream);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* CLIPFSAR_TIMELINE_H */
