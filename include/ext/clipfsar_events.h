/*
 * clipfsar_events.h -- C ABI of libclipfsar_events.so: onset / offset detection over every (session, class) pair's consecutive windows
 * (clip_fsar_amd.pool.StreamPool(events=EventRule(...))) for CLIP-FSAR (gfx950 / CDNA4).  The push that scores a session's windows
 * reduces them on the device to a compacted list of event records; the host turns the records into events (clip_fsar_amd.events).
 *
 * State is keyed as include/ext/clipfsar_class_smooth.h keys its own: a cell per (session slot, class store slot), valid iff its mark is
 * the store slot's current generation.  Four arrays [max_streams, cap]:
 *
 *   streak int32   >= 0: idle after that many consecutive windows with s >= on;  < 0: active after -1 - streak consecutive windows
 *                  with s < off
 *   length int32   windows of the current event, saturating at 2^31 - 1; meaningful while active
 *   peak   fp32    the maximum over the current idle streak or the current event
 *   marks  int32   the generation of the store slot at the time the cell was written; 0: never
 *
 * and gens [cap] int32 (each >= 1), keys [NKEYS] int32 and the DESCRIPTOR TABLE exactly as cfcs_smooth_classes takes them: one row of
 * CFEV_TABLE_COLS int32 per session in the push -- SLOT, NW, OUT0, NC, KEY0, CHUNK0 with CFEV_CHUNK = 256 columns per workgroup -- so
 * that one host plan and one upload of the keys serve both libraries.  A row of NW = 0 windows touches nothing.  A key outside [0, cap)
 * is never dereferenced: its column emits nothing and writes no state.  No list may name a store slot twice.
 *
 * THE RULE, one pair over its scores s_k in window order, with on, off (off <= on, finite) and min_on, min_off >= 1.  A cell whose mark
 * is not gens[key] starts idle (streak 0, length 0, peak 0).
 *   idle:    s >= on: peak = (streak == 0) ? s : fmaxf(peak, s), streak += 1; when streak == min_on: ONSET at this window with
 *            len = min_on, and the cell is active with no window below off counted and length = min_on.  s < on or s NaN: streak = 0.
 *   active:  length += 1 (saturating), peak = fmaxf(peak, s); the count of windows below off rises when s < off and returns to 0
 *            otherwise (NaN included); when it reaches min_off: OFFSET at this window with len = length - min_off, and the cell is
 *            idle with streak = 0.
 * The window that confirms one transition never counts towards the other (off <= on).  Afterwards the cell's mark is gens[key].  No
 * OFFSET is emitted for a class that was removed (its slot's generation moved on) nor for a session that was closed or reset (the caller
 * zeroed its row of marks): the pair simply starts idle again.
 *
 * RECORDS: events [max_events, 5] int32 = (table row, column j, window k within the row's windows of this call, kind, len) and
 * values [max_events, 2] fp32 = (s_k, peak), ordered by (row, column, window) -- a deterministic order: every record's position is the
 * exclusive prefix sum of the counts before it, never an atomic counter's answer.  n_events [1] int32 receives the TRUE total; records
 * at positions >= max_events are dropped, the state advances all the same.
 *
 * Three launches: a counting pass that commits nothing (per-thread counts and per-workgroup totals into `work`), an exclusive scan of the
 * workgroup totals by one workgroup (no workgroup ever waits on another), and an emitting pass that reruns the machine, places each
 * thread's records through an in-block scan and commits state and marks.  `work` holds cfev_workspace_ints(n_chunks) int32, n_chunks
 * the table's sum of ceil(NC / CFEV_CHUNK).
 *
 * Conventions (as include/ext/clipfsar_class_smooth.h): the library allocates no device memory and owns no stream, all work is enqueued on
 * `stream` (a hipStream_t) of the CURRENT device; return 0 = success, non-zero = error with the message in cfev_last_error()
 * (thread-local).  Every pointer is a DEVICE pointer owned by the caller except `table_host`, the HOST copy of the S rows, which the entry
 * point validates before it touches the device; `table_dev` is the device copy the caller uploaded on `stream` before the call.
 */
#ifndef CLIPFSAR_EVENTS_H
#define CLIPFSAR_EVENTS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* Built with -fvisibility=hidden: exactly the entry points declared between this push and the pop are exported
 * (tests/test_events_abi.py compares `nm -D` with this file). */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

typedef void* cfev_stream_t;

#define CFEV_ABI_VERSION 1
#define CFEV_MAX_STREAMS 65536
#define CFEV_CHUNK 256 /* columns per workgroup: one thread each */
#define CFEV_TABLE_COLS 6
#define CFEV_SLOT 0
#define CFEV_NW 1
#define CFEV_OUT0 2
#define CFEV_NC 3
#define CFEV_KEY0 4
#define CFEV_CHUNK0 5
#define CFEV_ONSET 1
#define CFEV_OFFSET 2
#define CFEV_EVENT_COLS 5 /* row, column, window, kind, len */
#define CFEV_VALUE_COLS 2 /* score, peak */
int cfev_version(void);
int cfev_abi_version(void);
const char* cfev_last_error(void);

/* int32 elements of `work` for a table of n_chunks workgroups: n_chunks * (CFEV_CHUNK + 1); -1 when n_chunks < 1 or the count is 2^31
 * or more */
int cfev_workspace_ints(int n_chunks);

/* ---- detection: for row r and its column j, key = keys[KEY0 + j], s_k = scores[OUT0 + k * NC + j], k = 0 .. NW - 1, the rule above on
 * the cell (SLOT, key).  scores is flat, NOUT floats (the sum of NW * NC over the table; 0: nothing is launched and n_events is left as
 * it is) and is only read.  1 <= S <= max_streams <= 65536, cap >= 1, max_streams * cap < 2^31, NKEYS >= 1, max_events >= 1. */
int cfev_detect(const float* scores, int32_t* streak, int32_t* length, float* peak, int32_t* marks, const int32_t* gens,
                const int32_t* keys, int32_t* events, float* values, int32_t* n_events, int32_t* work, const int32_t* table_host,
                const int32_t* table_dev, int S, int NOUT, int NKEYS, int max_streams, int cap, float on, float off, int min_on,
                int min_off, int max_events, cfev_stream_t stream);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* CLIPFSAR_EVENTS_H */
