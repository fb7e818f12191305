/*
 * clipfsar_pool_select.h -- C ABI of libclipfsar_pool_select.so: the selection of a stream pool with a shortlist
 * (clip_fsar_amd.pool.StreamPool(shortlist=...)) for CLIP-FSAR (gfx950 / CDNA4).  cfsh_select (include/ext/clipfsar_shortlist.h) ranks a
 * group's columns by coarse score alone.  In a pool a group is one session's windows of one push, and the pool keeps state per (session
 * slot, class store slot): smoothing, baselines, the event detector.  This selection respects that state -- a pair whose event is running,
 * whose onset streak is counting or that was selected on its own merit a few pushes ago is PINNED and stays listed -- and it defines a
 * gap: a pair that was not scored at the session's previous scoring push starts anew, because the selection zeroes its marks.
 *
 * Conventions (as include/ext/clipfsar_shortlist.h and include/ext/clipfsar_class_smooth.h): the library allocates no memory and owns no
 * stream, all work is enqueued on `stream` (a hipStream_t) of the CURRENT device; return 0 = success, non-zero = error with the message in
 * cfps_last_error() (thread-local).  Every pointer is a DEVICE pointer owned by the caller, WITH ONE EXCEPTION: the group table is passed
 * twice -- `table_host`, a HOST pointer to the G rows, which the entry point reads and validates before it touches the device, and
 * `table_dev`, the device copy of the same rows that the caller uploaded on `stream` before the call, which the kernel reads.  A table has
 * one row of CFPS_TABLE_COLS int32 per group:
 *
 *   [CFPS_Q0]    first query (window) of the group: the sum of NQ over the rows before
 *   [CFPS_NQ]    queries of the group, >= 0; a group without queries selects nothing, writes padding and touches no plane
 *   [CFPS_SLOT]  the session's slot, in [0, max_streams); no slot appears twice -- a group's workgroup alone reads and writes its slot's
 *                rows of the planes, which is what makes the commit free of races
 *   [CFPS_TICK]  the number of this scoring push of the session, >= 1 (1 at its first push that completes a window)
 *
 * The running sum of NQ must end at NQ.
 */
#ifndef CLIPFSAR_POOL_SELECT_H
#define CLIPFSAR_POOL_SELECT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* Built with -fvisibility=hidden: exactly the entry points declared between this push and the pop are exported
 * (tests/test_pool_select_abi.py compares `nm -D` with this file). */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

typedef void* cfps_stream_t;

/* library version (major*10000 + minor*100 + patch), ABI revision (bumped whenever an exported signature or the table layout changes)
 * and the last error text of the calling thread */
#define CFPS_ABI_VERSION 1
#define CFPS_MAX_KEEP 4096     /* CFSH_MAX_KEEP */
#define CFPS_MAX_GROUPS 65536  /* CFSH_MAX_GROUPS */
#define CFPS_MAX_STREAMS 65536 /* CFCS_MAX_STREAMS */
#define CFPS_MAX_HOLD 1048576  /* 2^20 */
#define CFPS_TABLE_COLS 4
#define CFPS_Q0 0
#define CFPS_NQ 1
#define CFPS_SLOT 2
#define CFPS_TICK 3
#define CFPS_NONE 0x7fffffff /* sel_cols of a place without a column; its sel_slots is -1 and its sel_pin 0 */
#define CFPS_PIN_EVENT 1     /* sel_pin bit 0: pinned by the detector's cell */
#define CFPS_PIN_HOLD 2      /* sel_pin bit 1: pinned by the hold */
int cfps_version(void);
int cfps_abi_version(void);
const char* cfps_last_error(void);

/* ---- the pinned selection, per group g of the table (session slot s, tick t), over the NC columns of S [NQ, NC]:
 *   the group's score  of column c is cfsh_select's: the maximum of S[q, c] over the group's queries, NaN ignored; a column that is NaN in
 *                      every query has no score; a column without a score or with a score of -inf is not selectable; -0.0 == +0.0
 *   pinned             is a column c whose key = cols[c] lies in [0, cap) and for whose cell = s * cap + key
 *                          seen[cell] == t - 1, and
 *                          (ev_marks is given and ev_marks[cell] == gens[key] and ev_streak[cell] != 0)          -> CFPS_PIN_EVENT
 *                          or (hold > 0 and merit[cell] >= 1 and t - merit[cell] <= hold)                       -> CFPS_PIN_HOLD
 *   kept               with P the number of pinned columns and K = min(keep, NC):
 *                          P <= K: every pinned column, whatever its score, and the K - P best selectable columns that are not pinned,
 *                                  the larger score first, the lower column on equal scores;
 *                          P >  K: the K best pinned columns, the larger score first, the lower column on equal scores; a pinned column
 *                                  that is not selectable ranks below every score, the lower column first
 *   written            in ASCENDING COLUMN ORDER: sel_cols[g * K + r] = the column, sel_slots[g * K + r] = cols[column], sel_pin[g * K + r]
 *                      = its CFPS_PIN_* bits (0: selected on its score); the places behind the kept ones hold CFPS_NONE, -1 and 0;
 *                      n_pins[g] = P, the true count (0 for a group without queries)
 *   committed          by the same launch, for every kept column whose key lies in [0, cap):
 *                          if seen[cell] != t - 1 (the pair is new, or returns after a gap): smooth_marks[cell], base_marks[cell] and
 *                              ev_marks[cell] = 0, each where the plane is given -- the pair starts anew in every state launch behind
 *                          seen[cell] = t
 *                          merit[cell] = t when the place's sel_pin is 0
 * The kept set, its order and the planes afterwards are a function of the bits of the inputs alone: a place is a prefix sum over the
 * columns, never a race, and two runs write the same bytes.  One 256-thread workgroup per group: the pins are counted, the group scores go
 * into `work` as 32-bit keys in which the pins are folded (P <= K: a pin's key is above every score; P > K: only pins have a key), then
 * the radix passes and the compaction of cfsh_select (one body, ext/select_keys.h).  The planes are read and written by the workgroup of
 * their slot alone; cols must not name a store slot in [0, cap) twice (the two columns would share a cell).
 * S [NQ, NC] fp32; cols [NC], gens [cap] int32; ev_streak, ev_marks, seen, merit, smooth_marks, base_marks [max_streams, cap] int32 --
 * ev_streak and ev_marks are both NULL or both given, smooth_marks and base_marks may each be NULL; sel_cols, sel_slots, sel_pin [G * K],
 * n_pins [G] int32; work: cfps_workspace_floats(G, NC) floats, contents undefined afterwards.  1 <= keep <= CFPS_MAX_KEEP, 0 <= hold <=
 * CFPS_MAX_HOLD, 1 <= G <= CFPS_MAX_GROUPS, G <= max_streams <= CFPS_MAX_STREAMS, NQ >= 1, NC >= 1, cap >= 1; NQ * NC, G * NC and
 * max_streams * cap below 2^31. */
int cfps_workspace_floats(int G, int NC); /* G * NC, or -1 when an argument is out of range or the product reaches 2^31 */
int cfps_select_pinned(const float* S, const int32_t* cols, const int32_t* gens, const int32_t* ev_streak, int32_t* ev_marks, int32_t* seen,
                       int32_t* merit, int32_t* smooth_marks, int32_t* base_marks, const int32_t* table_host, const int32_t* table_dev,
                       int G, int NQ, int NC, int keep, int hold, int max_streams, int cap, int32_t* sel_cols, int32_t* sel_slots,
                       int32_t* sel_pin, int32_t* n_pins, float* work, cfps_stream_t stream);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* CLIPFSAR_POOL_SELECT_H */
