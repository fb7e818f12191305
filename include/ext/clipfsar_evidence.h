/*
 * clipfsar_evidence.h -- C ABI of libclipfsar_evidence.so: the event evidence of a stream pool
 * (clip_fsar_amd.pool.StreamPool(events=..., evidence=Evidence(...))) for CLIP-FSAR (gfx950 / CDNA4).  The push that detects an event
 * copies the T ring rows of the event's window into a slot of a small store on the device, driven by the detector's records while they
 * are still there: no host synchronisation.  The store is a ring of `capacity` slots of [T, E] fp32; a capture stays readable until
 * `capacity` later captures have overwritten it, whatever becomes of the session's own ring.
 *
 * One entry point over the records of ONE cfev_detect call (include/ext/clipfsar_events.h: events [max_events, 5] int32 =
 * (table row, column j, window k, kind, len) and n_events [1] int32, as the detector leaves them) and a DESCRIPTOR TABLE of its own with
 * one row of CFED_TABLE_COLS int32 per row of the detector's table:
 *
 *   SLOT   the session's slot of the pool's ring
 *   POS0   ring position of the first frame of the row's first window of this push, (first_window * stride) mod cap, in the pool's
 *          `rate` form (a pool with rates: its rmax form, as include/ext/clipfsar_tempo.h has it)
 *   NW     the row's windows of this push
 *   KEEP0  the smallest k whose window is still wholly in the ring after the push (a push of several rounds has overwritten earlier ones)
 *   OUT0   as in the detector's table: where the row's [NW, NC] block of cells starts; with NC it locates a record's cell in `tempo`
 *   NC     the row's columns
 *
 * SEMANTICS.  Record i < min(n_events, max_events) QUALIFIES when its kind is in `kinds` (bit 0: CFEV_ONSET records, bit 1: CFEV_OFFSET
 * records), 0 <= row < S, 0 <= k < NW[row], 0 <= j < NC[row] and k >= KEEP0[row].  Qualifying records are ranked in record order by an
 * exclusive count; rank r < capacity receives store slot (head + r) mod capacity, and afterwards head = (head + min(qualifying,
 * capacity)) mod capacity.  where[i] = (slot, tempo index) of a captured record, and otherwise, for EVERY i < max_events:
 *   (-1, 0)   the kind is not captured, i is beyond the records, or the record is malformed (row, k or j out of range: its table row is
 *             never dereferenced beyond the bounds it failed, its cell of `tempo` never read)
 *   (-2, 0)   k < KEEP0: the window has left the ring
 *   (-3, 0)   the record qualifies, its rank is >= capacity
 * Slot s receives, for j' = 0 .. T - 1, the row ring[SLOT, (POS0 + k * stride + shift + j' * r) mod cap]: without `tempo` r = rate and
 * shift = 0 (tempo index 0); with it t = tempo[OUT0 + k * NC + j] (a value outside [0, R) is read as R - 1), r = rates[t] and
 * shift = (T - 1) * (rates[R - 1] - r), and rate must be rates[R - 1].  All arithmetic is integer, positions in 64 bit.  Store slots not
 * assigned in this call keep their bytes; ring, events, n_events and tempo are only read.  Two runs from the same head write the same
 * bytes everywhere.
 *
 * Two launches, no atomics, no workgroup waiting on another: a placement pass by ONE workgroup (chunks of 256 records in record order,
 * an in-block exclusive scan on top of a running base; it writes `where`, one source descriptor per store slot into `work` -- "none"
 * for every slot not assigned in this call, so `work` is fully rewritten -- and last the head), then a copy pass of one wave per
 * destination row of the store, capacity * T rows in a grid-stride loop: every store row has one writer, and the grid does not depend
 * on max_events.  Rows move in 16-byte pieces when E % 4 == 0 and ring and store are 16-byte aligned, in 4-byte pieces otherwise.
 *
 * Conventions (as include/ext/clipfsar_tempo.h): the library allocates no memory and owns no stream, all work is enqueued on `stream`
 * (a hipStream_t) of the CURRENT device; return 0 = success, non-zero = error with the message in cfed_last_error() (thread-local).
 * Every pointer is a DEVICE pointer owned by the caller, WITH TWO EXCEPTIONS, both read and validated before the device is touched and
 * needed only for the duration of the call: `table_host`, the HOST copy of the descriptor table whose device copy `table_dev` the
 * kernel reads, and `rates_host`, a HOST pointer to the R rates -- the kernel receives them by value, a struct of 8 ints.
 */
#ifndef CLIPFSAR_EVIDENCE_H
#define CLIPFSAR_EVIDENCE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* Built with -fvisibility=hidden: exactly the entry points declared between this push and the pop are exported
 * (tests/test_evidence_abi.py compares `nm -D` with this file). */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

typedef void* cfed_stream_t;

#define CFED_ABI_VERSION 1
#define CFED_MAX_STREAMS 65536
#define CFED_MAX_RATES 8
#define CFED_CHUNK 256 /* records per step of the placement pass: one thread each */
#define CFED_TABLE_COLS 6
#define CFED_SLOT 0
#define CFED_POS0 1
#define CFED_NW 2
#define CFED_KEEP0 3
#define CFED_OUT0 4
#define CFED_NC 5
#define CFED_KIND_ONSET 1  /* bit 0 of `kinds`: records of kind CFEV_ONSET */
#define CFED_KIND_OFFSET 2 /* bit 1 of `kinds`: records of kind CFEV_OFFSET */
#define CFED_NOT_CAPTURED (-1)
#define CFED_LEFT_RING (-2)
#define CFED_NO_ROOM (-3)
#define CFED_WORK_COLS 3 /* a store slot's source descriptor: ring slot (-1: none), first position, frame distance */
int cfed_version(void);
int cfed_abi_version(void);
const char* cfed_last_error(void);

/* int32 elements of `work` for a store of `capacity` slots: capacity * CFED_WORK_COLS; -1 when capacity < 1 or the count is 2^31 or more */
int cfed_workspace_ints(int capacity);

/* ---- capture (the semantics above).  ring [max_streams, cap, E] fp32; events [max_events, 5] int32; n_events [1] int32; tempo int32,
 * the push's session-major tempo plane, or NULL exactly when R == 0 (rates_host is then not read); store [capacity, T, E] fp32;
 * head [1] int32 in [0, capacity); where [max_events, 2] int32; work cfed_workspace_ints(capacity) int32.
 * 1 <= S <= max_streams <= 65536; T, E, cap, stride, rate >= 1; capacity >= 1; capacity * T * E and max_streams * cap below 2^31;
 * max_events >= 1; kinds in 1 .. 3; with rates 1 <= R <= 8, rates[0] >= 1, ascending, rates[R - 1] == rate.  Per table row:
 * 0 <= SLOT < max_streams, 0 <= POS0 < cap, NW >= 0, 0 <= KEEP0 <= NW, NC >= 1, OUT0 >= 0, and when KEEP0 < NW:
 * (NW - 1 - KEEP0) * stride + (T - 1) * rate + 1 <= cap -- the windows that can be captured lie in the ring together.  A store that
 * overlaps the ring is refused.  Moves 2 * captured * T * E * 4 bytes.  Two launches. */
int cfed_capture(const float* ring, const int32_t* events, const int32_t* n_events, const int32_t* tempo, float* store, int32_t* head,
                 int32_t* where, int32_t* work, const int32_t* table_host, const int32_t* table_dev, int S, int max_streams, int cap,
                 int max_events, int kinds, int T, int E, int stride, int rate, const int32_t* rates_host, int R, int capacity,
                 cfed_stream_t stream);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* CLIPFSAR_EVIDENCE_H */
