/*
 * clipfsar_contest.h -- C ABI of libclipfsar_contest.so: the contest of a stream pool with an event rule
 * (clip_fsar_amd.pool.StreamPool(events=EventRule(...), contest=Contest(...))) for CLIP-FSAR (gfx950 / CDNA4).  One stage between the
 * judged scores of a push and cfev_detect: every window's row is ranked on the device, its leading classes keep their scores and every
 * other candidate is demoted to -inf, which no threshold of the detector clears.  The contest keeps no state.
 *
 * The DESCRIPTOR TABLE is exactly cfev_detect's (include/ext/clipfsar_events.h) and cfcs_smooth_classes': one row of CFCT_TABLE_COLS int32
 * per session in the push -- SLOT, NW, OUT0, NC, KEY0, CHUNK0 -- so that one host plan and one upload serve smoothing, baseline, contest
 * and detector.  SLOT and CHUNK0 are ignored here.  A row of NW = 0 windows touches nothing.
 *
 * THE RULE, one ROW -- window k of table row r: s_j = scores[OUT0 + k * NC + j], key_j = keys[KEY0 + j], j = 0 .. NC - 1:
 *   candidate  0 <= key_j < cap, s_j is not NaN and s_j > -inf.  keys == NULL: every column has a valid key.
 *   order      a larger float ranks higher; -0.0 and +0.0 are equal.
 *   leaders    the R = min(top, number of candidates) highest candidates; among candidates equal to the R-th score the lowest columns
 *              are taken first.
 *   margin     (has_margin != 0) best = the highest candidate score, floor = best - margin, ONE rounded fp32 subtraction; a leader with
 *              s_j < floor stops being one.
 *   out        out[OUT0 + k * NC + j] receives the bits of s_j, except that a candidate that is not a leader becomes -inf.  NaN stays
 *              NaN, -inf stays -inf, and a column whose key is outside [0, cap) is copied unchanged.
 *   leaders    (when given) row i of leaders [sum NW, top] int32 holds the columns j of the row's leaders in ascending order, padded
 *              with CFCT_NONE; n_leaders [sum NW] int32 their number.  Rows in table order, then window order.
 * A key outside [0, cap) is never dereferenced; nothing here is dereferenced by key at all.
 *
 * One launch: one 256-thread workgroup per (table row, window) -- the row's scores as order-preserving keys into `work`, the row maximum,
 * the R-th largest key by four radix passes over per-wave histograms in LDS, the demoted plane, and a scan that restores the leaders in
 * ascending column order.  No workgroup waits on another; a leader's place is a prefix sum; the one atomic is the histogram count in
 * LDS, whose sums do not depend on their order: two runs give identical bytes.  `work` holds cfct_workspace_words(NOUT) uint32.
 *
 * Conventions (as include/ext/clipfsar_events.h): the library allocates no device memory and owns no stream, all work is enqueued on
 * `stream` (a hipStream_t) of the CURRENT device; return 0 = success, non-zero = error with the message in cfct_last_error()
 * (thread-local).  Every pointer is a DEVICE pointer owned by the caller except `table_host`, the HOST copy of the S rows, which the entry
 * point validates before it touches the device; `table_dev` is the device copy the caller uploaded on `stream` before the call.
 */
#ifndef CLIPFSAR_CONTEST_H
#define CLIPFSAR_CONTEST_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* Built with -fvisibility=hidden: exactly the entry points declared between this push and the pop are exported
 * (tests/test_contest_abi.py compares `nm -D` with this file). */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

typedef void* cfct_stream_t;

#define CFCT_ABI_VERSION 1
#define CFCT_MAX_STREAMS 65536
#define CFCT_TABLE_COLS 6
#define CFCT_SLOT 0
#define CFCT_NW 1
#define CFCT_OUT0 2
#define CFCT_NC 3
#define CFCT_KEY0 4
#define CFCT_CHUNK0 5
#define CFCT_NONE 0x7fffffff /* the padding of a leader list */
int cfct_version(void);
int cfct_abi_version(void);
const char* cfct_last_error(void);

/* uint32 elements of `work` for a plane of NOUT scores: NOUT, a key per score; -1 when NOUT < 0 */
int cfct_workspace_words(int NOUT);

/* ---- the contest.  scores is flat, NOUT floats (the sum of NW * NC over the table; 0: nothing is launched) and is only read; out is
 * flat, NOUT floats, and must not overlap scores.  leaders and n_leaders are both NULL or both given.  keys == NULL: every column
 * competes, and NKEYS, KEY0 and cap are ignored.  1 <= S <= 65536, NOUT >= 0, top >= 1; with keys: NKEYS >= 1, cap >= 1 and
 * KEY0 + NC <= NKEYS in every row; with has_margin: margin finite and >= 0. */
int cfct_contest(const float* scores, const int32_t* keys, float* out, int32_t* leaders, int32_t* n_leaders, uint32_t* work,
                 const int32_t* table_host, const int32_t* table_dev, int S, int NOUT, int NKEYS, int cap, int top, int has_margin,
                 float margin, cfct_stream_t stream);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* CLIPFSAR_CONTEST_H */
