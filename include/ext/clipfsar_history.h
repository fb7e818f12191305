/*
 * clipfsar_history.h -- C ABI of libclipfsar_history.so: the peak search of a stream pool with a history
 * (clip_fsar_amd.pool.StreamPool(history=History(frames=F)), StreamPool.search) for CLIP-FSAR (gfx950 / CDNA4).  The pool keeps every
 * session's tower rows in a store that outlives its ring, gathers the windows the store still holds (cfsp_window_sequences of
 * include/clipfsar_pool.h, the store as its ring) and scores them against a handful of classes; this library turns that score plane
 * into what a person reads: per class, the best occurrences across all sessions that do not overlap.  It keeps no state.
 *
 * The DESCRIPTOR TABLE is exactly the pool's (include/clipfsar_pool.h): one row of CFHS_TABLE_COLS int32 per searched session -- SLOT,
 * PUT_POS, N, FEAT_OFF, WIN_POS, NW, WIN_OFF, HAS_STATE -- so that the table the gather was given, host rows and device copy, is
 * passed on unchanged.  Only NW and WIN_OFF are read here: session row r owns the plane's rows WIN_OFF .. WIN_OFF + NW - 1, its
 * windows in ascending order.  A row of NW = 0 windows touches nothing.
 *
 * THE RULE.  scores is the plane [NW, K] fp32, row-major: K classes per window.  Per class k and session row r, with
 * s_j = scores[(WIN_OFF + j) * K + k], j = 0 .. NW_r - 1:
 *   candidate  s_j is not NaN and s_j > -inf and, with has_min, s_j >= min_score (an fp32 comparison).
 *   order      a larger float ranks higher; -0.0 and +0.0 are equal.
 *   peak       candidate j is a peak when no candidate v of the same row and class with 0 < |v - j| <= separation beats it; v beats
 *              j with a higher score, or with an equal score and v < j.  A local-maximum filter, not greedy suppression: a plateau
 *              yields its first window only, and rows never see each other's windows.
 *   hits       per class the `top` highest peaks over all rows; a tie at the last place goes to the lower plane row.
 * hit_rows [K, top] int32: the kept plane rows of class k in ASCENDING order, then CFHS_NONE; hit_scores [K, top] fp32: the bits
 * scores holds at (row, k), then 0; n_hits [K] int32: how many places are filled; n_peaks [K] int32: the class's peaks before `top`
 * cut them.
 *
 * Two launches.  history_peaks_kernel: a 256-thread workgroup per tile of 256 windows of one (row, class) stages the tile and
 * `separation` windows of halo on each side, clipped to the row, as order-preserving keys in LDS, applies the peak rule and writes
 * work[k * NW + n], the key of a peak or 0 -- transposed, so that the second kernel reads a class contiguously.  history_hits_kernel:
 * one 256-thread workgroup per class counts the peaks, finds the top-th largest key by four radix passes over per-wave histograms
 * in LDS and compacts the kept rows by prefix sums in ascending row order.  No workgroup waits on another; the one atomic is the
 * histogram count in LDS, whose sums do not depend on their order: two runs give identical bytes.  `work` holds
 * cfhs_workspace_words(NW, K) uint32 and must not overlap the plane or an output.
 *
 * Conventions (as include/ext/clipfsar_contest.h): the library allocates no device memory and owns no stream, all work is enqueued on
 * `stream` (a hipStream_t) of the CURRENT device; return 0 = success, non-zero = error with the message in cfhs_last_error()
 * (thread-local).  Every pointer is a DEVICE pointer owned by the caller except `table_host`, the HOST copy of the S rows, which the entry
 * point validates before it touches the device; `table_dev` is the device copy the caller uploaded on `stream` before the call.
 */
#ifndef CLIPFSAR_HISTORY_H
#define CLIPFSAR_HISTORY_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* Built with -fvisibility=hidden: exactly the entry points declared between this push and the pop are exported
 * (tests/test_history_abi.py compares `nm -D` with this file). */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

typedef void* cfhs_stream_t;

#define CFHS_ABI_VERSION 1
#define CFHS_MAX_STREAMS 65536
#define CFHS_TABLE_COLS 8
#define CFHS_SLOT 0
#define CFHS_PUT_POS 1
#define CFHS_N 2
#define CFHS_FEAT_OFF 3
#define CFHS_WIN_POS 4
#define CFHS_NW 5
#define CFHS_WIN_OFF 6
#define CFHS_HAS_STATE 7
#define CFHS_MAX_CLASSES 64
#define CFHS_MAX_TOP 4096
#define CFHS_MAX_SEPARATION 4096
#define CFHS_NONE 0x7fffffff /* an unused place of hit_rows */
int cfhs_version(void);
int cfhs_abi_version(void);
const char* cfhs_last_error(void);

/* uint32 elements of `work` for a plane of NW windows and K classes: NW * K, a key per score; -1 when NW < 0, K < 1 or the product
 * is above 2^30 */
int cfhs_workspace_words(int NW, int K);

/* ---- the peaks and hits.  scores [NW, K] is only read (NW = 0: the table is validated and nothing is launched).
 * 1 <= S <= 65536, NW >= 0 and the sum of the table's NW, WIN_OFF their running sum, 1 <= K <= 64, NW * K <= 2^30,
 * 0 <= separation <= 4096, 1 <= top <= 4096; with has_min: min_score is not NaN. */
int cfhs_peaks(const float* scores, uint32_t* work, int32_t* hit_rows, float* hit_scores, int32_t* n_hits, int32_t* n_peaks,
               const int32_t* table_host, const int32_t* table_dev, int S, int NW, int K, int separation, int has_min, float min_score,
               int top, cfhs_stream_t stream);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* CLIPFSAR_HISTORY_H */
