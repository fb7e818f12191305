/*
 * clipfsar_ledger.h -- C ABI of libclipfsar_ledger.so: the per-shot store of a live gallery with a ledger
 * (clip_fsar_amd.live_gallery.LiveGallery(ledger=ShotLedger(...)), clip_fsar_amd.ledger) for CLIP-FSAR (gfx950 / CDNA4).  A live
 * gallery keeps one running fp32 sum per class (include/clipfsar_live.h, cfsl_accumulate) and nothing of the single shots; the ledger
 * keeps every shot's ADDEND -- exactly the rows cfsl_accumulate summed for it -- in a store [shots, rows_kept, E] fp32, so that a
 * class's sum can be formed again from the addends that remain, in their order, bit for bit.  The library keeps no state.
 *
 * cfld_put    X [Nv, L, E]: the first rows_kept rows of video v go to store[slots[v]]; slots [Nv] int32 on the DEVICE.  A slot outside
 *             [0, shots) writes nothing.  The slots of one call must differ (the host planner hands out free slots): every store word has
 *             one writer.  One wave per row, 16-byte accesses.
 * cfld_resum  the DESCRIPTOR TABLE has one row of CFLD_TABLE_COLS int32 per touched class: SLOT (its slot of the gallery's store),
 *             FIRST and N: its addends are store[list[FIRST]], ..., store[list[FIRST + N - 1]], in that order; list [n_list] int32 on the
 *             DEVICE.  Per kept row r and element e, cfsl_accumulate's operation order with prior = 0:
 *                 a = 0; for i in list[FIRST : FIRST + N]: a += store[i][r][e]; sums[SLOT][r][e] = a; means[.][r][e] = a * (1.0f / (float)N)
 *             means is [cap, rows_kept, E] at the rows' slots with means_by_slot, else [S, rows_kept, E] in table order.  One workgroup
 *             per (table row, kept row).  The host refuses N < 1, a SLOT outside [0, cap) or twice in the table, and a FIRST that is
 *             not the running sum of the N before it (their total: n_list); the kernel writes nothing for a row the host would have
 *             refused, nor for one whose list names a ledger slot outside [0, shots).
 * cfld_fit    the same table and list.  For list position p of table row s, with x = store[list[p]] and, per element,
 *             m = sums[SLOT][r] - x[r] (one fp32 subtraction), the cosine of row r < T is
 *                 dot(x[r], m) / sqrtf(dot(x[r], x[r]) * dot(m, m)),
 *             each dot a lane-strided fmaf chain over 16-byte pieces (lane l: elements 4 l .. 4 l + 3, then + 256) closed by a wave
 *             sum; fit[p] is the T cosines summed in row order by one lane, times 1.0f / (float)T.  A class of N = 1 gives NaN, and so
 *             does a row of a zero x or m (0 / 0).  One workgroup per list position, its waves taking the rows in turn; no atomics:
 *             two runs give identical bytes.  A position whose row the host would have refused, or whose ledger slot lies outside
 *             [0, shots), is left alone.
 *
 * Conventions (as include/ext/clipfsar_history.h): the library allocates no device memory and owns no stream, all work is enqueued on
 * `stream` (a hipStream_t) of the CURRENT device; return 0 = success, non-zero = error with the message in cfld_last_error()
 * (thread-local).  Every pointer is a DEVICE pointer owned by the caller except `table_host`, the HOST copy of the S rows, which the
 * entry point validates before it touches the device; `table_dev` is the device copy the caller uploaded on `stream` before the call.
 * E % 4 == 0 and every float buffer is 16-byte aligned.
 */
#ifndef CLIPFSAR_LEDGER_H
#define CLIPFSAR_LEDGER_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* Built with -fvisibility=hidden: exactly the entry points declared between this push and the pop are exported
 * (tests/test_ledger_abi.py compares `nm -D` with this file). */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

typedef void* cfld_stream_t;

#define CFLD_ABI_VERSION 1
#define CFLD_MAX_ROWS 65536
#define CFLD_MAX_T 32
#define CFLD_TABLE_COLS 3
#define CFLD_SLOT 0
#define CFLD_FIRST 1
#define CFLD_N 2
int cfld_version(void);
int cfld_abi_version(void);
const char* cfld_last_error(void);

/* ---- addends into the store.  Nv, L >= 1, 1 <= rows_kept <= L, shots >= 1, E >= 4 and E % 4 == 0, Nv * rows_kept < 2^31; X and
 * store do not overlap. */
int cfld_put(const float* X, float* store, const int32_t* slots, int Nv, int L, int E, int shots, int rows_kept, cfld_stream_t stream);

/* ---- the touched classes' sums and means from their remaining addends.  store [shots, rows_kept, E], sums [cap, L, E] (rows
 * 0 .. rows_kept - 1 are written), 1 <= S <= min(65536, cap), n_list >= 1, 1 <= rows_kept <= L, E >= 1. */
int cfld_resum(const float* store, const int32_t* list, float* sums, float* means, const int32_t* table_host, const int32_t* table_dev,
               int S, int n_list, int shots, int rows_kept, int L, int E, int cap, int means_by_slot, cfld_stream_t stream);

/* ---- leave-one-out agreement.  store [shots, rows_kept, E], sums [cap, L, E] are only read; fit [n_list].  1 <= T <= min(32,
 * rows_kept), E >= 4 and E % 4 == 0; the table as for cfld_resum. */
int cfld_fit(const float* store, const float* sums, const int32_t* list, float* fit, const int32_t* table_host, const int32_t* table_dev,
             int S, int n_list, int shots, int rows_kept, int L, int T, int E, int cap, cfld_stream_t stream);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* CLIPFSAR_LEDGER_H */
