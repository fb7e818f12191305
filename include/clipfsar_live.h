/*
 * clipfsar_live.h -- C ABI of libclipfsar_live.so: the device side of a class gallery whose classes come, go and receive further shots
 * (clip_fsar_amd.live_gallery.LiveGallery) for CLIP-FSAR (gfx950 / CDNA4).
 *
 * include/clipfsar_gallery.h scores against a dense P [C, T, E]: the column order is the memory order, so a class can neither leave nor
 * be scored apart.  Here the prototypes live in a STORE of `cap` slots, P_store [cap, T, E] with norms pn_store [cap * T], and a column
 * is a slot number: column j of a call is slot cols[j].  Removing a class edits the column list, a subset is another list, and further
 * shots update one slot in place.
 *
 * Conventions (as include/clipfsar_gallery.h): the library allocates no memory and owns no stream, all work is enqueued on `stream` (a
 * hipStream_t) of the CURRENT device; return 0 = success, non-zero = error with the message in cfsl_last_error() (thread-local).  All
 * tensors are fp32 row-major.  Every pointer is a DEVICE pointer owned by the caller, WITH ONE EXCEPTION (as include/clipfsar_pool.h):
 * a DESCRIPTOR TABLE is passed twice -- `table_host`, a HOST pointer to the S rows, which the entry point reads and validates before it
 * touches the device, and `table_dev`, the device copy of the same rows that the caller uploaded on `stream` before the call, which
 * the kernel reads.  The host rows need to stay valid only for the duration of the call.  A table has one row of CFSL_TABLE_COLS int32
 * per updated class:
 *
 *   [CFSL_SLOT]   store slot of the class, 0 <= slot < cap, at most once per table
 *   [CFSL_OFF]    first video of the class's run in X: the sum of n over the rows before
 *   [CFSL_N]      videos in the run, >= 1
 *   [CFSL_PRIOR]  videos already summed into sums[slot], >= 0; 0: the sum starts at zero, whatever the slot held
 */
#ifndef CLIPFSAR_LIVE_H
#define CLIPFSAR_LIVE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* Built with -fvisibility=hidden: exactly the entry points declared between this push and the pop are exported
 * (tests/test_live_abi.py compares `nm -D` with this file). */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

typedef void* cfsl_stream_t;

/* library version (major*10000 + minor*100 + patch), ABI revision (bumped whenever an exported signature or the table layout changes)
 * and the last error text of the calling thread */
#define CFSL_ABI_VERSION 1
#define CFSL_MAX_T 32
#define CFSL_MAX_ROWS 65536
#define CFSL_TABLE_COLS 4
#define CFSL_SLOT 0
#define CFSL_OFF 1
#define CFSL_N 2
#define CFSL_PRIOR 3
int cfsl_version(void);
int cfsl_abi_version(void);
const char* cfsl_last_error(void);

/* ---- cos_sim + OTAM of every (query, column) pair, column j = slot cols[j] of the store: cfsg_otam_gallery's arithmetic
 * (include/clipfsar_gallery.h) on P_store[cols], bit for bit, without the copy:
 *     d = 1 - Xq P^T / (qn pn^T + 0.01),   logits[q, j] = -(OTAM(d_qj) + OTAM(d_qj^T)),   the second term 0 with single_direct.
 * Xq [NQ, T, E], qn [NQ*T], P_store [cap, T, E], pn_store [cap*T], cols [C] int32 (DEVICE), logits [NQ, C].  1 <= T <= 32,
 * E % 4 == 0, 4 <= E <= 8192, C >= 1, cap >= 1, cap * T and NQ * T below 2^31.  cols is device data: a slot outside [0, cap) is never
 * dereferenced and gives a column of NaN (the host validates the list).  Slots that cols does not name are not read.  Xq and P_store
 * are read as float4: both must be 16-byte aligned (a pointer that is not is refused before any launch). */
int cfsl_otam_indexed(const float* Xq, const float* qn, const float* P_store, const float* pn_store, const int32_t* cols, float* logits,
                      int NQ, int C, int cap, int T, int E, float lambda, int single_direct, cfsl_stream_t stream);

/* ---- further videos into the running sums of their classes, ragged over classes, one launch.  For row s of the table, kept row
 * r < rows_kept and column e:
 *     a = prior_s ? sums[slot_s, r, e] : 0;   for v = off_s .. off_s + n_s - 1:  a += X[v, r, e];   sums[slot_s, r, e] = a;
 *     mean = a * (1.0f / (prior_s + n_s))
 * -- cfsg_segment_mean's operation order, continued: a sum built over several calls has the bits of one cfsg_segment_mean over all the
 * videos.  X [Nv, L, E], sums [cap, L, E] (rows >= rows_kept are left alone), 1 <= rows_kept <= L.  means_by_slot != 0: means is
 * [cap, rows_kept, E] and the mean goes to means[slot_s] (the prototype store when rows_kept = T); 0: means is [S, rows_kept, E],
 * packed in table order.  Slots the table does not name are left alone.  The runs must be the prefix sums of n and end at Nv. */
int cfsl_accumulate(const float* X, float* sums, float* means, const int32_t* table_host, const int32_t* table_dev, int S, int Nv, int L,
                    int E, int cap, int rows_kept, int means_by_slot, cfsl_stream_t stream);

/* ---- L2 norms of the rows of the table's slots: pn_store[slot_s * T + t] = |P_store[slot_s, t]|, the bits of cfsg_row_norms on those
 * rows.  Only CFSL_SLOT of the table is read.  P_store [cap, T, E], pn_store [cap * T]. */
int cfsl_slot_norms(const float* P_store, float* pn_store, const int32_t* table_host, const int32_t* table_dev, int S, int cap, int T,
                    int E, cfsl_stream_t stream);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* CLIPFSAR_LIVE_H */
