/*
 * clipfsar_groups.h -- C ABI of libclipfsar_groups.so: cos_sim + OTAM and top-k of a RAGGED LIST of (queries x classes) rectangles over one
 * packed query matrix and one prototype store, in one launch each (clip_fsar_amd.live_gallery.LiveGallery.classify_grouped, the
 * per-session class lists of clip_fsar_amd.pool.StreamPool) for CLIP-FSAR (gfx950 / CDNA4).
 *
 * include/clipfsar_live.h scores ONE rectangle: every query of a call against the same column list.  Here a call holds G GROUPS: group g
 * is NQ_g consecutive queries and its own list of NC_g store slots -- a tenant's classes, an episode's N ways.  The lists lie one after
 * the other in `cols`, may overlap and may differ in length; the logits are flat, group g owning the row-major [NQ_g, NC_g] block at
 * OUT0_g.  Every element is what cfsl_otam_indexed gives for that group's queries and list, bit for bit.
 *
 * Conventions (as include/clipfsar_live.h): the library allocates no memory and owns no stream, all work is enqueued on `stream` (a
 * hipStream_t) of the CURRENT device; return 0 = success, non-zero = error with the message in cfgr_last_error() (thread-local).  All
 * tensors are fp32 row-major.  Every pointer is a DEVICE pointer owned by the caller, WITH ONE EXCEPTION (as include/clipfsar_pool.h):
 * the DESCRIPTOR TABLE is passed twice -- `table_host`, a HOST pointer to the G rows, which the entry point reads and validates before it
 * touches the device, and `table_dev`, the device copy of the same rows that the caller uploaded on `stream` before the call, which
 * the kernel reads.  The host rows need to stay valid only for the duration of the call.  A table has one row of CFGR_TABLE_COLS int32
 * per group:
 *
 *   [CFGR_Q0]     first query of the group: the sum of NQ over the rows before
 *   [CFGR_NQ]     queries of the group, >= 0 (a group without queries owns no tile and no logits)
 *   [CFGR_C0]     offset of the group's slot list in cols: the sum of NC over the rows before
 *   [CFGR_NC]     slots in the list, >= 1
 *   [CFGR_TILE0]  tiles before this group: the sum of ceil(NQ / QB) * ceil(NC / QB) over the rows before, QB = min(64 / T, 16) videos
 *   [CFGR_OUT0]   offset of the group's block in logits: the sum of NQ * NC over the rows before
 *
 * The running sums must end at NQ, NCOLS, the grid size and NOUT, and all of them stay below 2^31.
 */
#ifndef CLIPFSAR_GROUPS_H
#define CLIPFSAR_GROUPS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* Built with -fvisibility=hidden: exactly the entry points declared between this push and the pop are exported
 * (tests/test_groups_abi.py compares `nm -D` with this file). */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

typedef void* cfgr_stream_t;

/* library version (major*10000 + minor*100 + patch), ABI revision (bumped whenever an exported signature or the table layout changes)
 * and the last error text of the calling thread */
#define CFGR_ABI_VERSION 1
#define CFGR_MAX_T 32
#define CFGR_MAX_GROUPS 65536
#define CFGR_TOPK_MAX 16
#define CFGR_TABLE_COLS 6
#define CFGR_Q0 0
#define CFGR_NQ 1
#define CFGR_C0 2
#define CFGR_NC 3
#define CFGR_TILE0 4
#define CFGR_OUT0 5
int cfgr_version(void);
int cfgr_abi_version(void);
const char* cfgr_last_error(void);

/* ---- cos_sim + OTAM of every group's (query, column) pairs, one launch: for group g, query i < NQ_g and column j < NC_g
 *     logits[OUT0_g + i * NC_g + j] = cfsl_otam_indexed's logit of query Q0_g + i against slot cols[C0_g + j]
 * (include/clipfsar_live.h: d = 1 - Xq P^T / (qn pn^T + 0.01), -(OTAM(d) + OTAM(d^T)), the second term 0 with single_direct).
 * Xq [NQ, T, E], qn [NQ*T], P_store [cap, T, E], pn_store [cap*T], cols [NCOLS] int32 (DEVICE), logits [NOUT].  1 <= T <= 32,
 * E % 4 == 0, 4 <= E <= 8192, NQ >= 1, cap >= 1, 1 <= G <= CFGR_MAX_GROUPS; cap * T, NQ * T, NCOLS, NOUT and the tile count below 2^31.
 * cols is device data: a slot outside [0, cap) is never dereferenced and gives a column of NaN in its group (the host validates the
 * lists).  Slots that no list names are not read; logits outside [0, NOUT) are not written.  Xq and P_store are read as float4: both
 * must be 16-byte aligned (a pointer that is not is refused before any launch).
 * One 256-thread workgroup per tile of QB x QB (query, column) pairs; inside a group the column tile is the fastest index. */
int cfgr_otam_grouped(const float* Xq, const float* qn, const float* P_store, const float* pn_store, const int32_t* cols, float* logits,
                      const int32_t* table_host, const int32_t* table_dev, int G, int NQ, int NCOLS, int NOUT, int cap, int T, int E,
                      float lambda, int single_direct, cfgr_stream_t stream);

/* ---- top-k of every query's row of its group's block: cfsg_topk's rule (include/clipfsar_gallery.h) -- descending, ties to the lower
 * index, NaN and -inf never selected -- with the index counting within the group's own list.  logits [NOUT] as cfgr_otam_grouped wrote
 * it, values [NQ, k] fp32, index [NQ, k] int32.  1 <= k <= min(CFGR_TOPK_MAX, the smallest NC of a group with queries); such a group's
 * NC is at most 65535.  Only CFGR_Q0, CFGR_NQ, CFGR_NC and CFGR_OUT0 of the device rows are read; of the host rows everything but
 * CFGR_TILE0 (which depends on T) is validated as above, the sums ending at NQ and NOUT. */
int cfgr_topk_grouped(const float* logits, const int32_t* table_host, const int32_t* table_dev, int G, int NQ, int NOUT, int k,
                      float* values, int32_t* index, cfgr_stream_t stream);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* CLIPFSAR_GROUPS_H */
