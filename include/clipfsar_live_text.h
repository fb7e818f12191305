/*
 * clipfsar_live_text.h -- C ABI of libclipfsar_live_text.so: the EVAL_TEXT and COMBINE eval branches over a RAGGED LIST of (queries x
 * classes) rectangles, the classes named by slot lists over one text-row store
 * (clip_fsar_amd.live_text_gallery.LiveTextGallery) for CLIP-FSAR (gfx950 / CDNA4).
 *
 * include/clipfsar_gallery_text.h scores ONE dense rectangle: every query against text[0 .. C).  Both branches end in a softmax over the
 * classes, so "these N of the stored classes" is not a column slice of that call: the softmax has to run over the list.  Here a call
 * holds G GROUPS as include/clipfsar_groups.h's: group g is NQ_g consecutive queries and its own list of NC_g store slots; the lists lie
 * one after the other in `cols`, may overlap and may differ in length; the output is flat, group g owning the row-major [NQ_g, NC_g]
 * block at OUT0_g.  Every logit and every EVAL_TEXT probability is what cfgt_text_logits / cfgt_text_softmax give on the dense matrix
 * text_store[cols_g], bit for bit; COMBINE is cfgt_text_combine's formula over the group's row (bit for bit where both rows split into
 * float4 alike: every NC a multiple of 4).
 *
 * Conventions (as include/clipfsar_groups.h): the library allocates no memory and owns no stream, all work is enqueued on `stream` (a
 * hipStream_t) of the CURRENT device; return 0 = success, non-zero = error with the message in cflt_last_error() (thread-local).  All
 * tensors are fp32 row-major.  Every pointer is a DEVICE pointer owned by the caller, WITH ONE EXCEPTION: the DESCRIPTOR TABLE is passed
 * twice -- `table_host`, a HOST pointer to the G rows, which the entry point reads and validates before it touches the device, and
 * `table_dev`, the device copy of the same rows that the caller uploaded on `stream` before the call, which the kernels read.  The host
 * rows need to stay valid only for the duration of the call.  A table has one row of CFLT_TABLE_COLS int32 per group:
 *
 *   [CFLT_Q0]     first query of the group: the sum of NQ over the rows before
 *   [CFLT_NQ]     queries of the group, >= 0 (a group without queries owns no tile, no output and no partials)
 *   [CFLT_C0]     offset of the group's slot list in cols: the sum of NC over the rows before
 *   [CFLT_NC]     slots in the list, >= 1
 *   [CFLT_TILE0]  tiles before this group: the sum of ceil(NQ / 64) * ceil(NC / 64) over the rows before (a tile is 64 queries x 64
 *                 classes, one row per query and per class)
 *   [CFLT_OUT0]   offset of the group's block in the output: the sum of NQ * NC over the rows before
 *   [CFLT_PART0]  the group's first softmax partial, in (max, sum) pairs: the sum of NQ * ceil(NC / 64) over the rows before
 *   [CFLT_PAD]    0
 *
 * The running sums must end at NQ, NCOLS, the grid size, NOUT and NPART, and all of them stay below 2^31.
 */
#ifndef CLIPFSAR_LIVE_TEXT_H
#define CLIPFSAR_LIVE_TEXT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* Built with -fvisibility=hidden: exactly the entry points declared between this push and the pop are exported
 * (tests/test_live_text_abi.py compares `nm -D` with this file). */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

typedef void* cflt_stream_t;

/* library version (major*10000 + minor*100 + patch), ABI revision (bumped whenever an exported signature or the table layout changes)
 * and the last error text of the calling thread */
#define CFLT_ABI_VERSION 1
#define CFLT_MAX_GROUPS 65536
#define CFLT_TABLE_COLS 8
#define CFLT_Q0 0
#define CFLT_NQ 1
#define CFLT_C0 2
#define CFLT_NC 3
#define CFLT_TILE0 4
#define CFLT_OUT0 5
#define CFLT_PART0 6
#define CFLT_PAD 7
int cflt_version(void);
int cflt_abi_version(void);
const char* cflt_last_error(void);

/* ---- size in floats of the softmax-partials workspace of a table: 2 * NPART, 2 per (query, 64-class tile of its group).  Returns -1
 * for a null table, G outside 1 .. CFLT_MAX_GROUPS, a negative NQ, an NC < 1 or a size beyond 2^31 - 1.  Reads the counts alone. */
int cflt_workspace_floats(const int32_t* table_host, int G);

/* ---- zero-shot text logits of every group, one launch: for group g, query i < NQ_g and column j < NC_g
 *     logits[OUT0_g + i * NC_g + j] = scale[0] * (dot(emb[Q0_g + i], text_store[s]) / en[Q0_g + i] / tn_store[s]),  s = cols[C0_g + j]
 * cfgt_text_logits' operation order (include/clipfsar_gallery_text.h).  emb [NQ, E], en [NQ], text_store [cap, E], tn_store [cap],
 * cols [NCOLS] int32 (DEVICE), scale [1] (device), logits [NOUT].  partials [2 * NPART] receives (max, sum of expf(x - max)) of every
 * (query, 64-class tile of its group) at 2 * (PART0_g + i * ceil(NC_g / 64) + tile).  E % 4 == 0, 4 <= E <= 8192, NQ >= 1, cap >= 1,
 * 1 <= G <= CFLT_MAX_GROUPS; emb and text_store 16-byte aligned.
 * cols is device data: a slot outside [0, cap) is never dereferenced -- its row is staged as zeros and its norm is NaN, so that
 * column's logit is NaN (the host validates the lists).  Slots that no list names are not read; logits outside [0, NOUT) and partials
 * outside [0, 2 * NPART) are not written.
 * One 256-thread workgroup per tile; inside a group the class tile is the fastest index. */
int cflt_text_logits_grouped(const float* emb, const float* en, const float* text_store, const float* tn_store, const int32_t* cols,
                             const float* scale, float* logits, float* partials, const int32_t* table_host, const int32_t* table_dev,
                             int G, int NQ, int NCOLS, int NOUT, int NPART, int cap, int E, cflt_stream_t stream);

/* ---- softmax over the group's classes of every query row: cfgt_text_softmax per group.  logits and partials as written by
 * cflt_text_logits_grouped under the same table; probs [NOUT] may be logits (in place).  One workgroup per query. */
int cflt_text_softmax_grouped(const float* logits, const float* partials, float* probs, const int32_t* table_host,
                              const int32_t* table_dev, int G, int NQ, int NOUT, int NPART, cflt_stream_t stream);

/* ---- COMBINE fusion per group: out = p^coff * softmax_c((8 + v) / 8)^(1 - coff), both softmaxes over the group's NC_g classes
 * (cfgt_text_combine's formula).  visual [NOUT]: the OTAM logits in the layout cfgr_otam_grouped (include/clipfsar_groups.h) writes for
 * the same groups, with the same OUT0.  out [NOUT] may be logits (in place); coff finite.  One workgroup per query. */
int cflt_text_combine_grouped(const float* logits, const float* partials, const float* visual, float* out, const int32_t* table_host,
                              const int32_t* table_dev, int G, int NQ, int NOUT, int NPART, float coff, cflt_stream_t stream);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* CLIPFSAR_LIVE_TEXT_H */
