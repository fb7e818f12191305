/*
 * clipfsar_gallery.h -- C ABI of libclipfsar_gallery.so: the support gallery of CLIP-FSAR (gfx950 / CDNA4).
 *
 * A gallery stores class prototypes once and classifies any number of query videos against all of them.  In the reference's eval
 * branch (few_shot.py:2944-2990) queries and supports meet only in cos_sim and OTAM, and a prototype depends on its own class's
 * supports alone, so stored prototypes give exactly an episode's logits.  The entry points below are the gallery-only pieces; the
 * towers and context2 run on libclipfsar_hip.so.
 *
 * Conventions (as include/clipfsar_hip.h): every pointer is a DEVICE pointer owned by the caller, the library allocates no device
 * memory and owns no stream, all work is enqueued on `stream` (a hipStream_t) of the CURRENT device; return 0 = success, non-zero =
 * error with the message in cfsg_last_error() (thread-local).  Every entry point validates its arguments before it touches the device.
 * All tensors are fp32 row-major unless stated otherwise.
 */
#ifndef CLIPFSAR_GALLERY_H
#define CLIPFSAR_GALLERY_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* Built with -fvisibility=hidden: exactly the entry points declared between this push and the pop are exported
 * (tests/test_gallery_abi.py compares `nm -D` with this file). */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

typedef void* cfsg_stream_t;

/* library version (major*10000 + minor*100 + patch), ABI revision (bumped whenever an exported signature changes or is added) and the
 * last error text of the calling thread */
#define CFSG_ABI_VERSION 1
int cfsg_version(void);
int cfsg_abi_version(void);
const char* cfsg_last_error(void);

/* ---- support sequences (few_shot.py:2946, :2955): X[v] = [feats[v, 0..T-1]; text[cls_of_video[v]]].
 * feats [Nv, T, E], text [n_cls, E], cls_of_video [Nv] int32, X [Nv, T+1, E].  Any Nv, any number of videos per class.  A class id
 * outside [0, n_cls) poisons the text row with NaN (the host validates the ids). */
int cfsg_support_sequences(const float* feats, const float* text, const int32_t* cls_of_video, float* X, int Nv, int T, int E,
                           int n_cls, cfsg_stream_t stream);

/* ---- per-class mean over a contiguous run of videos (few_shot.py:2949-2962): out[c, r] = (sum over v in [offsets[c], offsets[c+1])
 * of X[v, r]) * (1 / count), summed in video order like cfsar_prototypes.  X [Nv, L, E], offsets [C+1] int32 (device), rows
 * 0 .. rows_kept-1 of each video (rows_kept <= L), out [C, rows_kept, E].  An empty or out-of-range run gives a NaN row. */
int cfsg_segment_mean(const float* X, const int32_t* offsets, float* out, int Nv, int L, int E, int C, int rows_kept,
                      cfsg_stream_t stream);

/* ---- L2 norm of every row: n[r] = |X[r]|.  X [R, E], n [R]. */
int cfsg_row_norms(const float* X, float* n, int R, int E, cfsg_stream_t stream);

/* ---- cos_sim + OTAM of every (query, class) pair (few_shot.py:1115-1124, 2657-2687, 2970-2990):
 *     d = 1 - Xq P^T / (qn pn^T + 0.01)      (eps added to the product of the norms, rows not pre-normalised),
 *     logits[q, c] = -(OTAM(d_qc) + OTAM(d_qc^T)),   the second term 0 with single_direct.
 * Xq [NQ, T, E], qn [NQ*T] (cfsg_row_norms of Xq), P [C, T, E], pn [C*T], logits [NQ, C]; dists_out (optional, may be NULL)
 * [NQ, C, T, T].  The similarities are an exact-fp32 MFMA GEMM (k-ordered fmaf chains); T <= 32, E % 4 == 0, 4 <= E <= 8192.  Xq and P
 * are read as float4: both must be 16-byte aligned (a pointer that is not is refused before any launch). */
int cfsg_otam_gallery(const float* Xq, const float* qn, const float* P, const float* pn, float* logits, float* dists_out, int NQ,
                      int C, int T, int E, float lambda, int single_direct, cfsg_stream_t stream);

/* ---- top-k per query: values [NQ, k] (descending), index [NQ, k] int32 class indices; ties go to the lower class index (the order of
 * a stable descending sort).  logits [NQ, C]; 1 <= k <= 16, k <= C <= 65535.  A NaN logit (a poisoned column of cfsl_otam_indexed) is
 * never selected, and neither is a logit of -inf.  A row with fewer than k selectable classes fills its remaining places with the value
 * -inf and the index 0x7fffffff (no class). */
int cfsg_topk(const float* logits, float* values, int32_t* index, int NQ, int C, int k, cfsg_stream_t stream);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* CLIPFSAR_GALLERY_H */
