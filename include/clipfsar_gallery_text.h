/*
 * clipfsar_gallery_text.h -- C ABI of libclipfsar_gallery_text.so: the text half of the support gallery of CLIP-FSAR (gfx950 / CDNA4).
 *
 * The EVAL_TEXT (few_shot.py:2835-2852) and COMBINE (:2855-2930) eval branches at any number of registered classes: the zero-shot
 * text logits scale * cos(mean_T query features, class text row) as one exact-fp32 MFMA GEMM, the softmax over the classes, and the
 * fusion of the text probabilities with the gallery's OTAM logits.  The row norms come from cfsg_row_norms and the OTAM logits from
 * cfsg_otam_gallery (include/clipfsar_gallery.h); the towers and context2 run on libclipfsar_hip.so.
 *
 * Conventions (as include/clipfsar_gallery.h): every pointer is a DEVICE pointer owned by the caller, the library allocates no device
 * memory and owns no stream, all work is enqueued on `stream` (a hipStream_t) of the CURRENT device; return 0 = success, non-zero =
 * error with the message in cfgt_last_error() (thread-local).  Every entry point validates its arguments before it touches the device.
 * All tensors are fp32 row-major.
 */
#ifndef CLIPFSAR_GALLERY_TEXT_H
#define CLIPFSAR_GALLERY_TEXT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* Built with -fvisibility=hidden: exactly the entry points declared between this push and the pop are exported
 * (tests/test_gallery_text_abi.py compares `nm -D` with this file). */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

typedef void* cfgt_stream_t;

/* library version (major*10000 + minor*100 + patch), ABI revision (bumped whenever an exported signature changes or is added) and the
 * last error text of the calling thread */
#define CFGT_ABI_VERSION 1
int cfgt_version(void);
int cfgt_abi_version(void);
const char* cfgt_last_error(void);

/* ---- mean over the frames (few_shot.py:2838-2841): out[n, e] = (sum over t, in t order, of feats[n, t, e]) / T.
 * feats [N, T, E], out [N, E]; 1 <= T <= 1024. */
int cfgt_frame_mean(const float* feats, float* out, int N, int T, int E, cfgt_stream_t stream);

/* ---- size in floats of the softmax-partials workspace of cfgt_text_logits for NQ queries x C classes: 2 per (query, 64-class tile).
 * Returns -1 for NQ <= 0, C <= 0 or a size beyond 2^31 - 1. */
int cfgt_workspace_floats(int NQ, int C);

/* ---- zero-shot text logits (few_shot.py:2843-2849, in the episode kernel's operation order):
 *     logits[q, c] = scale[0] * (dot(emb[q], text[c]) / en[q] / tn[c])      (no eps, unlike cos_sim)
 * emb [NQ, E] (cfgt_frame_mean of the tower features), en [NQ] and tn [C] their L2 norms (cfsg_row_norms), text [C, E], scale [1]
 * (device), logits [NQ, C].  The dot products are an exact-fp32 MFMA GEMM (k-ordered fmaf chains).  partials
 * [cfgt_workspace_floats(NQ, C)] receives (max, sum of expf(x - max)) of every (query, 64-class tile), for cfgt_text_softmax /
 * cfgt_text_combine.  emb and text 16-byte aligned, E % 4 == 0, 4 <= E <= 8192, NQ <= 65535 * 64. */
int cfgt_text_logits(const float* emb, const float* en, const float* text, const float* tn, const float* scale, float* logits,
                     float* partials, int NQ, int C, int E, cfgt_stream_t stream);

/* ---- softmax over the C classes of every query row (few_shot.py:2849): probs = expf(x - M) / S, M = max of the tile maxima m_j,
 * S = sum of s_j * expf(m_j - M).  logits and partials as written by cfgt_text_logits; probs [NQ, C] may be logits (in place). */
int cfgt_text_softmax(const float* logits, const float* partials, float* probs, int NQ, int C, cfgt_stream_t stream);

/* ---- COMBINE fusion (few_shot.py:2921-2928): out = p^coff * softmax_c((8 + v) / 8)^(1 - coff), p = the probabilities of
 * cfgt_text_softmax, v = visual [NQ, C] (cfsg_otam_gallery's logits = -cum).  out [NQ, C] may be logits (in place); coff finite. */
int cfgt_text_combine(const float* logits, const float* partials, const float* visual, float* out, int NQ, int C, float coff,
                      cfgt_stream_t stream);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* CLIPFSAR_GALLERY_TEXT_H */
