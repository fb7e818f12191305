/*
 * clipfsar_lastblock.h -- C ABI of libclipfsar_lastblock.so: the class-token attention of the LAST ViT block without its K | V projection
 * (clip_fsar_amd.engine.HipViT, option fold_last_kv) for CLIP-FSAR (gfx950 / CDNA4).
 *
 * The last block is pruned to the class-token rows behind the attention, so its one query per frame uses the K and V rows of the frame's
 * tokens only through two linear functionals per head h (64 columns), and both apply to the residual stream directly.  With x_t the raw
 * fp16 stream row of token t, (mu_t, sd_t) its LayerNorm statistics, Wk' = Wk diag(gamma), Wv' = Wv diag(gamma) (the LN-folded weights) and
 * q the class row's query:
 *
 *   key fold      g_h = (1/8) Wk'_h^T q_h  (a D-vector),  G_h = sum_k g_h[k]
 *   class attend  s_t = (x_t . g_h - mu_t G_h) / sd_t,  p = softmax_t(s),  z_h = sum_t p_t (x_t - mu_t) / sd_t  (a D-vector)
 *   value fold    o_h = Wv'_h z_h + d_v[h]
 *
 * (the terms of the scores that do not depend on t cancel in the softmax; sum_t p_t = 1 carries the bias).  o is what
 * cfsar_vit_attention_cls delivers from K and V rows rounded to 16 bits.
 *
 * Conventions (as include/clipfsar_groups.h): the library allocates no memory and owns no stream, all work is enqueued on `stream` (a
 * hipStream_t) of the CURRENT device; return 0 = success, non-zero = error with the message in cflb_last_error() (thread-local).  Every
 * pointer is a DEVICE pointer owned by the caller, 16-byte aligned, to a contiguous row-major tensor; arguments are validated before any
 * device work.  D = 64 * heads, 1 <= heads <= 16, F >= 1.  No atomics; every reduction has a fixed order that does not depend on F, so a
 * frame's bits do not depend on the batch it is served in.
 */
#ifndef CLIPFSAR_LASTBLOCK_H
#define CLIPFSAR_LASTBLOCK_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* Built with -fvisibility=hidden: exactly the entry points declared between this push and the pop are exported
 * (tests/test_lastblock_abi.py compares `nm -D` with this file). */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

typedef void* cflb_stream_t;

/* library version (major*10000 + minor*100 + patch), ABI revision (bumped whenever an exported signature changes) and the last error
 * text of the calling thread */
#define CFLB_ABI_VERSION 1
#define CFLB_MAX_HEADS 16
#define CFLB_FRAME_BATCH 16   /* frames per workgroup of the two fold kernels */
#define CFLB_TOKEN_CHUNK 32   /* tokens per step of the class-attend kernel's online softmax */
#define CFLB_BF16 1           /* dtype codes of q and oc */
#define CFLB_F16 2
int cflb_version(void);
int cflb_abi_version(void);
const char* cflb_last_error(void);

/* ---- key fold: g[f, h, k] = fp16((1/8) sum_j q[f, 64 h + j] Wk'[64 h + j, k]),  G[f, h] = sum_k g[f, h, k] (of the ROUNDED g, fp32).
 * q [F, D] bf16 or fp16 (dtype); wk_t [heads, D, 64] fp16, the TRANSPOSE of each head's rows: wk_t[h, k, j] = Wk'[64 h + j, k] (made once
 * when the weights are loaded); g [F, heads, D] fp16; G [F, heads] fp32.  The products are exact in fp32 accumulation (a bf16 q is an
 * fp16 value), g is rounded once. */
int cflb_key_fold(const void* q, int dtype, const void* wk_t, void* g, float* G, int F, int D, int heads, cflb_stream_t stream);

/* ---- class attend: z[f, h, :] = sum_t p_t (x_t - mu_t) / sd_t with p = softmax_t((x_t . g - mu_t G) / sd_t), t over the frame's ntok >= 1
 * rows.  x [F * ntok, D] fp16; g, G as cflb_key_fold wrote them; z [F, heads, D] fp32.  The row statistics come in EXACTLY ONE of two
 * forms: `partial` [F * ntok, slots, 2] fp32, the producer GEMM's (sum, sum of squares) pairs, 1 <= slots <= 16, finalized here with
 * cfsar_ln_stats_finalize's formula (mean = s / D, var = max(ss / D - mean^2, 0), sd = sqrt(var + eps)); or `rowstats` [F * ntok, 4] fp32 =
 * (mean, sd, 1 / sd, -).  The other pointer is null (and slots 0 with rowstats).  F * ntok below 2^31. */
int cflb_class_attend(const void* x, const void* g, const float* G, const float* partial, int slots, const float* rowstats, float eps,
                      float* z, int F, int ntok, int D, int heads, cflb_stream_t stream);

/* ---- value fold: oc[f, 64 h + j] = dtype(sum_k Wv'[64 h + j, k] z[f, h, k] + d_v[64 h + j]).  z [F, heads, D] fp32 (fed to the matrix
 * pipe as fp16 hi + lo pairs); wv [D, D] fp16 row-major; d_v [D] fp32; oc [F, D] bf16 or fp16 (dtype). */
int cflb_value_fold(const float* z, const void* wv, const float* d_v, void* oc, int dtype, int F, int D, int heads, cflb_stream_t stream);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* CLIPFSAR_LASTBLOCK_H */
