/*
 * clipfsar_align.h -- C ABI of libclipfsar_align.so: the OTAM soft alignment behind a score (clip_fsar_amd.align.Aligner,
 * StreamPool.explain) for CLIP-FSAR (gfx950 / CDNA4).  A logit of the default eval branch is -(F(D) + F(D^T)), D the T x T cosine-distance
 * matrix of one (query, class) pair and F the OTAM soft-min DP (few_shot.py:2657-2687).  The scoring kernels compute D, walk it and throw
 * both away.  This library keeps them: per pair it returns D, the value and the gradient dF/dD -- the soft alignment, whose cell (l, m) is
 * the probability that the soft path pairs query frame l with prototype frame m.
 *
 * Conventions (as include/ext/clipfsar_pool_select.h and include/ext/clipfsar_shortlist.h): the library allocates no memory and owns no
 * stream, all work is enqueued on `stream` (a hipStream_t) of the CURRENT device; return 0 = success, non-zero = error with the message in
 * cfal_last_error() (thread-local).  Every pointer is a DEVICE pointer owned by the caller, the two pair lists included.
 */
#ifndef CLIPFSAR_ALIGN_H
#define CLIPFSAR_ALIGN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* Built with -fvisibility=hidden: exactly the entry points declared between this push and the pop are exported
 * (tests/test_align_abi.py compares `nm -D` with this file). */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

typedef void* cfal_stream_t;

/* library version (major*10000 + minor*100 + patch), ABI revision (bumped whenever an exported signature changes) and the last error
 * text of the calling thread */
#define CFAL_ABI_VERSION 1
#define CFAL_MAX_T 32   /* frames of a sequence */
#define CFAL_MIN_E 4    /* a row is read in 16-byte pieces */
#define CFAL_MAX_E 8192
int cfal_version(void);
int cfal_abi_version(void);
const char* cfal_last_error(void);

/* ---- the alignment of NP pairs; pair i is query pair_q[i] of Xq against store slot pair_slot[i] of P.  Every fp32 operation below is
 * one rounded operation (no contraction).
 *   distances   D[l, m] = 1 - dot(q_l, p_m) / (qn[l] * pn[m] + 0.01f): the dot product accumulated in double in an order that depends on
 *               nothing but E, rounded to fp32 once, the rest fp32; qn and pn are the row norms the caller passes (cfsg_row_norms of the
 *               queries, the store's pn)
 *   soft-min    softmin(x_1..x_n) = mn - lambda * logf(sum_i expf((mn - x_i) / lambda)), mn = min x_i: the reference's
 *               -lambda * log(sum exp(-x / lambda)), stabilised -- the un-stabilised fp32 form underflows where the gradient is wanted
 *   forward     F(d), d a T x T matrix: the padded recurrence of csrc/otam_dp.h on a grid c[T][T + 2], columns 0 and T + 1 zero padding:
 *               c[l][0] = 0; c[0][m] = d[0][m - 1] + c[0][m - 1]; for l >= 1 c[l][m] = d[l][m - 1] + softmin(predecessors), these being
 *               {(l-1, 0), (l-1, 1), (l, 0)} at m = 1, {(l-1, m-1), (l, m-1)} at 2 <= m <= T, {(l-1, T), (l-1, T+1), (l, T)} at m = T + 1;
 *               F = c[T - 1][T + 1]
 *   backward    G(d) = dF/dd: adjoints a[T - 1][T + 1] = 1, all others 0; rows l = T - 1 .. 1, within a row m = T + 1 .. 1: for every
 *               predecessor p of (l, m), a[p] += a[l][m] * expf((s - c[p]) / lambda) with s = c[l][m] - d[l][m - 1]; flow into a padding
 *               cell c[.][0] is dropped; G[l][m - 1] = a[l][m] for l >= 1; row 0 is a running sum, so G[0][j - 1] = sum of a[0][m] over
 *               m = T + 1 .. j, added in that order
 *   outputs     logits[i] = -(F(D) + F(D^T)), plan[i] = G(D) + G(D^T)^T; with single_direct -F(D) and G(D).  plan >= 0, and every
 *               direction contributes at most 1 per cell.  dists[i] = D when dists is given.
 * A pair whose query lies outside [0, NQ) or whose slot lies outside [0, cap) is never dereferenced: its plan, its dists and its logit are
 * NaN.  A pair may appear twice; both copies carry the same bytes.  The outputs are a function of the bits of the inputs alone: no atomics,
 * every sum in a fixed order, and two runs write the same bytes.
 * One 256-thread workgroup per pair: its four waves compute the T * T dot products (16-byte loads, double accumulation, a fixed-order
 * wave reduction) into LDS, one wave per direction runs the forward and the backward pass out of LDS, and all threads add the two
 * directions' gradients into plan.
 * Xq [NQ, T, E], P [cap, T, E] fp32, 16-byte aligned; qn [NQ * T], pn [cap * T] fp32; pair_q, pair_slot [NP] int32; plan, dists
 * [NP, T, T], logits [NP] fp32; dists may be NULL.  1 <= T <= CFAL_MAX_T; E % 4 == 0, CFAL_MIN_E <= E <= CFAL_MAX_E; NP, NQ, cap >= 1;
 * NP * T * T, NQ * T and cap * T below 2^31; lambda > 0 and finite. */
int cfal_align(const float* Xq, const float* qn, const float* P, const float* pn, const int32_t* pair_q, const int32_t* pair_slot, int NP,
               int NQ, int cap, int T, int E, float lambda, int single_direct, float* plan, float* dists_or_null, float* logits,
               cfal_stream_t stream);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* CLIPFSAR_ALIGN_H */
