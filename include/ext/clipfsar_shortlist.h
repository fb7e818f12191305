/*
 * clipfsar_shortlist.h -- C ABI of libclipfsar_shortlist.so: the coarse stage of two-stage scoring
 * (clip_fsar_amd.shortlist.Shortlist) for CLIP-FSAR (gfx950 / CDNA4).  A cheap score of every (query, class) pair picks, per GROUP of
 * consecutive queries, the K classes worth the exact cosine + OTAM kernel, and writes their store slots as the per-group lists
 * cfgr_otam_grouped (include/clipfsar_groups.h) reads from device memory -- the host does not synchronise between the stages.
 *
 * The coarse score.  OTAM walks the matrix cos(q_i, p_j) of a query's T frame rows against a class's T prototype rows.  The mean of that
 * matrix over its T x T cells is ONE dot product, <u_q, u_p>, with u the mean of a sequence's unit-normalised rows.  So a class is one
 * [E] row of a COARSE STORE [cap, E] beside the prototype store, a query is one [E] row, and the scores are a GEMM.  It is a heuristic,
 * not a bound on the OTAM logit; what is exact is the selection: which classes are kept is a bit-for-bit function of the coarse scores.
 *
 * Conventions (as include/ext/clipfsar_class_smooth.h and include/clipfsar_groups.h): the library allocates no memory and owns no stream,
 * all work is enqueued on `stream` (a hipStream_t) of the CURRENT device; return 0 = success, non-zero = error with the message in
 * cfsh_last_error() (thread-local).  All tensors are fp32 row-major unless said otherwise.  Every pointer is a DEVICE pointer owned by the
 * caller, WITH ONE EXCEPTION: the group table of cfsh_select is passed twice -- `table_host`, a HOST pointer to the G rows, which the entry
 * point reads and validates before it touches the device, and `table_dev`, the device copy of the same rows that the caller uploaded on
 * `stream` before the call, which the kernel reads.  A table has one row of CFSH_TABLE_COLS int32 per group:
 *
 *   [CFSH_Q0]   first query of the group: the sum of NQ over the rows before
 *   [CFSH_NQ]   queries of the group, >= 0 (a group without queries selects nothing)
 *
 * The running sum must end at NQ.
 */
#ifndef CLIPFSAR_SHORTLIST_H
#define CLIPFSAR_SHORTLIST_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* Built with -fvisibility=hidden: exactly the entry points declared between this push and the pop are exported
 * (tests/test_shortlist_abi.py compares `nm -D` with this file). */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

typedef void* cfsh_stream_t;

/* library version (major*10000 + minor*100 + patch), ABI revision (bumped whenever an exported signature or the table layout changes)
 * and the last error text of the calling thread */
#define CFSH_ABI_VERSION 1
/* CFSH_MAX_T is not a need of the kernel, which sums over t in a loop: it is the limit of the second stage (CFGR_MAX_T of
 * include/clipfsar_groups.h, CFSL_MAX_T of the store) -- a longer sequence has no exact kernel to be shortlisted for -- and the largest T
 * at which the rounding of a coarse row, (T + 2) * 2^-24 per unit of the mean |x| / norm, is tested. */
#define CFSH_MAX_T 32
#define CFSH_MAX_KEEP 4096
#define CFSH_MAX_GROUPS 65536
#define CFSH_TABLE_COLS 2
#define CFSH_Q0 0
#define CFSH_NQ 1
#define CFSH_NONE 0x7fffffff /* sel_cols of a place without a column; its sel_slots is -1 */
#define CFSH_TINY 1e-12f     /* a row norm below it counts as this */
int cfsh_version(void);
int cfsh_abi_version(void);
const char* cfsh_last_error(void);

/* ---- the coarse row of a sequence: the mean of its unit-normalised rows.  For i < n, with b = slots[i] when a list is given and b = i
 * otherwise (b names a block of T rows of X, of T values of norms and a row of out):
 *     acc = 0;  for t = 0 .. T-1 in order, per column e:  acc = acc + X[b, t, e] / fmaxf(norms[b * T + t], CFSH_TINY)
 *     out[b, e] = acc * (1.0f / (float)T)
 * every operation ONE rounded fp32 operation (a rounded quotient, then a rounded sum: nothing is fused), so the value of a row depends on
 * nothing but that sequence.  One kernel serves both sides: the store passes its prototypes P [cap, T, E], their norms pn [cap * T] and
 * the list of slots whose rows are out of date, and writes the coarse store [cap, E]; the queries pass Xq [n, T, E], qn [n * T] and no
 * list (slots = NULL), and write U [n, E].  X, norms and out have `cap` blocks; without a list n <= cap.  slots is device data: a slot
 * outside [0, cap) is never dereferenced and writes nothing; no list should name a slot twice (both writes would carry the same value).
 * X and out are read and written as float4: 16-byte aligned, E % 4 == 0, 4 <= E <= 8192, 1 <= T <= CFSH_MAX_T, n >= 1, cap >= 1,
 * cap * T below 2^31. */
int cfsh_mean_unit_rows(const float* X, const float* norms, const int32_t* slots_or_null, float* out, int n, int cap, int T, int E,
                        cfsh_stream_t stream);

/* ---- the coarse scores: S[q, j] = <U[q], C_store[cols[j]]>, a row-major [NQ, NC] matrix, by the exact-fp32 tile GEMM of the gallery
 * kernels (chunks of 32 products summed from zero, then added to the running sum).  U [NQ, E], C_store [cap, E], cols [NC] int32
 * (DEVICE): a slot outside [0, cap) is never dereferenced and gives a column of NaN.  U and C_store are read as float4: 16-byte aligned,
 * E % 4 == 0, 4 <= E <= 8192; NQ, NC, cap >= 1, NQ * NC below 2^31.  One 256-thread workgroup per 64 x 64 tile. */
int cfsh_coarse_scores(const float* U, const float* C_store, const int32_t* cols, float* S, int NQ, int NC, int cap, int E,
                       cfsh_stream_t stream);

/* ---- the selection, per group g of the table, over the NC columns of S [NQ, NC]:
 *   the group's score  of column c is the maximum of S[q, c] over the group's queries q, NaN ignored (a column that is NaN in every
 *                      query, and every column of a group without queries, has no score and is not selectable; neither is a score of
 *                      -inf, the value top-k gives an empty place)
 *   kept               are the K = min(keep, NC) best selectable columns: the larger score first, the lower column on equal scores;
 *                      -0.0 and +0.0 are equal, as floats compare
 *   written            in ASCENDING COLUMN ORDER: sel_cols[g * K + r] = the column, sel_slots[g * K + r] = cols[column]; when fewer than
 *                      K columns are selectable the places behind them hold CFSH_NONE and -1
 * so the kept set and its order are a function of the bits of S alone: a place is a prefix sum over the columns, never a race, and two
 * runs write the same bytes.  One 256-thread workgroup per group: the group scores as order-preserving 32-bit keys into `work`, four
 * radix passes (per-wave histograms in LDS) for the K-th largest key, then a scan over the columns that compacts "above the threshold,
 * and the first few equal to it".  work: cfsh_workspace_floats(G, NC) floats, contents undefined afterwards.  cols [NC] int32, sel_cols
 * and sel_slots [G * K] int32.  1 <= keep <= CFSH_MAX_KEEP, 1 <= G <= CFSH_MAX_GROUPS, NQ >= 1, NC >= 1, NQ * NC and G * NC below 2^31. */
int cfsh_workspace_floats(int G, int NC); /* G * NC, or -1 when an argument is out of range or the product reaches 2^31 */
int cfsh_select(const float* S, const int32_t* cols, const int32_t* table_host, const int32_t* table_dev, int G, int NQ, int NC,
                int keep, int32_t* sel_cols, int32_t* sel_slots, float* work, cfsh_stream_t stream);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* CLIPFSAR_SHORTLIST_H */
