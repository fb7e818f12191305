/*
 * clipfsar_still.h -- C ABI of libclipfsar_still.so: the still-frame gate of a stream pool (clip_fsar_amd.pool.StreamPool(still=...),
 * semantics in clip_fsar_amd.still) for CLIP-FSAR (gfx950 / CDNA4).  A frame of a pixel push that did not change against its
 * predecessor takes the predecessor's tower row instead of going through the tower.  Three entry points, in the order a push calls them:
 * the change count of every frame against its predecessor, the packing of the frames that go through the tower (with the update of the
 * store of every session's newest frame), and the expansion of the kept frames' tower rows to a row per frame.
 *
 * A push is described by one table of CFSK_TABLE_COLS int32 per session, rows in the order of the packed frames:
 *     CFSK_SLOT      the session's slot: its row of `prev` [max_streams, L] and of the pool's ring [max_streams, cap, E]
 *     CFSK_F0        the row of the session's first frame in the packed frames [N, L]: the prefix sum of the counts before it
 *     CFSK_N         its frames in this push, >= 1
 *     CFSK_LAST_POS  the ring position of the session's newest frame before the push, (t - 1) mod cap, or -1: the session has no
 *                    predecessor (nothing of prev[slot] and of ring[slot] is read then)
 *
 * Conventions (as include/clipfsar_pool.h): the library allocates no memory and owns no stream, all work is enqueued on `stream` (a
 * hipStream_t) of the CURRENT device; return 0 = success, non-zero = error with the message in cfsk_last_error() (thread-local).  All
 * tensors are row-major.  Every pointer is a DEVICE pointer owned by the caller, WITH THE EXCEPTIONS `table_host`, `kept_host` and
 * `src_host`: HOST copies of the lists whose device copies (`table_dev`, `kept_dev`, `src_dev`) the kernels read, validated before the
 * device is touched and needed only for the duration of the call.
 */
#ifndef CLIPFSAR_STILL_H
#define CLIPFSAR_STILL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* Built with -fvisibility=hidden: exactly the entry points declared between this push and the pop are exported
 * (tests/test_still_abi.py compares `nm -D` with this file). */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

typedef void* cfsk_stream_t;

/* library version (major*10000 + minor*100 + patch), ABI revision (bumped whenever an exported signature changes) and the last error
 * text of the calling thread */
#define CFSK_ABI_VERSION 1
#define CFSK_TABLE_COLS 4
#define CFSK_SLOT 0
#define CFSK_F0 1
#define CFSK_N 2
#define CFSK_LAST_POS 3
#define CFSK_MAX_STREAMS 65536
#define CFSK_CHUNK 8192 /* elements of a frame that one workgroup compares at a time */
int cfsk_version(void);
int cfsk_abi_version(void);
const char* cfsk_last_error(void);

/* int32 values of the `work` buffer cfsk_changed needs for N frames of L elements: N * ceil(L / CFSK_CHUNK); -1 when N < 1, L < 1 or
 * the product is 2^31 or more */
int cfsk_workspace_ints(int N, long long L);

/* ---- change counts: frames [N, L] fp32, prev [max_streams, L] fp32 -> counts [N] int32.  Frame i of table row s (F0_s <= i < F0_s +
 * N_s) has the predecessor frames[i - 1] when i > F0_s, prev[SLOT_s] when i == F0_s and LAST_POS_s >= 0, and none otherwise:
 *     counts[i] = the number of elements e with  not (fabsf(x[e] - y[e]) <= tol),  x the frame and y its predecessor;  -1 without one
 * The subtraction is one rounded fp32 operation.  A NaN in either frame counts as changed, and so does inf - inf; -0.0 against +0.0
 * does not.  tol must be finite and >= 0.  The count is an integer: the same bits whatever the order of the reduction.
 * Two launches: every workgroup counts a chunk of CFSK_CHUNK elements of one frame (a grid over (frame, chunk), a wave reduction, then
 * across the waves through LDS, integers throughout) into work [cfsk_workspace_ints(N, L)]; the second launch adds up a frame's chunks.
 * 16-byte loads when L % 4 == 0 and frames and prev are 16-byte aligned, 4-byte loads otherwise; element offsets are 64-bit (N * L may
 * pass 2^31; L itself, the number of chunks and N stay below it).  Every frame is read as x and, unless it is a session's last, as y:
 * up to 2 * N * L * 4 bytes are requested (the floor, every frame fetched once, is (N + S) * L * 4).  frames and prev are only read;
 * counts and work may not overlap them. */
int cfsk_changed(const float* frames, const float* prev, int32_t* counts, int32_t* work, const int32_t* table_host, const int32_t* table_dev,
                 int S, int N, long long L, int max_streams, float tol, cfsk_stream_t stream);

/* ---- pack: ONE launch, two copies with disjoint destinations:
 *     packed[r]     = frames[kept[r]]           r < NK      (0 <= NK <= N; kept strictly ascending in 0 .. N - 1; with NK == 0 or
 *                                                            NK == N -- the caller then runs the tower on `frames` itself -- packed,
 *                                                            kept_host and kept_dev may be null and nothing is packed)
 *     prev[SLOT_s]  = frames[F0_s + N_s - 1]    for every table row
 * Enqueued after cfsk_changed on the same stream: that read of prev precedes this overwrite.  Rows of prev whose slot is not in the
 * table are not touched.  packed [NK, L]; packed and prev may not overlap frames or each other.  16-byte accesses when L % 4 == 0 and
 * all three bases are 16-byte aligned, 4-byte accesses otherwise. */
int cfsk_pack(const float* frames, float* packed, float* prev, const int32_t* kept_host, const int32_t* kept_dev, int NK,
              const int32_t* table_host, const int32_t* table_dev, int S, int N, long long L, int max_streams, cfsk_stream_t stream);

/* ---- expand: kept_feats [NK, E], ring [max_streams, cap, E] -> feats [N, E]:
 *     feats[i] = src[i] >= 0 ? kept_feats[src[i]] : ring[SLOT_s, LAST_POS_s]       s the table row of frame i
 * Refused when a src value lies outside [-1, NK) or a -1 sits in a row with LAST_POS < 0.  With NK == 0 kept_feats may be null.  The
 * ring is only read and every row of feats has one writer; feats may not overlap kept_feats or the ring.  The call runs before the
 * push writes its rows into the ring.  One launch; 16-byte accesses when E % 4 == 0 and the bases are 16-byte aligned. */
int cfsk_expand(const float* kept_feats, const float* ring, float* feats, const int32_t* src_host, const int32_t* src_dev, int NK,
                const int32_t* table_host, const int32_t* table_dev, int S, int N, int E, int max_streams, int cap, cfsk_stream_t stream);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* CLIPFSAR_STILL_H */
