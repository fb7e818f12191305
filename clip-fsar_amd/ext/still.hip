// The still-frame gate of a stream pool (libclipfsar_still.so, C ABI in include/ext/clipfsar_still.h): the change count of every frame of
// a pixel push against its predecessor, the packing of the frames that go through the tower (with the update of the store of every
// session's newest frame), and the expansion of the kept frames' tower rows to a row per frame.
// The compare is the bandwidth kernel: a frame is L = 3 H W floats (150 528 at 224 x 224), so the grid runs over (frame, chunk of
// CFSK_CHUNK elements) and not over frames -- 32 frames alone would leave most of the chip idle.  A workgroup compares its chunk with
// 16-byte loads (all of a thread's loads issued before the first compare), every thread counts in an int, the wave adds its lanes up,
// the workgroup its waves through LDS, and one thread stores the chunk's count; a second, tiny launch adds up a frame's chunks.
// Integers throughout: the result does not depend on any order.  The SIMPLE form was built: a frame is fetched once as x and once more
// as the predecessor y of the frame after it (2 N L 4 bytes requested against a floor of (N + S) L 4; the second fetch of a frame
// follows the first by one workgroup's worth of items and is served by the caches where they hold it).
// The pack is a chunked row copy over the same (row, chunk) grid, one launch for both of its destinations; the expansion moves rows of
// E floats, one WAVE per destination row as pool.hip's gather does.  Every destination element has exactly one writer (two runs write
// identical bytes), no workgroup waits on another.  Plain C++.
// A plug-in library (build.py, PLUGIN_LIBS): it lives beside csrc/, whose files and export sets stay as they are.
#include <math.h>

#include "../csrc/ring_rows.h"
#include "../csrc/side_lib.h"
#include "../../include/ext/clipfsar_still.h"

namespace {

constexpr int THREADS = 256;
constexpr int WAVE = 64;
constexpr int WAVES = THREADS / WAVE;
constexpr int COLS = CFSK_TABLE_COLS;
constexpr int CHUNK = CFSK_CHUNK;                // elements of a frame per workgroup and item
static_assert(CHUNK % (4 * THREADS) == 0, "a chunk is a whole number of 16-byte pieces per thread");

// the table row of frame r: the last row whose F0 is <= r (F0 starts at 0 and strictly ascends: every row has N >= 1).  Uniform.
__device__ __forceinline__ const int* find_row(const int* __restrict__ table, unsigned S, unsigned r) {
    unsigned lo = 0, hi = S;                     // table[lo][F0] <= r; hi == S or table[hi][F0] > r
    while (hi - lo > 1) {
        const unsigned mid = (lo + hi) >> 1;
        if ((unsigned)table[mid * COLS + CFSK_F0] <= r) lo = mid;
        else hi = mid;
    }
    return table + lo * COLS;
}

__device__ __forceinline__ unsigned wave_id() { return __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE); }

// 1 when the element changed: not (|x - y| <= tol), the subtraction rounded once.  A NaN on either side, and inf - inf, fail the <=.
__device__ __forceinline__ int moved(float x, float y, float tol) { return !(fabsf(__fsub_rn(x, y)) <= tol); }
__device__ __forceinline__ int moved(float4 x, float4 y, float tol) {
    return moved(x.x, y.x, tol) + moved(x.y, y.y, tol) + moved(x.z, y.z, tol) + moved(x.w, y.w, tol);
}

__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, WAVE);
    return v;
}

// ---- change counts, first launch.  Item = (frame i, chunk c) of `chunks` chunks per frame; work[item] = the chunk's count, or -1 in
// every chunk of a frame without a predecessor (nothing is loaded for it).  `pieces` = pieces of a frame, `per` = pieces of a chunk.
template <bool VEC>
__global__ __launch_bounds__(THREADS) void still_changed_kernel(const float* __restrict__ frames, const float* __restrict__ prev,
                                                                int* __restrict__ work, const int* __restrict__ table, unsigned S,
                                                                unsigned items, unsigned chunks, unsigned pieces, float tol) {
    typedef typename Piece<VEC>::type P;
    constexpr unsigned per = VEC ? CHUNK / 4 : CHUNK;
    constexpr unsigned each = per / THREADS;     // pieces per thread: 8 of 16 bytes, or 32 of 4
    __shared__ int part[WAVES];
    for (unsigned item = blockIdx.x; item < items; item += gridDim.x) {
        const unsigned i = item / chunks, c = item - i * chunks;
        const int* d = find_row(table, S, i);
        const bool first = i == (unsigned)d[CFSK_F0];
        if (first && d[CFSK_LAST_POS] < 0) {                    // workgroup-uniform
            if (threadIdx.x == 0) work[item] = -1;
            continue;
        }
        const size_t L = (size_t)pieces;                         // in pieces: 64-bit offsets from here on
        const P* x = reinterpret_cast<const P*>(frames) + (size_t)i * L;
        const P* y = first ? reinterpret_cast<const P*>(prev) + (size_t)d[CFSK_SLOT] * L : x - L;
        const unsigned p0 = c * per + threadIdx.x;
        int n = 0;
        if (p0 - threadIdx.x + per <= pieces) {                  // a whole chunk: every load ahead of the first compare
            P xs[each], ys[each];
#pragma unroll
            for (unsigned k = 0; k < each; ++k) xs[k] = x[p0 + k * THREADS];
#pragma unroll
            for (unsigned k = 0; k < each; ++k) ys[k] = y[p0 + k * THREADS];
#pragma unroll
            for (unsigned k = 0; k < each; ++k) n += moved(xs[k], ys[k], tol);
        } else {                                                 // the frame's last chunk
            for (unsigned p = p0; p < pieces; p += THREADS) n += moved(x[p], y[p], tol);
        }
        n = wave_sum_int(n);
        if (threadIdx.x % WAVE == 0) part[wave_id()] = n;
        __syncthreads();
        if (threadIdx.x == 0) {
            int sum = 0;
#pragma unroll
            for (int w = 0; w < WAVES; ++w) sum += part[w];
            work[item] = sum;
        }
        __syncthreads();                                         // part is written again by the next item
    }
}

// ---- change counts, second launch: counts[i] = the sum of frame i's chunks, or -1 (its chunks all say so)
__global__ __launch_bounds__(THREADS) void still_finish_kernel(const int* __restrict__ work, int* __restrict__ counts, unsigned N,
                                                               unsigned chunks) {
    for (unsigned i = blockIdx.x * THREADS + threadIdx.x; i < N; i += gridDim.x * THREADS) {
        const int* w = work + (size_t)i * chunks;
        int sum = w[0];
        if (sum >= 0)
            for (unsigned c = 1; c < chunks; ++c) sum += w[c];
        counts[i] = sum;
    }
}

// ---- pack.  Item = (row r, chunk c); rows 0 .. nk - 1: packed[r] = frames[kept[r]]; rows nk .. nk + S - 1: prev[SLOT_s] =
// frames[F0_s + N_s - 1], s = r - nk.
template <bool VEC>
__global__ __launch_bounds__(THREADS) void still_pack_kernel(const float* __restrict__ frames, float* __restrict__ packed,
                                                             float* __restrict__ prev, const int* __restrict__ kept,
                                                             const int* __restrict__ table, unsigned nk, unsigned items, unsigned chunks,
                                                             unsigned pieces) {
    typedef typename Piece<VEC>::type P;
    constexpr unsigned per = VEC ? CHUNK / 4 : CHUNK;
    for (unsigned item = blockIdx.x; item < items; item += gridDim.x) {
        const unsigned r = item / chunks, c = item - r * chunks;
        const size_t L = (size_t)pieces;
        const P* src;
        P* dst;
        if (r < nk) {
            src = reinterpret_cast<const P*>(frames) + (size_t)kept[r] * L;
            dst = reinterpret_cast<P*>(packed) + (size_t)r * L;
        } else {
            const int* d = table + (size_t)(r - nk) * COLS;
            src = reinterpret_cast<const P*>(frames) + (size_t)(d[CFSK_F0] + d[CFSK_N] - 1) * L;
            dst = reinterpret_cast<P*>(prev) + (size_t)d[CFSK_SLOT] * L;
        }
        const unsigned end = c * per + per < pieces ? c * per + per : pieces;
        for (unsigned p = c * per + threadIdx.x; p < end; p += THREADS) dst[p] = src[p];
    }
}

// ---- expand.  One wave per row i of feats: kept_feats[src[i]], or the ring row of the session's newest frame before the push.
template <bool VEC>
__global__ __launch_bounds__(THREADS) void still_expand_kernel(const float* __restrict__ kept_feats, const float* __restrict__ ring,
                                                               float* __restrict__ feats, const int* __restrict__ src,
                                                               const int* __restrict__ table, unsigned S, unsigned N, unsigned pieces,
                                                               unsigned cap) {
    typedef typename Piece<VEC>::type P;
    const unsigned lane = threadIdx.x % WAVE;
    for (unsigned i = blockIdx.x * WAVES + wave_id(); i < N; i += gridDim.x * WAVES) {
        const int at = src[i];
        const P* from;
        if (at >= 0) {
            from = reinterpret_cast<const P*>(kept_feats) + (size_t)at * pieces;
        } else {
            const int* d = find_row(table, S, i);
            from = reinterpret_cast<const P*>(ring) + ((size_t)d[CFSK_SLOT] * cap + (unsigned)d[CFSK_LAST_POS]) * pieces;
        }
        P* to = reinterpret_cast<P*>(feats) + (size_t)i * pieces;
        for (unsigned p = lane; p < pieces; p += WAVE) to[p] = from[p];
    }
}

// the host copy of the table, before any device work.  cap > 0: LAST_POS is checked against it as well.
int check_table(const char* what, const int32_t* t, int S, int N, int max_streams, int cap) {
    SIDE_REQUIRE(max_streams >= 1 && max_streams <= CFSK_MAX_STREAMS, "%s: max_streams=%d outside 1 .. %d", what, max_streams,
                 CFSK_MAX_STREAMS);
    SIDE_REQUIRE(S >= 1 && S <= max_streams, "%s: a table of S=%d rows for max_streams=%d", what, S, max_streams);
    SlotBits seen(max_streams);
    SIDE_REQUIRE(seen.ok(), "%s: out of host memory for %d slots", what, max_streams);
    long long f0 = 0;
    for (int s = 0; s < S; ++s) {
        const int32_t* d = t + (size_t)s * COLS;
        const int slot = d[CFSK_SLOT];
        SIDE_REQUIRE(slot >= 0 && slot < max_streams, "%s: row %d has slot %d outside 0 .. %d", what, s, slot, max_streams - 1);
        SIDE_REQUIRE(!seen.test_and_set(slot), "%s: slot %d appears twice in the table (row %d)", what, slot, s);
        SIDE_REQUIRE(d[CFSK_N] >= 1, "%s: row %d has n=%d frames, every row needs at least 1", what, s, d[CFSK_N]);
        SIDE_REQUIRE(d[CFSK_F0] == f0, "%s: row %d has f0=%d, the prefix sum of the counts is %lld", what, s, d[CFSK_F0], f0);
        SIDE_REQUIRE(d[CFSK_LAST_POS] >= -1 && (cap <= 0 || d[CFSK_LAST_POS] < cap),
                     "%s: row %d has last_pos=%d outside -1 .. %d", what, s, d[CFSK_LAST_POS], cap > 0 ? cap - 1 : 0x7fffffff);
        f0 += d[CFSK_N];
        SIDE_REQUIRE(f0 <= MAX_ITEMS, "%s: the table's counts are too large for one launch (row %d)", what, s);
    }
    SIDE_REQUIRE(f0 == N, "%s: the table's n sum to %lld, not to N=%d", what, f0, N);
    return 0;
}

// do the byte ranges [a, a + na) and [b, b + nb) share a byte?
bool overlap(const void* a, long long na, const void* b, long long nb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + (uintptr_t)nb && b0 < a0 + (uintptr_t)na;
}

long long chunks_of(long long L) { return (L + CHUNK - 1) / CHUNK; }

}  // namespace

extern "C" int cfsk_version(void) { return 100; /* 0.1.0 */ }
extern "C" int cfsk_abi_version(void) { return CFSK_ABI_VERSION; }
extern "C" const char* cfsk_last_error(void) { return g_err; }

extern "C" int cfsk_workspace_ints(int N, long long L) {
    if (N < 1 || L < 1 || L > MAX_ITEMS) return -1;
    const long long ints = (long long)N * chunks_of(L);
    return ints <= MAX_ITEMS ? (int)ints : -1;
}

extern "C" int cfsk_changed(const float* frames, const float* prev, int32_t* counts, int32_t* work, const int32_t* table_host,
                            const int32_t* table_dev, int S, int N, long long L, int max_streams, float tol, cfsk_stream_t stream) {
    SIDE_REQUIRE(frames && prev && counts && work && table_host && table_dev, "cfsk_changed: null pointer");
    SIDE_REQUIRE(N > 0 && L > 0, "cfsk_changed: bad shape (N=%d L=%lld)", N, L);
    SIDE_REQUIRE(L <= MAX_ITEMS, "cfsk_changed: L=%lld elements per frame, a frame is indexed with 32 bits", L);
    SIDE_REQUIRE(isfinite(tol) && tol >= 0.f, "cfsk_changed: tol=%g must be finite and >= 0", (double)tol);
    if (check_table("cfsk_changed", table_host, S, N, max_streams, 0)) return 1;
    const long long chunks = chunks_of(L), items = (long long)N * chunks;
    SIDE_REQUIRE(items <= MAX_ITEMS, "cfsk_changed: too large for one launch (N=%d frames of %lld chunks)", N, chunks);
    const long long fb = (long long)N * L * 4, pb = (long long)max_streams * L * 4;
    SIDE_REQUIRE(!overlap(counts, (long long)N * 4, frames, fb) && !overlap(counts, (long long)N * 4, prev, pb) &&
                     !overlap(work, items * 4, frames, fb) && !overlap(work, items * 4, prev, pb) &&
                     !overlap(counts, (long long)N * 4, work, items * 4),
                 "cfsk_changed: counts or work overlaps frames, prev or each other -- give each a buffer of its own");
    const bool vec = vec_ok(frames, prev, (int)(L % 4));       // L % 4 in place of L: the same verdict, and L need not fit an int
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (vec)
        hipLaunchKernelGGL(still_changed_kernel<true>, dim3(blocks_for(items, 1)), dim3(THREADS), 0, s, frames, prev, work, table_dev,
                           (unsigned)S, (unsigned)items, (unsigned)chunks, (unsigned)(L / 4), tol);
    else
        hipLaunchKernelGGL(still_changed_kernel<false>, dim3(blocks_for(items, 1)), dim3(THREADS), 0, s, frames, prev, work, table_dev,
                           (unsigned)S, (unsigned)items, (unsigned)chunks, (unsigned)L, tol);
    if (check_launch("cfsk_changed")) return 1;
    hipLaunchKernelGGL(still_finish_kernel, dim3(blocks_for(N, THREADS)), dim3(THREADS), 0, s, work, counts, (unsigned)N, (unsigned)chunks);
    return check_launch("cfsk_changed");
}

extern "C" int cfsk_pack(const float* frames, float* packed, float* prev, const int32_t* kept_host, const int32_t* kept_dev, int NK,
                         const int32_t* table_host, const int32_t* table_dev, int S, int N, long long L, int max_streams,
                         cfsk_stream_t stream) {
    SIDE_REQUIRE(frames && prev && table_host && table_dev, "cfsk_pack: null pointer");
    SIDE_REQUIRE(N > 0 && L > 0, "cfsk_pack: bad shape (N=%d L=%lld)", N, L);
    SIDE_REQUIRE(L <= MAX_ITEMS, "cfsk_pack: L=%lld elements per frame, a frame is indexed with 32 bits", L);
    SIDE_REQUIRE(NK >= 0 && NK <= N, "cfsk_pack: NK=%d kept frames outside 0 .. N=%d", NK, N);
    const int nk = NK == N ? 0 : NK;             // every frame kept: the caller's tower reads `frames`, nothing is packed
    SIDE_REQUIRE(nk == 0 || (packed && kept_host && kept_dev), "cfsk_pack: null pointer (packed or kept, with NK=%d of N=%d)", NK, N);
    if (check_table("cfsk_pack", table_host, S, N, max_streams, 0)) return 1;
    for (int r = 0; r < nk; ++r) {
        SIDE_REQUIRE(kept_host[r] >= 0 && kept_host[r] < N, "cfsk_pack: kept[%d]=%d outside 0 .. %d", r, kept_host[r], N - 1);
        SIDE_REQUIRE(r == 0 || kept_host[r] > kept_host[r - 1], "cfsk_pack: kept[%d]=%d after kept[%d]=%d, the list must be strictly ascending",
                     r, kept_host[r], r - 1, kept_host[r - 1]);
    }
    const long long chunks = chunks_of(L), items = ((long long)nk + S) * chunks;
    SIDE_REQUIRE(items <= MAX_ITEMS, "cfsk_pack: too large for one launch (NK=%d S=%d rows of %lld chunks)", NK, S, chunks);
    const long long fb = (long long)N * L * 4, pb = (long long)max_streams * L * 4, kb = (long long)nk * L * 4;
    SIDE_REQUIRE(!overlap(prev, pb, frames, fb), "cfsk_pack: prev overlaps frames -- the store is a buffer of its own");
    SIDE_REQUIRE(nk == 0 || (!overlap(packed, kb, frames, fb) && !overlap(packed, kb, prev, pb)),
                 "cfsk_pack: packed overlaps frames or prev -- give it a buffer of its own");
    const bool vec = vec_ok(frames, prev, (int)(L % 4)) && (nk == 0 || ((uintptr_t)packed & 15u) == 0);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (vec)
        hipLaunchKernelGGL(still_pack_kernel<true>, dim3(blocks_for(items, 1)), dim3(THREADS), 0, s, frames, packed, prev, kept_dev,
                           table_dev, (unsigned)nk, (unsigned)items, (unsigned)chunks, (unsigned)(L / 4));
    else
        hipLaunchKernelGGL(still_pack_kernel<false>, dim3(blocks_for(items, 1)), dim3(THREADS), 0, s, frames, packed, prev, kept_dev,
                           table_dev, (unsigned)nk, (unsigned)items, (unsigned)chunks, (unsigned)L);
    return check_launch("cfsk_pack");
}

extern "C" int cfsk_expand(const float* kept_feats, const float* ring, float* feats, const int32_t* src_host, const int32_t* src_dev, int NK,
                           const int32_t* table_host, const int32_t* table_dev, int S, int N, int E, int max_streams, int cap,
                           cfsk_stream_t stream) {
    SIDE_REQUIRE(ring && feats && src_host && src_dev && table_host && table_dev, "cfsk_expand: null pointer");
    SIDE_REQUIRE(N > 0 && E > 0 && cap > 0, "cfsk_expand: bad shape (N=%d E=%d cap=%d)", N, E, cap);
    SIDE_REQUIRE(NK >= 0 && NK <= N, "cfsk_expand: NK=%d kept frames outside 0 .. N=%d", NK, N);
    SIDE_REQUIRE(NK == 0 || kept_feats, "cfsk_expand: null pointer (kept_feats, with NK=%d)", NK);
    if (check_table("cfsk_expand", table_host, S, N, max_streams, cap)) return 1;
    for (int s = 0; s < S; ++s) {
        const int32_t* d = table_host + (size_t)s * COLS;
        for (int i = d[CFSK_F0]; i < d[CFSK_F0] + d[CFSK_N]; ++i) {
            SIDE_REQUIRE(src_host[i] >= -1 && src_host[i] < NK, "cfsk_expand: src[%d]=%d outside -1 .. NK-1=%d", i, src_host[i], NK - 1);
            SIDE_REQUIRE(src_host[i] >= 0 || d[CFSK_LAST_POS] >= 0,
                         "cfsk_expand: src[%d]=-1 in row %d, whose session has no frame before the push (last_pos=%d)", i, s,
                         d[CFSK_LAST_POS]);
        }
    }
    const bool vec = vec_ok(ring, feats, E) && ((uintptr_t)kept_feats & 15u) == 0;
    const long long pieces = vec ? E / 4 : E;
    SIDE_REQUIRE((long long)N * pieces <= MAX_ITEMS && (long long)max_streams * cap * pieces <= MAX_ITEMS,
                 "cfsk_expand: too large for one launch (N=%d E=%d max_streams=%d cap=%d)", N, E, max_streams, cap);
    const long long ob = (long long)N * E * 4;
    SIDE_REQUIRE(!overlap(feats, ob, ring, (long long)max_streams * cap * E * 4) &&
                     (NK == 0 || !overlap(feats, ob, kept_feats, (long long)NK * E * 4)),
                 "cfsk_expand: feats overlaps kept_feats or the ring -- give it a buffer of its own");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (vec)
        hipLaunchKernelGGL(still_expand_kernel<true>, dim3(blocks_for(N, WAVES)), dim3(THREADS), 0, s, kept_feats, ring, feats, src_dev,
                           table_dev, (unsigned)S, (unsigned)N, (unsigned)pieces, (unsigned)cap);
    else
        hipLaunchKernelGGL(still_expand_kernel<false>, dim3(blocks_for(N, WAVES)), dim3(THREADS), 0, s, kept_feats, ring, feats, src_dev,
                           table_dev, (unsigned)S, (unsigned)N, (unsigned)pieces, (unsigned)cap);
    return check_launch("cfsk_expand");
}
