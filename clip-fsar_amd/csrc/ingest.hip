// Frame ingest (libclipfsar_ingest.so, C ABI in include/clipfsar_ingest.h): the test-time frame transform of rowops.hip's
// preprocess_kernel over clips of mixed geometry in ONE launch.  preprocess_kernel takes one (T, H, W) per launch; here a call is a
// descriptor table with one int32 row per group of frames that share a geometry, and the kernel finds a frame's group in it.
// One WORKGROUP per (frame, block of ROWS output rows): the frame number comes from blockIdx, so the search over the table's prefix
// offsets and the group's geometry are workgroup-uniform (the table loads are scalar loads), and the threads then stride over the
// block's pieces of PX horizontally adjacent pixels -- consecutive lanes write consecutive 16-byte (PX = 4) or 4-byte (PX = 1) pieces
// of a row of each channel plane.  The per-pixel arithmetic is frame_transform.h's, shared with preprocess_kernel: the same bits.
// A library of its own: the other five keep their pinned export sets.
#include <stdint.h>

#include "side_lib.h"
#include "frame_transform.h"
#include "../../include/clipfsar_ingest.h"

namespace {

constexpr int THREADS = 256;
constexpr int ROWS = 32;                       // output rows per workgroup: 32 x 224 / 4 = 7 pieces per thread at crop 224
constexpr unsigned MAX_BLOCKS = 4096;          // grid-stride beyond, as pool.hip
constexpr int COLS = CFSI_TABLE_COLS;

// the table row whose frames include frame fr: the last one whose prefix offset is <= fr (offsets start at 0 and strictly increase, n >= 1).
// Everything here is workgroup-uniform.
__device__ __forceinline__ const int* find_group(const int* __restrict__ table, unsigned S, unsigned fr) {
    unsigned lo = 0, hi = S;                   // table[lo][OUT_OFF] <= fr; hi == S or table[hi][OUT_OFF] > fr
    while (hi - lo > 1) {
        const unsigned mid = (lo + hi) >> 1;
        if ((unsigned)table[mid * COLS + CFSI_OUT_OFF] <= fr) lo = mid;
        else hi = mid;
    }
    return table + lo * COLS;
}

template <int PX>
__global__ __launch_bounds__(THREADS) void ingest_transform_kernel(const unsigned char* __restrict__ src, float* __restrict__ out,
                                                                   const int* __restrict__ table, unsigned S, unsigned units,
                                                                   unsigned upf, int crop, float m0, float m1, float m2, float is0,
                                                                   float is1, float is2) {
    const float mean[3] = {m0, m1, m2}, istd[3] = {is0, is1, is2};
    const unsigned ppr = (unsigned)crop / PX;                                  // pieces per output row
    for (unsigned u = blockIdx.x; u < units; u += gridDim.x) {
        const unsigned fr = u / upf;
        const int yb = (int)(u - fr * upf) * ROWS;
        const int* d = find_group(table, S, fr);
        const int H = d[CFSI_H], W = d[CFSI_W], y0 = d[CFSI_Y0], x0 = d[CFSI_X0];
        const float ry = frame_transform_ratio(H, d[CFSI_SCALE_H]), rx = frame_transform_ratio(W, d[CFSI_SCALE_W]);
        const unsigned char* f = src + (long long)(unsigned)d[CFSI_SRC_OFF16] * CFSI_SRC_ALIGN +
                                 (long long)(fr - (unsigned)d[CFSI_OUT_OFF]) * H * W * 3;
        float* o = out + (size_t)fr * 3 * crop * crop;
        const unsigned pieces = (unsigned)(crop - yb < ROWS ? crop - yb : ROWS) * ppr;
        for (unsigned p = threadIdx.x; p < pieces; p += THREADS) {
            const unsigned r = p / ppr;
            const int y = yb + (int)r, x = (int)(p - r * ppr) * PX;
            float v[PX][3];
#pragma unroll
            for (int j = 0; j < PX; ++j) frame_transform_pixel(f, H, W, ry, rx, y + y0, x + j + x0, mean, istd, v[j]);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float* dst = o + ((size_t)c * crop + y) * crop + x;
                if constexpr (PX == 4) *reinterpret_cast<float4*>(dst) = make_float4(v[0][c], v[1][c], v[2][c], v[3][c]);
                else *dst = v[0][c];
            }
        }
    }
}

constexpr long long MAX_ITEMS = 0x7fffffffLL;   // frames, work units and the bytes of one frame are indexed with 32 bits

// The host copy of the table, before any device work.
int check_table(const int32_t* t, int S, long long N, int crop, long long src_bytes) {
    SIDE_REQUIRE(S >= 1 && S <= CFSI_MAX_GROUPS, "cfsi_transform_frames: a table of S=%d rows, outside 1 .. %d", S, CFSI_MAX_GROUPS);
    long long frames = 0;
    for (int s = 0; s < S; ++s) {
        const int32_t* d = t + (size_t)s * COLS;
        const long long n = d[CFSI_N], H = d[CFSI_H], W = d[CFSI_W], sh = d[CFSI_SCALE_H], sw = d[CFSI_SCALE_W];
        SIDE_REQUIRE(n >= 1, "cfsi_transform_frames: row %d has n=%lld frames, a group needs at least 1", s, n);
        SIDE_REQUIRE(H >= 2 && W >= 2, "cfsi_transform_frames: row %d has a source of %lld x %lld, H and W must be at least 2", s, H, W);
        SIDE_REQUIRE(sh >= crop && sw >= crop, "cfsi_transform_frames: row %d has scale %lld x %lld below crop=%d", s, sh, sw, crop);
        SIDE_REQUIRE(d[CFSI_Y0] >= 0 && d[CFSI_X0] >= 0 && d[CFSI_Y0] + (long long)crop <= sh && d[CFSI_X0] + (long long)crop <= sw,
                     "cfsi_transform_frames: row %d: the crop window (y0=%d x0=%d crop=%d) lies outside the scaled image %lld x %lld", s,
                     d[CFSI_Y0], d[CFSI_X0], crop, sh, sw);
        SIDE_REQUIRE(d[CFSI_OUT_OFF] == frames, "cfsi_transform_frames: row %d has out_off %d, the prefix sum of n is %lld", s,
                     d[CFSI_OUT_OFF], frames);
        SIDE_REQUIRE(H * W * 3 <= MAX_ITEMS, "cfsi_transform_frames: row %d: a frame of %lld x %lld is too large for 32-bit indexing", s, H, W);
        SIDE_REQUIRE(d[CFSI_SRC_OFF16] >= 0, "cfsi_transform_frames: row %d has a negative source offset %d", s, d[CFSI_SRC_OFF16]);
        const long long first = (long long)d[CFSI_SRC_OFF16] * CFSI_SRC_ALIGN, bytes = n * H * W * 3;
        SIDE_REQUIRE(first + bytes <= src_bytes, "cfsi_transform_frames: row %d: bytes %lld .. %lld lie beyond src_bytes=%lld", s, first,
                     first + bytes, src_bytes);
        frames += n;
        SIDE_REQUIRE(frames <= MAX_ITEMS, "cfsi_transform_frames: the table's n are too large for one launch (row %d)", s);
    }
    SIDE_REQUIRE(frames == N, "cfsi_transform_frames: the table's n sum to %lld, not to N=%lld", frames, N);
    return 0;
}

}  // namespace

extern "C" int cfsi_version(void) { return 100; /* 0.1.0 */ }
extern "C" int cfsi_abi_version(void) { return CFSI_ABI_VERSION; }
extern "C" const char* cfsi_last_error(void) { return g_err; }

extern "C" int cfsi_transform_frames(const uint8_t* src, int64_t src_bytes, float* out, const int32_t* table_host, const int32_t* table_dev,
                                     int S, int N, int crop, const float* mean3, const float* std3, cfsi_stream_t stream) {
    SIDE_REQUIRE(src && out && table_host && table_dev && mean3 && std3, "cfsi_transform_frames: null pointer");
    SIDE_REQUIRE(N > 0 && crop > 0 && src_bytes > 0, "cfsi_transform_frames: bad shape (N=%d crop=%d src_bytes=%lld)", N, crop,
                 (long long)src_bytes);
    SIDE_REQUIRE(std3[0] != 0.f && std3[1] != 0.f && std3[2] != 0.f, "cfsi_transform_frames: a std of 0");
    if (check_table(table_host, S, N, crop, (long long)src_bytes)) return 1;
    const long long upf = (crop + ROWS - 1) / ROWS, units = (long long)N * upf;
    SIDE_REQUIRE(3LL * crop * crop <= MAX_ITEMS && units <= MAX_ITEMS, "cfsi_transform_frames: too large for one launch (N=%d crop=%d)", N,
                 crop);
    const unsigned blocks = (unsigned)(units < MAX_BLOCKS ? units : MAX_BLOCKS);
    const float is0 = 1.0f / std3[0], is1 = 1.0f / std3[1], is2 = 1.0f / std3[2];
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (crop % 4 == 0 && ((uintptr_t)out & 15u) == 0)
        hipLaunchKernelGGL(ingest_transform_kernel<4>, dim3(blocks), dim3(THREADS), 0, s, src, out, table_dev, (unsigned)S, (unsigned)units,
                           (unsigned)upf, crop, mean3[0], mean3[1], mean3[2], is0, is1, is2);
    else
        hipLaunchKernelGGL(ingest_transform_kernel<1>, dim3(blocks), dim3(THREADS), 0, s, src, out, table_dev, (unsigned)S, (unsigned)units,
                           (unsigned)upf, crop, mean3[0], mean3[1], mean3[2], is0, is1, is2);
    return check_launch("cfsi_transform_frames");
}
