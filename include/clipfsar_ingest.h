/*
 * clipfsar_ingest.h -- C ABI of libclipfsar_ingest.so: the test-time frame transform (uint8 THWC -> bilinear resize -> crop window ->
 * normalise -> fp32 [3, crop, crop] per frame) over clips of MIXED geometry in one launch, for CLIP-FSAR (gfx950 / CDNA4).  The device
 * side of clip_fsar_amd.ingest.FrameIngest.
 *
 * cfsar_preprocess_frames (include/clipfsar_hip.h) takes one (T, H, W) per call.  Here the frames of a call lie in one staging buffer
 * `src` of `src_bytes` uint8, as GROUPS: a group is a run of n frames of one geometry, [n, H, W, 3] dense (in practice one session's
 * clip).  A call is described by a DESCRIPTOR TABLE with one row of CFSI_TABLE_COLS int32 per group (O(groups), never O(frames)):
 *
 *   [CFSI_SRC_OFF16] offset of the group's first byte in src, in units of CFSI_SRC_ALIGN = 16 bytes (so 32 GiB are addressable)
 *   [CFSI_N]         frames of the group, n >= 1
 *   [CFSI_OUT_OFF]   index of the group's first frame in out: the sum of n over the rows before
 *   [CFSI_H], [CFSI_W]             source size, each >= 2
 *   [CFSI_SCALE_H], [CFSI_SCALE_W] size the frame is resized to, each >= crop
 *   [CFSI_Y0], [CFSI_X0]           top-left corner of the crop window in the resized frame; the window lies inside it
 *
 * out [N, 3, crop, crop] fp32 row-major, N = the sum of n.  A frame's output has the BITS cfsar_preprocess_frames writes for the same
 * frame and geometry: both kernels compile the per-pixel arithmetic from one header (csrc/frame_transform.h).
 *
 * Conventions (as include/clipfsar_pool.h): the library allocates no memory and owns no stream, all work is enqueued on `stream` (a
 * hipStream_t) of the CURRENT device; return 0 = success, non-zero = error with the message in cfsi_last_error() (thread-local).  Every
 * pointer is a DEVICE pointer owned by the caller, WITH THE EXCEPTIONS the pool header and cfsar_preprocess_frames already make: the
 * table is passed twice -- `table_host`, a HOST pointer to the S rows, which the entry point reads and validates before it touches the
 * device, and `table_dev`, the device copy of the same rows that the caller uploaded on `stream` before the call, which the kernel reads
 * -- and mean3 / std3 are HOST pointers to 3 floats each.  The host rows need to stay valid only for the duration of the call.  Each call
 * is one launch at any number of groups and frames.  out is written with 16-byte stores when crop % 4 == 0 and out is 16-byte aligned,
 * with 4-byte stores otherwise; src is read bytewise and needs no alignment of its own.
 */
#ifndef CLIPFSAR_INGEST_H
#define CLIPFSAR_INGEST_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* Built with -fvisibility=hidden: exactly the entry points declared between this push and the pop are exported
 * (tests/test_ingest_abi.py compares `nm -D` with this file). */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

typedef void* cfsi_stream_t;

/* library version (major*10000 + minor*100 + patch), ABI revision (bumped whenever an exported signature or the table layout changes)
 * and the last error text of the calling thread */
#define CFSI_ABI_VERSION 1
#define CFSI_MAX_GROUPS 65536
#define CFSI_SRC_ALIGN 16
#define CFSI_TABLE_COLS 9
#define CFSI_SRC_OFF16 0
#define CFSI_N 1
#define CFSI_OUT_OFF 2
#define CFSI_H 3
#define CFSI_W 4
#define CFSI_SCALE_H 5
#define CFSI_SCALE_W 6
#define CFSI_Y0 7
#define CFSI_X0 8
int cfsi_version(void);
int cfsi_abi_version(void);
const char* cfsi_last_error(void);

/* ---- the transform: for every row s of the table and i = 0 .. n_s - 1,
 *   out[out_off_s + i] = normalise(crop(resize(src[16 * src_off16_s + i * H_s * W_s * 3 ...], scale_h_s, scale_w_s), y0_s, x0_s, crop))
 * 1 <= S <= CFSI_MAX_GROUPS, N >= 1, crop >= 1.  Fails, before any device work, on a null pointer, on a row with n < 1, H or W < 2, a
 * scale below crop, a crop window outside the resized frame, an out_off that is not the running sum of n (or a total that is not N), a
 * group whose n * H * W * 3 bytes do not lie inside src_bytes, a std of 0, and on sizes beyond 32-bit indexing. */
int cfsi_transform_frames(const uint8_t* src, int64_t src_bytes, float* out, const int32_t* table_host, const int32_t* table_dev, int S,
                          int N, int crop, const float* mean3, const float* std3, cfsi_stream_t stream);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* CLIPFSAR_INGEST_H */
