// The per-pixel arithmetic of the test-time frame transform (reference datasets/utils/transformations.py:663-716 after ToTensorVideo,
// before the permute): source index of a bilinear resize with align_corners = False, the clamps, the four weights, the four-tap
// expression on uint8 / 255 and the normalisation.  rowops.hip (preprocess_kernel, one geometry per launch) and ingest.hip
// (ingest_transform_kernel, a geometry per descriptor-table row) both call these, and a frame comes out with the same bits from either.
//
// Every rounding is WRITTEN OUT (__fmul_rn / __fmaf_rn / ...).  As an ordinary expression,
//     v = hy * (hx * a + lx * b) + ly * (hx * c + lx * d),
// the compiler contracts each sum into ONE fma and is free to pick which of the two products it fuses; it does pick differently from one
// kernel to the next (and from one channel to the next), which puts results one unit in the last place apart.  What is written here is,
// operation for operation, what preprocess_kernel computed when it held this arithmetic itself (read off its ISA), so
// cfsar_preprocess_frames keeps its bits: lx * b is rounded, hx * a is fused; ly * bottom is rounded, hy * top is fused.
#pragma once

// torch: scale = in / out (correctly rounded)
__device__ __forceinline__ float frame_transform_ratio(int in, int out) { return __fdiv_rn((float)in, (float)out); }

// hx * a + lx * b in one fma: lx * b is rounded first, hx * a is the fused product
__device__ __forceinline__ float frame_transform_lerp(float hx, float a, float lx, float b) { return __fmaf_rn(hx, a, __fmul_rn(lx, b)); }

template <int C>
__device__ __forceinline__ float frame_transform_channel(const unsigned char* p00, const unsigned char* p01, const unsigned char* p10,
                                                         const unsigned char* p11, float hy, float ly, float hx, float lx, float mean,
                                                         float istd) {
    const float inv255 = 1.0f / 255.0f;
    const float a = __fmul_rn((float)p00[C], inv255), b = __fmul_rn((float)p01[C], inv255);
    const float c = __fmul_rn((float)p10[C], inv255), d = __fmul_rn((float)p11[C], inv255);
    const float top = frame_transform_lerp(hx, a, lx, b);
    const float bottom = frame_transform_lerp(hx, c, lx, d);
    const float v = __fmaf_rn(hy, top, __fmul_rn(ly, bottom));
    return __fmul_rn(__fsub_rn(v, mean), istd);
}

// f: the frame's first byte (uint8 [H, W, 3]); (yy, xx): the output pixel in the SCALED image (crop offset already added);
// o[c] = (bilinear(f)[c] / 255 - mean[c]) * istd[c]
__device__ __forceinline__ void frame_transform_pixel(const unsigned char* __restrict__ f, int H, int W, float ry, float rx, int yy, int xx,
                                                      const float (&mean)[3], const float (&istd)[3], float (&o)[3]) {
    float fy = __fmaf_rn(ry, __fadd_rn((float)yy, 0.5f), -0.5f);             // area_pixel_compute_source_index
    float fx = __fmaf_rn(rx, __fadd_rn((float)xx, 0.5f), -0.5f);
    fy = fy < 0.f ? 0.f : fy;
    fx = fx < 0.f ? 0.f : fx;
    const int iy0 = (int)fy, ix0 = (int)fx;
    const int iy1 = iy0 + (iy0 < H - 1 ? 1 : 0), ix1 = ix0 + (ix0 < W - 1 ? 1 : 0);
    const float ly = __fsub_rn(fy, (float)iy0), lx = __fsub_rn(fx, (float)ix0);
    const float hy = __fsub_rn(1.f, ly), hx = __fsub_rn(1.f, lx);
    const unsigned char* p00 = f + ((long long)iy0 * W + ix0) * 3;
    const unsigned char* p01 = f + ((long long)iy0 * W + ix1) * 3;
    const unsigned char* p10 = f + ((long long)iy1 * W + ix0) * 3;
    const unsigned char* p11 = f + ((long long)iy1 * W + ix1) * 3;
    o[0] = frame_transform_channel<0>(p00, p01, p10, p11, hy, ly, hx, lx, mean[0], istd[0]);
    o[1] = frame_transform_channel<1>(p00, p01, p10, p11, hy, ly, hx, lx, mean[1], istd[1]);
    o[2] = frame_transform_channel<2>(p00, p01, p10, p11, hy, ly, hx, lx, mean[2], istd[2]);
}
