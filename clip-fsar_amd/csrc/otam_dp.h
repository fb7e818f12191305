// OTAM soft-min DP (few_shot.py:2657-2687), un-stabilised like the reference: the one recurrence of cos_otam_kernel (tail.hip) and of
// otam_tile (otam_tile.h: otam_gallery_kernel in gallery.hip, otam_indexed_kernel in live.hip), so equal distance blocks give bit-equal
// results in all of them.
#pragma once
#include <hip/hip_runtime.h>

constexpr int MAX_T = 32;
// TT > 0: T is the compile-time constant TT, every loop unrolls and the two DP rows live in registers.  TT == 0: run-time T, the
// rows live in the caller's LDS scratch `rows` (2 rows, `rstride` floats apart, rstride >= T + 2, per thread) -- never in scratch
// memory: the recurrence is one dependent chain of T*T cells, and a scratch round trip per cell made cos_otam_kernel 140 us for an
// 8x8 problem.
template <int TT>
__device__ __forceinline__ float otam_dp(const float* d /*[T][T] row stride rs, col stride cs*/, int rs, int cs, int Trt, float lbda,
                                         float* rows, int rstride) {
    const int T = TT > 0 ? TT : Trt;
    // padded width M = T+2; columns 0 and T+1 are zero padding (few_shot.py:2663)
    float regs[TT > 0 ? 2 * (TT + 2) : 1];
    float* prev = TT > 0 ? regs : rows;
    float* cur = TT > 0 ? regs + (TT + 2) : rows + rstride;
    const float il = 1.0f / lbda;
    prev[0] = 0.f;
#pragma unroll
    for (int m = 1; m <= T + 1; ++m) {                      // first row: running sum (:2668-2671)
        const float dv = (m <= T) ? d[0 * rs + (m - 1) * cs] : 0.f;
        prev[m] = dv + prev[m - 1];
    }
#pragma unroll
    for (int l = 1; l < T; ++l) {
        cur[0] = 0.f;
        {   // first non-zero column (:2675)
            const float dv = d[l * rs + 0 * cs];
            cur[1] = dv - lbda * logf(expf(-prev[0] * il) + expf(-prev[1] * il) + expf(-cur[0] * il));
        }
#pragma unroll
        for (int m = 2; m <= T; ++m) {                      // middle columns (:2678-2679)
            const float dv = d[l * rs + (m - 1) * cs];
            cur[m] = dv - lbda * logf(expf(-prev[m - 1] * il) + expf(-cur[m - 1] * il));
        }
        // last (padding) column (:2683)
        cur[T + 1] = 0.f - lbda * logf(expf(-prev[T] * il) + expf(-prev[T + 1] * il) + expf(-cur[T] * il));
#pragma unroll
        for (int m = 0; m <= T + 1; ++m) prev[m] = cur[m];
    }
    return prev[T + 1];
}
