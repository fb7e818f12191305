// Top-k of one row of logits by one wave: the body of topk_kernel (gallery.hip) and of topk_grouped_kernel (groups.hip).  Each lane keeps
// the best TOPK_MAX of its strided classes (a compare-exchange chain with constant indices: registers only), then k rounds of a wave-wide
// arg-max over the lanes' heads.  Order: larger value first, the lower class index on ties (a stable descending sort).  A NaN logit is
// never selected, and neither is one of -inf: -inf is the value of an empty place, whose index is 0x7fffffff (no class).  The loop skips
// both; before it did, a -inf class was kept with its index when its lane already held a class and lost it to 0x7fffffff when it was the
// lane's first.
#pragma once
#include "common.h"

constexpr int TOPK_MAX = 16;
__device__ __forceinline__ bool topk_better(float a, int ia, float b, int ib) { return a > b || (a == b && ia < ib); }

// row [C] -> values [k], index [k] (of the same query); all 64 lanes of the wave call it, lane = their number
__device__ __forceinline__ void topk_wave(const float* __restrict__ row, int C, int k, float* __restrict__ values,
                                          int32_t* __restrict__ index, int lane) {
    float v[TOPK_MAX];
    int ix[TOPK_MAX];
#pragma unroll
    for (int j = 0; j < TOPK_MAX; ++j) { v[j] = -__builtin_inff(); ix[j] = 0x7fffffff; }
    for (int c = lane; c < C; c += 64) {
        float x = row[c];
        int xi = c;
        if (!(x > -__builtin_inff())) continue;            // NaN or -inf: not selectable
#pragma unroll
        for (int j = 0; j < TOPK_MAX; ++j) {
            if (topk_better(x, xi, v[j], ix[j])) {
                const float tv = v[j];
                const int ti = ix[j];
                v[j] = x; ix[j] = xi; x = tv; xi = ti;
            }
        }
    }
    for (int r = 0; r < k; ++r) {
        float bv = v[0];
        int bi = ix[0];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(bv, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (topk_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
        }
        if (lane == 0) {
            values[r] = bv;
            index[r] = bi;
        }
        if (ix[0] == bi) {                                 // the winner's lane pops its head
#pragma unroll
            for (int j = 0; j < TOPK_MAX - 1; ++j) { v[j] = v[j + 1]; ix[j] = ix[j + 1]; }
            v[TOPK_MAX - 1] = -__builtin_inff();
            ix[TOPK_MAX - 1] = 0x7fffffff;
        }
    }
}
