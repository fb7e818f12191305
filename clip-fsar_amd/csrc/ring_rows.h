// What the ring libraries share (stream.hip: B lockstep streams; pool.hip: sessions of a descriptor table): the row pieces and launch
// limits of their copy kernels -- which keep thread mappings of their own -- and the smoothing recurrence, so that both libraries give
// the same bits on the same windows.
#pragma once
#include <stdint.h>

#include "common.h"

constexpr unsigned MAX_BLOCKS = 4096;          // grid-stride beyond: 16 workgroups per CU of rows in flight is past what HBM needs
constexpr long long MAX_ITEMS = 0x7fffffffLL;  // the kernels index rows, row pieces and windows with 32 bits

// a row piece: 16 bytes when the rows allow it, 4 otherwise
template <bool VEC> struct Piece { typedef float type; };
template <> struct Piece<true> { typedef float4 type; };

inline bool vec_ok(const void* a, const void* b, int E) { return E % 4 == 0 && (((uintptr_t)a | (uintptr_t)b) & 15u) == 0; }

inline unsigned blocks_for(long long items, int per_block) {
    const long long b = (items + per_block - 1) / per_block;
    return (unsigned)(b < MAX_BLOCKS ? b : MAX_BLOCKS);
}

// The smoothing of one (stream, class): nW windows C floats apart, sequential in k, from *state when have_state and into it.  om is
// 1 - alpha rounded to fp32; (1 - alpha) * x is rounded to fp32, then ONE fma per step.  o may be x: the calling thread alone touches
// the elements.
__device__ __forceinline__ void smooth_run(const float* x, float* o, float* state, unsigned nW, unsigned C, float alpha,
                                           float om, bool have_state) {
    float y = have_state ? *state : 0.f;
    for (unsigned k = 0; k < nW; ++k) {
        const float xk = x[(size_t)k * C];
        y = (k == 0 && !have_state) ? xk : __fmaf_rn(alpha, y, __fmul_rn(om, xk));
        o[(size_t)k * C] = y;
    }
    *state = y;
}
