// The row search of the launches over the 6-column descriptor table of per-class smoothing (include/ext/clipfsar_class_smooth.h): one
// workgroup per (table row, chunk of columns), the row found in the table's CHUNK0 column.  For the libraries of build.py's PLUGIN_LIBS
// (baseline.hip); class_smooth.hip and events.hip keep the copies they were built and measured with.
#pragma once
#include <stdint.h>

// the table row whose CHUNK0 is the last one <= b (every row has NC >= 1, so CHUNK0 rises strictly) -> its number.  `cols` values per
// row, CHUNK0 at `chunk0`.  The workgroup number b is uniform, so the search runs on scalar values.
__device__ __forceinline__ unsigned find_chunk_row(const int32_t* __restrict__ table, unsigned S, unsigned b, unsigned cols, unsigned chunk0) {
    unsigned lo = 0, hi = S;                   // table[lo][CHUNK0] <= b; hi == S or table[hi][CHUNK0] > b
    while (hi - lo > 1) {
        const unsigned mid = (lo + hi) >> 1;
        if ((unsigned)table[mid * cols + chunk0] <= b) lo = mid;
        else hi = mid;
    }
    return lo;
}
