// The shot ledger of a live gallery (libclipfsar_ledger.so, C ABI in include/ext/clipfsar_ledger.h): a store [shots, rows_kept, E] of
// every shot's ADDEND -- the rows cfsl_accumulate (csrc/live.hip) summed for it -- and the three kernels over it.
// ledger_put_kernel copies a call's addends into the store slots a per-video list names: one WAVE per row, the lanes striding over the
// row's 16-byte pieces (evidence.hip's copy shape).  ledger_resum_kernel forms a touched class's sum again from the addends that
// remain: one workgroup per (table row, kept row), accumulate_kernel's shape and, with prior = 0, its operation order -- a = 0, then
// a += addend in list order, then a * (1 / n) -- so the bits are those cfsl_accumulate gives on the same addends.  ledger_fit_kernel is
// the leave-one-out audit: one workgroup per shot, each of its waves taking rows r < T in turn; per row three dots of
// slot_norms_kernel's kind (a lane-strided fmaf chain, here over 16-byte pieces, closed by wave_sum) give the cosine between the shot
// and the rest of its class, and one lane sums the T cosines in row order.
// Every output word has one writer and nothing is counted by a shared counter: two runs write identical bytes.  A table row the host
// would have refused, and a ledger slot outside the store, write nothing.  Plain C++.
// A plug-in library (build.py, PLUGIN_LIBS): it lives beside csrc/, whose files and export sets stay as they are.
#include "../csrc/side_lib.h"
#include "../../include/ext/clipfsar_ledger.h"

#include <math.h>

namespace {

constexpr int COLS = CFLD_TABLE_COLS;
constexpr int WAVE = 64;
constexpr int PUT_WG = 256, PUT_WAVES = PUT_WG / WAVE;
constexpr int SUM_WG = 128;
constexpr int FIT_WG = 256, FIT_WAVES = FIT_WG / WAVE;
constexpr unsigned MAX_GRID = 1u << 20;               // the put's workgroups: a longer call's waves take several rows

__device__ __forceinline__ unsigned wave_id() { return __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE); }

// ---- put.  Row q of the call is kept row r = q mod rows_kept of video v = q / rows_kept.
__global__ __launch_bounds__(PUT_WG) void ledger_put_kernel(const float4* __restrict__ X, float4* __restrict__ store,
                                                            const int32_t* __restrict__ slots, unsigned rows, unsigned L, unsigned pieces,
                                                            unsigned shots, unsigned rows_kept) {
    const unsigned lane = threadIdx.x % WAVE;
    for (unsigned q = blockIdx.x * PUT_WAVES + wave_id(); q < rows; q += gridDim.x * PUT_WAVES) {
        const unsigned v = q / rows_kept, r = q - v * rows_kept;
        const unsigned slot = (unsigned)slots[v];
        if (slot >= shots) continue;                           // not kept: nothing is written
        const float4* src = X + ((size_t)v * L + r) * pieces;
        float4* dst = store + ((size_t)slot * rows_kept + r) * pieces;
        for (unsigned p = lane; p < pieces; p += WAVE) dst[p] = src[p];
    }
}

// the table row s as the kernels trust it: a class slot inside the gallery's store and a run inside the list
__device__ __forceinline__ bool row_ok(const int32_t* row, int cap, int n_list) {
    const int slot = row[CFLD_SLOT], first = row[CFLD_FIRST], n = row[CFLD_N];
    return (unsigned)slot < (unsigned)cap && first >= 0 && n >= 1 && n <= n_list - first;
}

// ---- resum: one workgroup per (table row, kept row)
__global__ __launch_bounds__(SUM_WG) void ledger_resum_kernel(const float* __restrict__ store, const int32_t* __restrict__ list,
                                                              float* __restrict__ sums, float* __restrict__ means,
                                                              const int32_t* __restrict__ table, int n_list, int shots, int rows_kept, int L,
                                                              int E, int cap, int means_by_slot) {
    const int s = blockIdx.x / rows_kept, r = blockIdx.x - s * rows_kept, tid = threadIdx.x;
    const int32_t* row = table + (size_t)s * COLS;
    if (!row_ok(row, cap, n_list)) return;
    const int slot = row[CFLD_SLOT], lo = row[CFLD_FIRST], hi = lo + row[CFLD_N];
    for (int i = lo; i < hi; ++i)
        if ((unsigned)list[i] >= (unsigned)shots) return;      // (uniform) a ledger slot outside the store: the class keeps its sum
    const float inv = 1.0f / (float)(hi - lo);
    float* sm = sums + ((size_t)slot * L + r) * E;
    float* o = means + ((size_t)(means_by_slot ? slot : s) * rows_kept + r) * E;
    for (int e = tid; e < E; e += SUM_WG) {
        float a = 0.f;
        for (int i = lo; i < hi; ++i) a += store[((size_t)list[i] * rows_kept + r) * E + e];
        sm[e] = a;
        o[e] = a * inv;
    }
}

// ---- fit: one workgroup per list position p.  Its table row is the last one whose FIRST is at most p (the host checked that FIRST is
// the running sum of N >= 1, so FIRST ascends strictly): a bisection of at most 17 steps over at most 65536 rows.
__global__ __launch_bounds__(FIT_WG) void ledger_fit_kernel(const float* __restrict__ store, const float* __restrict__ sums,
                                                            const int32_t* __restrict__ list, float* __restrict__ fit,
                                                            const int32_t* __restrict__ table, int S, int n_list, int shots, int rows_kept,
                                                            int L, int T, int pieces, int cap) {
    __shared__ float cosine[CFLD_MAX_T];
    const int p = blockIdx.x, lane = threadIdx.x % WAVE;
    int a = 0, b = S;
    for (int step = 0; step < 17 && b - a > 1; ++step) {
        const int mid = (a + b) >> 1;
        if (table[(size_t)mid * COLS + CFLD_FIRST] <= p) a = mid;
        else b = mid;
    }
    const int32_t* row = table + (size_t)a * COLS;
    if (!row_ok(row, cap, n_list)) return;                     // (uniform, as every exit before the barrier is)
    const int n = row[CFLD_N], first = row[CFLD_FIRST];
    if (p < first || p >= first + n) return;
    const unsigned shot = (unsigned)list[p];
    if (shot >= (unsigned)shots) return;
    const float4* x0 = reinterpret_cast<const float4*>(store) + (size_t)shot * rows_kept * pieces;
    const float4* s0 = reinterpret_cast<const float4*>(sums) + (size_t)row[CFLD_SLOT] * L * pieces;
    for (int r = (int)wave_id(); r < T; r += FIT_WAVES) {
        const float4* x = x0 + (size_t)r * pieces;
        const float4* sm = s0 + (size_t)r * pieces;
        float xx = 0.f, mm = 0.f, xm = 0.f;
        for (int q = lane; q < pieces; q += WAVE) {
            const float4 xv = x[q], sv = sm[q];
            const float m0 = sv.x - xv.x, m1 = sv.y - xv.y, m2 = sv.z - xv.z, m3 = sv.w - xv.w;
            xx = fmaf(xv.x, xv.x, xx); xx = fmaf(xv.y, xv.y, xx); xx = fmaf(xv.z, xv.z, xx); xx = fmaf(xv.w, xv.w, xx);
            mm = fmaf(m0, m0, mm); mm = fmaf(m1, m1, mm); mm = fmaf(m2, m2, mm); mm = fmaf(m3, m3, mm);
            xm = fmaf(xv.x, m0, xm); xm = fmaf(xv.y, m1, xm); xm = fmaf(xv.z, m2, xm); xm = fmaf(xv.w, m3, xm);
        }
        xx = wave_sum(xx);
        mm = wave_sum(mm);
        xm = wave_sum(xm);
        if (lane == 0) cosine[r] = xm / sqrtf(xx * mm);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float acc = 0.f;
        for (int r = 0; r < T; ++r) acc += cosine[r];
        fit[p] = n == 1 ? __builtin_nanf("") : acc * (1.0f / (float)T);     // one shot: nothing to compare with
    }
}

// the host rows of a table: class slots in [0, cap), each at most once; N >= 1; FIRST the running sum, n_list in all
int check_table(const char* who, const int32_t* t, int S, int cap, int n_list) {
    SIDE_REQUIRE(S >= 1 && S <= CFLD_MAX_ROWS && S <= cap, "%s: a table of %d rows (1 .. min(%d, cap = %d))", who, S, CFLD_MAX_ROWS, cap);
    SlotBits seen(cap);
    SIDE_REQUIRE(seen.ok(), "%s: out of host memory for %d slots", who, cap);
    long long at = 0;
    for (int s = 0; s < S; ++s) {
        const int32_t* row = t + (size_t)s * COLS;
        const int slot = row[CFLD_SLOT];
        SIDE_REQUIRE(slot >= 0 && slot < cap, "%s: row %d: slot %d outside [0, %d)", who, s, slot, cap);
        SIDE_REQUIRE(!seen.test_and_set(slot), "%s: row %d: slot %d appears twice in the table", who, s, slot);
        SIDE_REQUIRE(row[CFLD_N] >= 1, "%s: row %d: a class of %d shots, at least 1 is needed", who, s, row[CFLD_N]);
        SIDE_REQUIRE(row[CFLD_FIRST] == at, "%s: row %d: FIRST = %d is not the running sum %lld of the counts before", who, s,
                     row[CFLD_FIRST], at);
        at += row[CFLD_N];
    }
    SIDE_REQUIRE(at == n_list, "%s: the classes' shots add up to %lld, not to n_list = %d", who, at, n_list);
    return 0;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

bool overlap(const void* a, long long na, const void* b, long long nb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + (uintptr_t)nb && b0 < a0 + (uintptr_t)na;
}

}  // namespace

extern "C" int cfld_version(void) { return 100; /* 0.1.0 */ }
extern "C" int cfld_abi_version(void) { return CFLD_ABI_VERSION; }
extern "C" const char* cfld_last_error(void) { return g_err; }

extern "C" int cfld_put(const float* X, float* store, const int32_t* slots, int Nv, int L, int E, int shots, int rows_kept,
                        cfld_stream_t stream) {
    SIDE_REQUIRE(X && store && slots, "cfld_put: null pointer (X, store or slots)");
    SIDE_REQUIRE(Nv >= 1 && L >= 1 && shots >= 1 && rows_kept >= 1 && rows_kept <= L,
                 "cfld_put: bad shape (Nv=%d L=%d shots=%d rows_kept=%d; all >= 1, rows_kept <= L)", Nv, L, shots, rows_kept);
    SIDE_REQUIRE(E >= 4 && E % 4 == 0, "cfld_put: E=%d must be a multiple of 4, at least 4", E);
    SIDE_REQUIRE(aligned16(X) && aligned16(store), "cfld_put: X and store must be 16-byte aligned");
    const long long rows = (long long)Nv * rows_kept;
    SIDE_REQUIRE(rows <= 0x7fffffffLL, "cfld_put: Nv * rows_kept = %lld rows exceed 32-bit sizes", rows);
    SIDE_REQUIRE(!overlap(X, (long long)Nv * L * E * 4, store, (long long)shots * rows_kept * E * 4),
                 "cfld_put: store overlaps X -- the ledger keeps a copy, give it a buffer of its own");
    const long long want = (rows + PUT_WAVES - 1) / PUT_WAVES;
    const unsigned grid = (unsigned)(want < (long long)MAX_GRID ? want : (long long)MAX_GRID);
    hipLaunchKernelGGL(ledger_put_kernel, dim3(grid), dim3(PUT_WG), 0, static_cast<hipStream_t>(stream),
                       reinterpret_cast<const float4*>(X), reinterpret_cast<float4*>(store), slots, (unsigned)rows, (unsigned)L,
                       (unsigned)(E / 4), (unsigned)shots, (unsigned)rows_kept);
    return check_launch("cfld_put");
}

extern "C" int cfld_resum(const float* store, const int32_t* list, float* sums, float* means, const int32_t* table_host,
                          const int32_t* table_dev, int S, int n_list, int shots, int rows_kept, int L, int E, int cap, int means_by_slot,
                          cfld_stream_t stream) {
    SIDE_REQUIRE(store && list && sums && means && table_host && table_dev,
                 "cfld_resum: null pointer (store, list, sums, means, table_host or table_dev)");
    SIDE_REQUIRE(n_list >= 1 && shots >= 1 && L >= 1 && E >= 1 && cap >= 1 && rows_kept >= 1 && rows_kept <= L,
                 "cfld_resum: bad shape (n_list=%d shots=%d rows_kept=%d L=%d E=%d cap=%d; all >= 1, rows_kept <= L)", n_list, shots,
                 rows_kept, L, E, cap);
    if (check_table("cfld_resum", table_host, S, cap, n_list)) return 1;
    const long long blocks = (long long)S * rows_kept;
    SIDE_REQUIRE(blocks <= 0x7fffffffLL, "cfld_resum: %lld output rows exceed 32-bit sizes", blocks);
    hipLaunchKernelGGL(ledger_resum_kernel, dim3((unsigned)blocks), dim3(SUM_WG), 0, static_cast<hipStream_t>(stream), store, list, sums,
                       means, table_dev, n_list, shots, rows_kept, L, E, cap, means_by_slot);
    return check_launch("cfld_resum");
}

extern "C" int cfld_fit(const float* store, const float* sums, const int32_t* list, float* fit, const int32_t* table_host,
                        const int32_t* table_dev, int S, int n_list, int shots, int rows_kept, int L, int T, int E, int cap,
                        cfld_stream_t stream) {
    SIDE_REQUIRE(store && sums && list && fit && table_host && table_dev,
                 "cfld_fit: null pointer (store, sums, list, fit, table_host or table_dev)");
    SIDE_REQUIRE(n_list >= 1 && shots >= 1 && L >= 1 && cap >= 1 && rows_kept >= 1 && rows_kept <= L,
                 "cfld_fit: bad shape (n_list=%d shots=%d rows_kept=%d L=%d cap=%d; all >= 1, rows_kept <= L)", n_list, shots, rows_kept, L,
                 cap);
    SIDE_REQUIRE(T >= 1 && T <= CFLD_MAX_T && T <= rows_kept, "cfld_fit: T=%d rows outside 1 .. min(%d, rows_kept = %d)", T, CFLD_MAX_T,
                 rows_kept);
    SIDE_REQUIRE(E >= 4 && E % 4 == 0, "cfld_fit: E=%d must be a multiple of 4, at least 4", E);
    SIDE_REQUIRE(aligned16(store) && aligned16(sums), "cfld_fit: store and sums must be 16-byte aligned");
    if (check_table("cfld_fit", table_host, S, cap, n_list)) return 1;
    hipLaunchKernelGGL(ledger_fit_kernel, dim3((unsigned)n_list), dim3(FIT_WG), 0, static_cast<hipStream_t>(stream), store, sums, list, fit,
                       table_dev, S, n_list, shots, rows_kept, L, T, E / 4, cap);
    return check_launch("cfld_fit");
}
