// Event evidence of a stream pool (libclipfsar_evidence.so, C ABI in include/ext/clipfsar_evidence.h): the T ring rows of the window
// behind an event record, copied into a slot of a device store in the push that detected it, driven by the detector's records while
// they are still on the device.  Two kernels.  The PLACEMENT pass is one workgroup that walks the records in chunks of CFED_CHUNK in
// record order: an exclusive scan of the "qualifies" flags in LDS on top of a running base ranks them, rank r takes store slot
// (head + r) mod capacity, and the pass writes `where`, one source descriptor per store slot into `work` and, last, the head.  The
// COPY pass has tempo.hip's gather shape turned around: one WAVE per destination row of the store, the lanes striding over the row's
// 16-byte pieces; a row whose slot has no descriptor is left alone.  Its grid is a function of capacity * T alone.
// Every word of where, work, head and every captured store row has exactly one writer (two runs write identical bytes): nothing is
// counted by a shared counter, no workgroup waits on another; plain C++.  The rates travel by value in the placement kernel's arguments, as tempo.hip's do.
// A plug-in library (build.py, PLUGIN_LIBS): it lives beside csrc/, whose files and export sets stay as they are.
#include "../csrc/ring_rows.h"
#include "../csrc/side_lib.h"
#include "../../include/ext/clipfsar_events.h"
#include "../../include/ext/clipfsar_evidence.h"

namespace {

constexpr int THREADS = CFED_CHUNK;
constexpr int WAVE = 64;
constexpr int WAVES = THREADS / WAVE;
constexpr int COLS = CFED_TABLE_COLS;
constexpr int WORK = CFED_WORK_COLS;

struct Rates {
    int r[CFED_MAX_RATES];
};

// rates.r[i], i below R <= 8: a select chain over the by-value struct, so that nothing is indexed in memory (tempo.hip's)
__device__ __forceinline__ int rate_of(const Rates& rates, int i) {
    int v = rates.r[0];
#pragma unroll
    for (int k = 1; k < CFED_MAX_RATES; ++k) v = i == k ? rates.r[k] : v;
    return v;
}

// ---- placement.  ONE workgroup.  Thread x of a chunk owns record i = chunk base + x.  `flags` is double-buffered for the
// Hillis-Steele scan: 8 steps over 256 flags.  Everything a thread dereferences is bounded first: the record by i < n <= max_events,
// the table row by 0 <= row < S, the tempo cell by 0 <= k < NW and 0 <= j < NC of that row (the caller's plane holds OUT0 + NW * NC
// cells), the descriptor by slot < capacity.
__global__ __launch_bounds__(THREADS) void evidence_place_kernel(const int* __restrict__ events, const int* __restrict__ n_events,
                                                                 const int* __restrict__ tempo, const int* __restrict__ table,
                                                                 int* __restrict__ head, int* __restrict__ where, int* __restrict__ work,
                                                                 int S, int max_events, int kinds, int T, int cap, int stride, int rate,
                                                                 int R, int capacity, Rates rates) {
    __shared__ int flags[2][THREADS];
    const int x = threadIdx.x;
    const int n_true = n_events[0];
    const int n = n_true < 0 ? 0 : (n_true < max_events ? n_true : max_events);
    int h = head[0] % capacity;                                // read by every thread before the one write at the end
    h = h < 0 ? h + capacity : h;
    long long base = 0;                                        // qualifying records before this chunk
    for (int c0 = 0; c0 < max_events; c0 += THREADS) {         // block-uniform trip count
        const int i = c0 + x;
        int code = CFED_NOT_CAPTURED, t = 0, k = 0;
        const int* d = table;
        bool q = false;
        if (i < n) {
            const int* e = events + (size_t)i * CFEV_EVENT_COLS;
            const int row = e[0], j = e[1], kind = e[3];
            k = e[2];
            const bool wanted = (kind == CFEV_ONSET && (kinds & CFED_KIND_ONSET)) || (kind == CFEV_OFFSET && (kinds & CFED_KIND_OFFSET));
            if (wanted && row >= 0 && row < S) {
                d = table + (size_t)row * COLS;
                if (k >= 0 && k < d[CFED_NW] && j >= 0 && j < d[CFED_NC]) {
                    if (k < d[CFED_KEEP0]) code = CFED_LEFT_RING;
                    else {
                        q = true;
                        if (tempo != nullptr) {
                            t = tempo[(long long)d[CFED_OUT0] + (long long)k * d[CFED_NC] + j];
                            t = (t < 0 || t >= R) ? R - 1 : t;
                        }
                    }
                }
            }
        }
        int buf = 0;
        flags[0][x] = q ? 1 : 0;
        __syncthreads();
        for (int step = 1; step < THREADS; step <<= 1) {       // inclusive scan
            const int v = flags[buf][x] + (x >= step ? flags[buf][x - step] : 0);
            flags[buf ^ 1][x] = v;
            buf ^= 1;
            __syncthreads();
        }
        const int incl = flags[buf][x], total = flags[buf][THREADS - 1];
        __syncthreads();                                       // the buffers are rewritten by the next chunk
        if (q) {
            const long long rank = base + incl - 1;
            if (rank >= capacity) code = CFED_NO_ROOM;
            else {
                const int slot = (int)(((long long)h + rank) % capacity);
                const int r = tempo != nullptr ? rate_of(rates, t) : rate;
                const long long shift = tempo != nullptr ? (long long)(T - 1) * (rate - r) : 0;
                int* w = work + (size_t)slot * WORK;
                w[0] = d[CFED_SLOT];
                w[1] = (int)(((long long)d[CFED_POS0] + (long long)k * stride + shift) % cap);
                w[2] = r;
                code = slot;
            }
        }
        if (i < max_events) {
            where[(size_t)i * 2] = code;
            where[(size_t)i * 2 + 1] = code >= 0 ? t : 0;
        }
        base += total;
    }
    // the slots this call did not assign: their descriptor says "none".  Slot s was assigned iff (s - h) mod capacity < taken.
    const int taken = base < capacity ? (int)base : capacity;
    for (int s = x; s < capacity; s += THREADS) {
        int off = s - h;
        off = off < 0 ? off + capacity : off;
        if (off >= taken) {
            int* w = work + (size_t)s * WORK;
            w[0] = -1;
            w[1] = 0;
            w[2] = 0;
        }
    }
    if (x == 0) head[0] = (int)(((long long)h + taken) % capacity);
}

__device__ __forceinline__ unsigned wave_id() { return __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE); }

// ---- copy.  Row r of the store is frame j' = r mod T of slot s = r / T.  The descriptor's ring slot is below max_streams and its
// position below cap (the host checked the table, the placement reduced mod cap), and (first + j' * dist) mod cap < cap: every source
// row lies inside the ring.
template <bool VEC>
__global__ __launch_bounds__(THREADS) void evidence_copy_kernel(const float* __restrict__ ring, float* __restrict__ store,
                                                                const int* __restrict__ work, unsigned rows, unsigned T, unsigned pieces,
                                                                unsigned cap) {
    typedef typename Piece<VEC>::type P;
    const unsigned lane = threadIdx.x % WAVE;
    for (unsigned r = blockIdx.x * WAVES + wave_id(); r < rows; r += gridDim.x * WAVES) {
        const unsigned s = r / T, j = r - s * T;
        const int* w = work + (size_t)s * WORK;
        const int slot = w[0];
        if (slot < 0) continue;                                // not assigned in this call: the row keeps its bytes
        const unsigned pos = (unsigned)(((long long)w[1] + (long long)j * w[2]) % cap);
        const P* src = reinterpret_cast<const P*>(ring) + ((size_t)slot * cap + pos) * pieces;
        P* dst = reinterpret_cast<P*>(store) + (size_t)r * pieces;
        for (unsigned p = lane; p < pieces; p += WAVE) dst[p] = src[p];
    }
}

// do the byte ranges [a, a + na) and [b, b + nb) share a byte?
bool overlap(const void* a, long long na, const void* b, long long nb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + (uintptr_t)nb && b0 < a0 + (uintptr_t)na;
}

}  // namespace

extern "C" int cfed_version(void) { return 100; /* 0.1.0 */ }
extern "C" int cfed_abi_version(void) { return CFED_ABI_VERSION; }
extern "C" const char* cfed_last_error(void) { return g_err; }

extern "C" int cfed_workspace_ints(int capacity) {
    const long long n = (long long)capacity * WORK;
    return capacity < 1 || n > MAX_ITEMS ? -1 : (int)n;
}

extern "C" int cfed_capture(const float* ring, const int32_t* events, const int32_t* n_events, const int32_t* tempo, float* store,
                            int32_t* head, int32_t* where, int32_t* work, const int32_t* table_host, const int32_t* table_dev, int S,
                            int max_streams, int cap, int max_events, int kinds, int T, int E, int stride, int rate,
                            const int32_t* rates_host, int R, int capacity, cfed_stream_t stream) {
    SIDE_REQUIRE(ring && events && n_events && store && head && where && work && table_host && table_dev, "cfed_capture: null pointer");
    SIDE_REQUIRE(R >= 0 && R <= CFED_MAX_RATES, "cfed_capture: R=%d rates outside 0 .. %d", R, CFED_MAX_RATES);
    SIDE_REQUIRE((tempo == nullptr) == (R == 0), "cfed_capture: tempo is %s with R=%d -- the plane goes with the rates, NULL with R=0",
                 tempo ? "given" : "NULL", R);
    SIDE_REQUIRE(R == 0 || rates_host, "cfed_capture: null pointer (rates_host with R=%d)", R);
    SIDE_REQUIRE(max_streams >= 1 && max_streams <= CFED_MAX_STREAMS, "cfed_capture: max_streams=%d outside 1 .. %d", max_streams,
                 CFED_MAX_STREAMS);
    SIDE_REQUIRE(S >= 1 && S <= max_streams, "cfed_capture: a table of S=%d rows for max_streams=%d", S, max_streams);
    SIDE_REQUIRE(T >= 1 && E >= 1 && cap >= 1, "cfed_capture: bad shape (T=%d E=%d cap=%d)", T, E, cap);
    SIDE_REQUIRE(stride >= 1, "cfed_capture: stride=%d must be at least 1", stride);
    SIDE_REQUIRE(rate >= 1, "cfed_capture: rate=%d must be at least 1", rate);
    SIDE_REQUIRE(capacity >= 1, "cfed_capture: capacity=%d must be at least 1", capacity);
    SIDE_REQUIRE(max_events >= 1, "cfed_capture: max_events=%d must be at least 1", max_events);
    SIDE_REQUIRE(kinds >= 1 && kinds <= 3, "cfed_capture: kinds=%d outside 1 .. 3 (bit 0: onsets, bit 1: offsets)", kinds);
    SIDE_REQUIRE((long long)capacity * T * E <= MAX_ITEMS, "cfed_capture: a store of capacity=%d x T=%d x E=%d floats is 2^31 or more",
                 capacity, T, E);
    SIDE_REQUIRE((long long)max_streams * cap <= MAX_ITEMS, "cfed_capture: a ring of max_streams=%d x cap=%d rows is 2^31 or more",
                 max_streams, cap);
    Rates rates;
    for (int i = 0; i < CFED_MAX_RATES; ++i) rates.r[i] = i < R ? rates_host[i] : 0;
    if (R > 0) {
        SIDE_REQUIRE(rates.r[0] >= 1, "cfed_capture: rates[0]=%d must be at least 1", rates.r[0]);
        for (int i = 1; i < R; ++i)
            SIDE_REQUIRE(rates.r[i] > rates.r[i - 1], "cfed_capture: rates[%d]=%d after rates[%d]=%d, the rates must be strictly ascending", i,
                         rates.r[i], i - 1, rates.r[i - 1]);
        SIDE_REQUIRE(rates.r[R - 1] == rate, "cfed_capture: rate=%d is not rates[%d]=%d, the largest of the rates", rate, R - 1,
                     rates.r[R - 1]);
    }
    for (int s = 0; s < S; ++s) {
        const int32_t* d = table_host + (size_t)s * COLS;
        SIDE_REQUIRE(d[CFED_SLOT] >= 0 && d[CFED_SLOT] < max_streams, "cfed_capture: row %d has slot %d outside 0 .. %d", s, d[CFED_SLOT],
                     max_streams - 1);
        SIDE_REQUIRE(d[CFED_POS0] >= 0 && d[CFED_POS0] < cap, "cfed_capture: row %d has ring position pos0=%d outside 0 .. cap-1 (cap=%d)", s,
                     d[CFED_POS0], cap);
        SIDE_REQUIRE(d[CFED_NW] >= 0, "cfed_capture: row %d has a negative count (nW=%d)", s, d[CFED_NW]);
        SIDE_REQUIRE(d[CFED_KEEP0] >= 0 && d[CFED_KEEP0] <= d[CFED_NW], "cfed_capture: row %d has keep0=%d outside 0 .. nW=%d", s,
                     d[CFED_KEEP0], d[CFED_NW]);
        SIDE_REQUIRE(d[CFED_NC] >= 1, "cfed_capture: row %d has nc=%d columns, at least 1 is needed", s, d[CFED_NC]);
        SIDE_REQUIRE(d[CFED_OUT0] >= 0, "cfed_capture: row %d has a negative cell offset (out0=%d)", s, d[CFED_OUT0]);
        if (d[CFED_KEEP0] < d[CFED_NW]) {
            const long long span = (long long)(d[CFED_NW] - 1 - d[CFED_KEEP0]) * stride + (long long)(T - 1) * rate + 1;
            SIDE_REQUIRE(span <= cap, "cfed_capture: row %d: the %lld frames of its windows keep0=%d .. nW=%d do not fit a ring of cap=%d", s,
                         span, d[CFED_KEEP0], d[CFED_NW], cap);
        }
    }
    SIDE_REQUIRE(!overlap(ring, (long long)max_streams * cap * E * 4, store, (long long)capacity * T * E * 4),
                 "cfed_capture: store overlaps ring -- the evidence is a copy, give it a buffer of its own");
    const bool vec = vec_ok(ring, store, E);
    const unsigned pieces = (unsigned)(vec ? E / 4 : E);
    const long long rows = (long long)capacity * T;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(evidence_place_kernel, dim3(1), dim3(THREADS), 0, s, events, n_events, tempo, table_dev, head, where, work, S,
                       max_events, kinds, T, cap, stride, rate, R, capacity, rates);
    if (check_launch("cfed_capture")) return 1;
    if (vec)
        hipLaunchKernelGGL(evidence_copy_kernel<true>, dim3(blocks_for(rows, WAVES)), dim3(THREADS), 0, s, ring, store, work, (unsigned)rows,
                           (unsigned)T, pieces, (unsigned)cap);
    else
        hipLaunchKernelGGL(evidence_copy_kernel<false>, dim3(blocks_for(rows, WAVES)), dim3(THREADS), 0, s, ring, store, work, (unsigned)rows,
                           (unsigned)T, pieces, (unsigned)cap);
    return check_launch("cfed_capture");
}
