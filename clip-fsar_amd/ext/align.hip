// The OTAM soft alignment behind a score (libclipfsar_align.so, C ABI in include/ext/clipfsar_align.h): per (query, store slot) pair the
// T x T cosine-distance matrix D, the value F(D) + F(D^T) whose negative is the pair's logit, and the gradient dF/dD -- cell (l, m) is
// the probability that the soft path pairs query frame l with prototype frame m.  The scoring kernels (otam_dp.h's recurrence) are
// un-stabilised forward passes that throw D away; this is another recurrence, restated here: the soft-min is taken relative to its
// smallest argument, so that expf stays in range where the un-stabilised fp32 form underflows, and a backward pass follows the forward.
// One 256-thread workgroup per pair.  1: the four waves compute the T * T dot products -- a wave owns query rows, a lane 16-byte pieces
// of a row, products accumulated in double in an order that E alone decides, then the wave's butterfly -- and write D to LDS.  2: wave 0
// runs D, wave 1 runs D^T (the same LDS block read with the strides swapped): forward into c, kept whole because the backward pass reads
// it, then the adjoints row by row from the last, two rows of them alive.  The recurrence is one dependent chain, so one lane walks it.
// 3: all threads add the two directions' gradients into plan.  Every cell has one writer, every loop is bounded by T or E and every sum
// has a fixed order: two runs write the same bytes.
// A plug-in library (build.py, PLUGIN_LIBS): it lives beside csrc/, whose files and export sets stay as they are.
#include "../csrc/side_lib.h"
#include "../../include/ext/clipfsar_align.h"

#include <math.h>

// every fp32 operation of the definitions is one rounded operation: a product is never fused into the sum it feeds
#pragma clang fp contract(off)

namespace {

constexpr int WG = 256, WAVES = 4;
constexpr int MAX_T = CFAL_MAX_T;
constexpr int CW = MAX_T + 2;                                                 // a row of the padded grid: columns 0 and T + 1 are padding
constexpr int MB = 4;                                                         // prototype rows a wave takes against one query row at a time
constexpr long long MAX_32 = 0x7fffffffLL;

__device__ __forceinline__ float rel(float x, float mn, float lam) { return expf(__fdiv_rn(mn - x, lam)); }

__device__ __forceinline__ float softmin2(float x1, float x2, float lam) {
    const float mn = fminf(x1, x2);
    return mn - lam * logf(rel(x1, mn, lam) + rel(x2, mn, lam));
}

__device__ __forceinline__ float softmin3(float x1, float x2, float x3, float lam) {
    const float mn = fminf(fminf(x1, x2), x3);
    return mn - lam * logf(rel(x1, mn, lam) + rel(x2, mn, lam) + rel(x3, mn, lam));
}

// One direction, one lane: d(l, m) = D[l * rs + m * cs].  c [T][CW]: the padded grid, written whole; a [2][CW]: the adjoints of the
// row being read and of the row above; G [T * T] row-major in this direction's own (l, m).  -> F.
__device__ float forward_backward(const float* D, int rs, int cs, int T, float lam, float* c, float* a, float* G) {
    // ---- forward
    c[0] = 0.f;
    for (int m = 1; m <= T; ++m) c[m] = D[(m - 1) * cs] + c[m - 1];           // row 0: a running sum
    c[T + 1] = 0.f + c[T];
    for (int l = 1; l < T; ++l) {
        const float* up = c + (l - 1) * CW;
        float* cur = c + l * CW;
        const float* d = D + l * rs;
        cur[0] = 0.f;
        float left = d[0] + softmin3(up[0], up[1], 0.f, lam);
        cur[1] = left;
        for (int m = 2; m <= T; ++m) {
            left = d[(m - 1) * cs] + softmin2(up[m - 1], left, lam);
            cur[m] = left;
        }
        cur[T + 1] = 0.f + softmin3(up[T], up[T + 1], left, lam);
    }
    const float F = c[(T - 1) * CW + T + 1];
    // ---- backward
    float* an = a;                                                            // the adjoints of row l
    float* au = a + CW;                                                       // and of row l - 1, gathered as row l is read
    for (int m = 0; m <= T; ++m) an[m] = 0.f;
    an[T + 1] = 1.f;
    for (int l = T - 1; l >= 1; --l) {
        const float* up = c + (l - 1) * CW;
        const float* cur = c + l * CW;
        const float* d = D + l * rs;
        for (int m = 0; m <= T + 1; ++m) au[m] = 0.f;
        {                                                                     // m = T + 1: predecessors (l-1, T), (l-1, T+1), (l, T)
            const float am = an[T + 1], s = cur[T + 1] - 0.f;
            au[T] = au[T] + am * rel(up[T], s, lam);
            au[T + 1] = au[T + 1] + am * rel(up[T + 1], s, lam);
            an[T] = an[T] + am * rel(cur[T], s, lam);
        }
        for (int m = T; m >= 2; --m) {                                        // predecessors (l-1, m-1), (l, m-1)
            const float am = an[m], s = cur[m] - d[(m - 1) * cs];
            G[l * T + m - 1] = am;
            au[m - 1] = au[m - 1] + am * rel(up[m - 1], s, lam);
            an[m - 1] = an[m - 1] + am * rel(cur[m - 1], s, lam);
        }
        {                                                                     // m = 1: (l-1, 0) and (l, 0) are padding, (l-1, 1) is not
            const float am = an[1], s = cur[1] - d[0];
            G[l * T] = am;
            au[1] = au[1] + am * rel(up[1], s, lam);
        }
        float* t = an;
        an = au;
        au = t;
    }
    float run = 0.f;                                                          // row 0 is a running sum: every later cell holds d[0][j]
    for (int m = T + 1; m >= 1; --m) {
        run = run + an[m];
        if (m <= T) G[m - 1] = run;
    }
    return F;
}

__global__ __launch_bounds__(WG) void otam_align_kernel(const float* __restrict__ Xq, const float* __restrict__ qn,
                                                        const float* __restrict__ P, const float* __restrict__ pn,
                                                        const int32_t* __restrict__ pair_q, const int32_t* __restrict__ pair_slot, int NQ,
                                                        int cap, int T, int E, float lam, int single_direct, float* __restrict__ plan,
                                                        float* __restrict__ dists, float* __restrict__ logits) {
    __shared__ float D[MAX_T * MAX_T];
    __shared__ float C[2][MAX_T * CW];
    __shared__ float A[2][2 * CW];
    __shared__ float G[2][MAX_T * MAX_T];
    __shared__ float F[2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t pair = blockIdx.x;
    const int TT = T * T;
    const unsigned qi = (unsigned)pair_q[pair], slot = (unsigned)pair_slot[pair];
    float* out_plan = plan + pair * TT;
    float* out_d = dists ? dists + pair * TT : nullptr;
    if (qi >= (unsigned)NQ || slot >= (unsigned)cap) {                        // uniform: a pair outside the inputs is never dereferenced
        const float nan = __builtin_nanf("");
        for (int i = tid; i < TT; i += WG) {
            out_plan[i] = nan;
            if (out_d) out_d[i] = nan;
        }
        if (tid == 0) logits[pair] = nan;
        return;
    }
    // ---- 1. the distances: a wave per query row, MB prototype rows at a time against one load of the query's piece
    const float* xq = Xq + (size_t)qi * T * E;
    const float* xp = P + (size_t)slot * T * E;
    const float* nq = qn + (size_t)qi * T;
    const float* np = pn + (size_t)slot * T;
    for (int l = wave; l < T; l += WAVES) {
        const float* q = xq + (size_t)l * E;
        const float qnl = nq[l];
        for (int m0 = 0; m0 < T; m0 += MB) {
            const float* p[MB];
            double acc[MB];
#pragma unroll
            for (int j = 0; j < MB; ++j) {
                p[j] = xp + (size_t)min(m0 + j, T - 1) * E;                   // a row past the last one: the last one again, not written
                acc[j] = 0.0;
            }
            for (int e = lane * 4; e < E; e += 64 * 4) {
                const float4 u = *reinterpret_cast<const float4*>(q + e);
#pragma unroll
                for (int j = 0; j < MB; ++j) {
                    const float4 v = *reinterpret_cast<const float4*>(p[j] + e);
                    acc[j] = acc[j] + (double)u.x * (double)v.x;
                    acc[j] = acc[j] + (double)u.y * (double)v.y;
                    acc[j] = acc[j] + (double)u.z * (double)v.z;
                    acc[j] = acc[j] + (double)u.w * (double)v.w;
                }
            }
#pragma unroll
            for (int j = 0; j < MB; ++j) {
#pragma unroll
                for (int o = 32; o >= 1; o >>= 1) acc[j] = acc[j] + __shfl_xor(acc[j], o, 64);
                if (lane == 0 && m0 + j < T) D[l * T + m0 + j] = 1.0f - __fdiv_rn((float)acc[j], qnl * np[m0 + j] + 0.01f);
            }
        }
    }
    __syncthreads();
    // ---- 2. a wave per direction: D as it is, and D^T by swapped strides
    const int n_dir = single_direct ? 1 : 2;
    if (wave < n_dir && lane == 0) F[wave] = forward_backward(D, wave ? 1 : T, wave ? T : 1, T, lam, C[wave], A[wave], G[wave]);
    __syncthreads();
    // ---- 3. the outputs
    for (int i = tid; i < TT; i += WG) {
        float g = G[0][i];
        if (n_dir == 2) g = g + G[1][(i % T) * T + i / T];
        out_plan[i] = g;
        if (out_d) out_d[i] = D[i];
    }
    if (tid == 0) logits[pair] = n_dir == 2 ? -(F[0] + F[1]) : -F[0];
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace

extern "C" int cfal_version(void) { return 100; /* 0.1.0 */ }
extern "C" int cfal_abi_version(void) { return CFAL_ABI_VERSION; }
extern "C" const char* cfal_last_error(void) { return g_err; }

extern "C" int cfal_align(const float* Xq, const float* qn, const float* P, const float* pn, const int32_t* pair_q, const int32_t* pair_slot,
                          int NP, int NQ, int cap, int T, int E, float lambda, int single_direct, float* plan, float* dists_or_null,
                          float* logits, cfal_stream_t stream) {
    const char* who = "cfal_align";
    SIDE_REQUIRE(Xq && qn && P && pn && pair_q && pair_slot && plan && logits, "%s: null pointer (dists alone may be null)", who);
    SIDE_REQUIRE(NP >= 1, "%s: NP=%d pairs, at least 1 is needed", who, NP);
    SIDE_REQUIRE(NQ >= 1, "%s: NQ=%d queries, at least 1 is needed", who, NQ);
    SIDE_REQUIRE(cap >= 1, "%s: cap=%d slots, at least 1 is needed", who, cap);
    SIDE_REQUIRE(T >= 1 && T <= CFAL_MAX_T, "%s: T=%d outside 1 .. %d", who, T, CFAL_MAX_T);
    SIDE_REQUIRE(E >= CFAL_MIN_E && E <= CFAL_MAX_E && E % 4 == 0, "%s: E=%d must be a multiple of 4 in %d .. %d", who, E, CFAL_MIN_E,
                 CFAL_MAX_E);
    SIDE_REQUIRE((long long)NP * T * T <= MAX_32, "%s: NP * T * T = %lld plan cells exceed 32-bit sizes", who, (long long)NP * T * T);
    SIDE_REQUIRE((long long)NQ * T <= MAX_32, "%s: NQ * T = %lld query rows exceed 32-bit sizes", who, (long long)NQ * T);
    SIDE_REQUIRE((long long)cap * T <= MAX_32, "%s: cap * T = %lld prototype rows exceed 32-bit sizes", who, (long long)cap * T);
    SIDE_REQUIRE(lambda > 0.f && lambda <= 3.402823466e38f, "%s: lambda=%g must be positive and finite", who, (double)lambda);
    SIDE_REQUIRE(single_direct == 0 || single_direct == 1, "%s: single_direct=%d must be 0 or 1", who, single_direct);
    SIDE_REQUIRE(aligned16(Xq) && aligned16(P), "%s: Xq and P must be 16-byte aligned (Xq %p, P %p)", who, (const void*)Xq, (const void*)P);
    hipLaunchKernelGGL(otam_align_kernel, dim3((unsigned)NP), dim3(WG), 0, static_cast<hipStream_t>(stream), Xq, qn, P, pn, pair_q,
                       pair_slot, NQ, cap, T, E, lambda, single_direct, plan, dists_or_null, logits);
    return check_launch(who);
}
