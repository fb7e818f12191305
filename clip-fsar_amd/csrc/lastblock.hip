// The last ViT block's class-token attention without its K | V projection (libclipfsar_lastblock.so, C ABI and the algebra in
// include/clipfsar_lastblock.h): key fold -> class attend -> value fold.  A library of its own: the other eight keep their pinned export
// sets and kernel counts.
//
// All three kernels run on v_mfma_f32_16x16x32_f16 (lane l holds A[row l & 15][k = 8 (l >> 4) + j], B[k = 8 (l >> 4) + j][col l & 15],
// j < 8, and C[row 4 (l >> 4) + r][col l & 15], r < 4).  The two folds are [16 frames, 64] x [64, D] and [16 frames, D] x [D, 64] per
// head and workgroup, operands straight from global memory.
//
// class_attend_kernel: ONE workgroup of four waves per frame reads the frame's rows from HBM ONCE, in chunks of CHUNK = 32 tokens staged
// in LDS (the next chunk's loads are in flight while a chunk is worked on), with an ONLINE SOFTMAX over the chunks (no second pass over
// the rows).  Per chunk:
//   scores   S[t, h] = x_t . g_h: A = the chunk's rows (ds_read_b128), B = g (heads padded to 16; each wave keeps the fragments of its
//            k steps in registers for the whole frame), the k steps dealt round-robin to the waves, partial sums combined in wave order;
//   softmax  wave 0, lane (h, tq) owns tokens 8 tq .. 8 tq + 7 of head h -- which IS the A fragment of the next product: running maximum m,
//            alpha = exp(m_old - m_new), weights w_t = fp16(exp(s_t - m_new) / sd_t), and the two sums that normalise them EXACTLY as
//            rounded, l = sum w_t sd_t and c = sum w_t mu_t;
//   z        Z[h, k] = alpha Z[h, k] + sum_t w_t x_t[k]: A = w (heads x tokens), B = the chunk's rows with TOKENS as the K dimension,
//            i.e. a transposing LDS read (ds_read_b64_tr_b16) of the row-major image; each wave owns `heads` of the D / 16 column tiles.
// At the end z = (Z - c) / l.  The accumulators are rescaled by alpha in every chunk (alpha = 1 costs the same multiply), so the
// rescale is no rare branch.  LDS rows are 2 D + 32 bytes apart: 16-byte aligned, and 8 banks on from row to row.
#include "side_lib.h"
#include "../../include/clipfsar_lastblock.h"

namespace {

constexpr int CHUNK = CFLB_TOKEN_CHUNK, FB = CFLB_FRAME_BATCH;
static_assert(CHUNK == 32 && FB == 16, "one MFMA K step of tokens, one MFMA tile of frames");
typedef __fp16 tr_f16x4 __attribute__((__vector_size__(4 * sizeof(__fp16))));          // the transposing LDS read's own vector type

// ds_read_b64_tr_b16: lane 4 q + p of each 16-lane group addresses row q, columns 4 p .. 4 p + 3 of a 4 x 16 block of 16-bit elements and
// receives column (lane & 15) of the block's 4 rows.  Every lane of the wave must take part.
__device__ __forceinline__ f16x4 lds_read_tr(const unsigned char* p) {
    return __builtin_bit_cast(f16x4, __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) tr_f16x4*)(p)));
}

__device__ __forceinline__ f32x4 mfma16(f16x8 a, f16x8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }

// sum over the 16 lanes that share l >> 4, result in all of them
__device__ __forceinline__ float row16_sum(float v) {
    v = cfsar_dpp_sum8(v);
    return v + cfsar_dpp_move<0x140>(v);               // row_mirror
}

template <typename TQ>
__global__ __launch_bounds__(256) void key_fold_kernel(const TQ* __restrict__ q, const _Float16* __restrict__ wk_t, _Float16* __restrict__ g,
                                                       float* __restrict__ G, int F, int D, int heads) {
    __shared__ float Gp[4][FB];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, c = lane & 15, kg = lane >> 4;
    const int f0 = blockIdx.x * FB, h = blockIdx.y;
    f16x8 a[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
        for (int e = 0; e < 8; ++e) a[ks][e] = (_Float16)0.f;
        if (f0 + c < F) {
            const TQ* qp = q + (size_t)(f0 + c) * D + h * 64 + ks * 32 + 8 * kg;
#pragma unroll
            for (int e = 0; e < 8; ++e) a[ks][e] = (_Float16)(float)qp[e];
        }
    }
    float gsum[4] = {0.f, 0.f, 0.f, 0.f};
    for (int nt = w; nt < D / 16; nt += 4) {
        const int k = nt * 16 + c;
        const _Float16* wp = wk_t + ((size_t)h * D + k) * 64 + 8 * kg;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        acc = mfma16(a[0], *reinterpret_cast<const f16x8*>(wp), acc);
        acc = mfma16(a[1], *reinterpret_cast<const f16x8*>(wp + 32), acc);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const _Float16 gv = (_Float16)(acc[r] * 0.125f);
            gsum[r] += (float)gv;
            const int fr = f0 + 4 * kg + r;
            if (fr < F) g[((size_t)fr * heads + h) * D + k] = gv;
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float s = row16_sum(gsum[r]);
        if (c == 0) Gp[w][4 * kg + r] = s;
    }
    __syncthreads();
    if (threadIdx.x < FB && f0 + (int)threadIdx.x < F) {
        const int i = threadIdx.x;
        G[(size_t)(f0 + i) * heads + h] = ((Gp[0][i] + Gp[1][i]) + Gp[2][i]) + Gp[3][i];
    }
}

template <typename TO>
__global__ __launch_bounds__(256) void value_fold_kernel(const float* __restrict__ z, const _Float16* __restrict__ wv,
                                                         const float* __restrict__ d_v, TO* __restrict__ oc, int F, int D, int heads) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, c = lane & 15, kg = lane >> 4;
    const int f0 = blockIdx.x * FB, h = blockIdx.y, n = h * 64 + w * 16 + c;
    const bool rowok = f0 + c < F;
    const float* zp = z + ((size_t)(rowok ? f0 + c : f0) * heads + h) * D + 8 * kg;
    const _Float16* wp = wv + (size_t)n * D + 8 * kg;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < D; k += 32) {
        const f32x4 z0 = *reinterpret_cast<const f32x4*>(zp + k), z1 = *reinterpret_cast<const f32x4*>(zp + k + 4);
        f16x8 hi, lo;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float v = rowok ? (e < 4 ? z0[e] : z1[e - 4]) : 0.f;
            hi[e] = (_Float16)v;
            lo[e] = (_Float16)(v - (float)hi[e]);
        }
        const f16x8 b = *reinterpret_cast<const f16x8*>(wp + k);
        acc = mfma16(lo, b, acc);
        acc = mfma16(hi, b, acc);
    }
    const float bias = d_v[n];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int fr = f0 + 4 * kg + r;
        if (fr < F) oc[(size_t)fr * D + n] = (TO)(acc[r] + bias);
    }
}

// NT: an upper bound of heads = the column tiles of a wave in the z product (and twice the k steps of a wave in the score product).
// Up to 12 heads the kernel is held to two waves per SIMD (256 registers, two workgroups per CU); with 16 it takes one.
template <int NT>
__global__ __launch_bounds__(256, NT <= 12 ? 2 : 1) void class_attend_kernel(const _Float16* __restrict__ x, const _Float16* __restrict__ g,
                                                           const float* __restrict__ G, const float* __restrict__ partial, int slots,
                                                           const float* __restrict__ rowstats, float eps, float* __restrict__ z,
                                                           int ntok, int D, int heads) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c = lane & 15, kg = lane >> 4;
    const int f = blockIdx.x, stride = 2 * D + 32;
    unsigned char* xs = smem;                                                    // [CHUNK][stride]: the chunk's rows
    float* Sp = reinterpret_cast<float*>(smem + CHUNK * stride);                 // [4 waves][CHUNK][16]: partial scores
    f16x8* afrag = reinterpret_cast<f16x8*>(Sp + 4 * CHUNK * 16);                // [64]: the weights, as the z product's A fragments
    float* mu_s = reinterpret_cast<float*>(afrag + 64);                          // [CHUNK] each
    float *sd_s = mu_s + CHUNK, *rsd_s = sd_s + CHUNK, *alpha_s = rsd_s + CHUNK; // alpha_s [16], fin_s [32]: c and 1 / l per head
    float* fin_s = alpha_s + 16;
    const size_t row0 = (size_t)f * ntok;

    f16x8 gfrag[(NT + 1) / 2];                                                   // g of head c, k steps w, w + 4, ...
#pragma unroll
    for (int i = 0; i < (NT + 1) / 2; ++i) {
#pragma unroll
        for (int e = 0; e < 8; ++e) gfrag[i][e] = (_Float16)0.f;
        const int ks = w + 4 * i;
        if (ks < 2 * heads && c < heads) gfrag[i] = *reinterpret_cast<const f16x8*>(g + ((size_t)f * heads + c) * D + ks * 32 + 8 * kg);
    }
    const float Gh = c < heads ? G[(size_t)f * heads + c] : 0.f;
    f32x4 acc[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m_run = -INFINITY, l_run = 0.f, c_run = 0.f;                           // wave 0: head c's running maximum and the two sums
    const int pieces = D / 8;

    // Software pipeline: the NEXT chunk's rows and statistics are fetched into registers (v, st) while this chunk is worked on, and stored
    // to LDS behind the chunk's last barrier.  A thread fetches pieces tid, tid + 256, ... of the chunk's CHUNK * D / 8 16-byte pieces
    // (`heads` of them) and, with the 7 other lanes of its row tid >> 3, the row's statistics: as partials, slots 2 q and 2 q + 1 (summed
    // over the 8 lanes as ln_stats_finalize8_kernel does); finalized, lane q = 0 alone.
    uint4 v[NT];
    float4 st;
    const int srow = tid >> 3, sq = tid & 7;
    const float invD = 1.0f / (float)D;
    auto fetch = [&](int t0) {
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            v[i] = make_uint4(0u, 0u, 0u, 0u);                                   // rows behind the frame: zeros
            if (i < heads) {
                const int idx = tid + 256 * i, r = idx / pieces, p = idx - r * pieces;
                if (t0 + r < ntok) v[i] = *reinterpret_cast<const uint4*>(x + (row0 + t0 + r) * D + p * 8);
            }
        }
        st = make_float4(0.f, 0.f, 0.f, 0.f);
        if (t0 + srow < ntok) {
            const size_t m = row0 + t0 + srow;
            if (rowstats) {
                if (sq == 0) st = *reinterpret_cast<const float4*>(rowstats + m * 4);
            } else {
                const float2* pp = reinterpret_cast<const float2*>(partial) + m * slots + 2 * sq;
                if (2 * sq < slots) st.x = pp[0].x, st.y = pp[0].y;
                if (2 * sq + 1 < slots) st.z = pp[1].x, st.w = pp[1].y;
            }
        }
    };
    fetch(0);

    for (int t0 = 0; t0 < ntok; t0 += CHUNK) {
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            if (i < heads) {
                const int idx = tid + 256 * i, r = idx / pieces, p = idx - r * pieces;
                *reinterpret_cast<uint4*>(xs + r * stride + p * 16) = v[i];
            }
        }
        {
            float mean = st.x, sd = st.y, rsd = st.z;
            if (!rowstats) {
                const float s = cfsar_dpp_sum8(st.x + st.z), ss = cfsar_dpp_sum8(st.y + st.w);
                mean = s * invD;
                sd = sqrtf(fmaxf(ss * invD - mean * mean, 0.f) + eps);
                rsd = 1.0f / sd;
            }
            if (t0 + srow >= ntok) mean = 0.f, sd = 1.f, rsd = 0.f;
            if (sq == 0) mu_s[srow] = mean, sd_s[srow] = sd, rsd_s[srow] = rsd;
        }
        __syncthreads();
        if (t0 + CHUNK < ntok) fetch(t0 + CHUNK);
        {                                                                        // scores: both token tiles, this wave's k steps
            f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int i = 0; i < (NT + 1) / 2; ++i) {
                const int ks = w + 4 * i;
                if (ks < 2 * heads) {
                    const unsigned char* ap = xs + c * stride + (ks * 32 + 8 * kg) * 2;
                    s0 = mfma16(*reinterpret_cast<const f16x8*>(ap), gfrag[i], s0);
                    s1 = mfma16(*reinterpret_cast<const f16x8*>(ap + 16 * stride), gfrag[i], s1);
                }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                Sp[(w * CHUNK + 4 * kg + r) * 16 + c] = s0[r];
                Sp[(w * CHUNK + 16 + 4 * kg + r) * 16 + c] = s1[r];
            }
        }
        __syncthreads();
        if (w == 0) {                                                            // softmax step of head c, tokens 8 kg .. 8 kg + 7
            float s[8], cm = -INFINITY;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int t = 8 * kg + j;
                const float S = ((Sp[t * 16 + c] + Sp[(CHUNK + t) * 16 + c]) + Sp[(2 * CHUNK + t) * 16 + c]) + Sp[(3 * CHUNK + t) * 16 + c];
                s[j] = t0 + t < ntok ? (S - mu_s[t] * Gh) * rsd_s[t] : -INFINITY;
                cm = fmaxf(cm, s[j]);
            }
            cm = fmaxf(cm, __shfl_xor(cm, 16, 64));
            cm = fmaxf(cm, __shfl_xor(cm, 32, 64));
            const float m_new = fmaxf(m_run, cm);                                // finite: token t0 belongs to the frame
            const float alpha = expf(m_run - m_new);
            float ls = 0.f, cs = 0.f;
            f16x8 wv;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int t = 8 * kg + j;
                wv[j] = (_Float16)(expf(s[j] - m_new) * rsd_s[t]);               // exp(-inf) = 0 behind the frame
                const float wf = (float)wv[j];
                ls = fmaf(wf, sd_s[t], ls);
                cs = fmaf(wf, mu_s[t], cs);
            }
            ls += __shfl_xor(ls, 16, 64);
            ls += __shfl_xor(ls, 32, 64);
            cs += __shfl_xor(cs, 16, 64);
            cs += __shfl_xor(cs, 32, 64);
            l_run = fmaf(l_run, alpha, ls);
            c_run = fmaf(c_run, alpha, cs);
            m_run = m_new;
            afrag[lane] = wv;
            if (kg == 0) alpha_s[c] = alpha;
        }
        __syncthreads();
        {                                                                        // Z = alpha Z + w^T x over this wave's column tiles
            const f16x8 a = afrag[lane];
            float al[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) al[r] = alpha_s[4 * kg + r];
            // two transposed blocks = tokens 8 kg .. 8 kg + 7 of column tile i * 4 + w
            const unsigned char* bp = xs + (8 * kg + (c >> 2)) * stride + (4 * (c & 3)) * 2;
#pragma unroll
            for (int i = 0; i < NT; ++i) {
                if (i < heads) {                                                 // uniform: every lane takes part in the read
                    const unsigned char* p = bp + (i * 4 + w) * 32;
                    const f16x4 b0 = lds_read_tr(p), b1 = lds_read_tr(p + 4 * stride);
                    const f16x8 b = {b0[0], b0[1], b0[2], b0[3], b1[0], b1[1], b1[2], b1[3]};
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[i][r] *= al[r];
                    acc[i] = mfma16(a, b, acc[i]);
                }
            }
        }
        __syncthreads();
    }
    if (w == 0 && kg == 0) fin_s[c] = c_run, fin_s[16 + c] = 1.0f / l_run;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        if (i < heads) {
            const int col = (i * 4 + w) * 16 + c;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int h = 4 * kg + r;
                if (h < heads) z[((size_t)f * heads + h) * D + col] = (acc[i][r] - fin_s[h]) * fin_s[16 + h];
            }
        }
    }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

int check_dims(const char* who, int F, int D, int heads) {
    SIDE_REQUIRE(heads >= 1 && heads <= CFLB_MAX_HEADS && D == 64 * heads && F >= 1,
                 "%s: bad shape (F=%d D=%d heads=%d; F >= 1, 1 <= heads <= %d, D == 64 * heads)", who, F, D, heads, CFLB_MAX_HEADS);
    return 0;
}

int attend_lds_bytes(int D) { return CHUNK * (2 * D + 32) + 4 * CHUNK * 16 * 4 + 64 * 16 + (3 * CHUNK + 16 + 32) * 4; }

template <int NT>
int launch_attend(const char* who, const void* x, const void* g, const float* G, const float* partial, int slots, const float* rowstats,
                  float eps, float* z, int F, int ntok, int D, int heads, hipStream_t s) {
    const int lds = attend_lds_bytes(D);
    if (lds > 48 * 1024) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(class_attend_kernel<NT>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (e != hipSuccess) return fail("%s: %d bytes of LDS: %s", who, lds, hipGetErrorString(e));
    }
    hipLaunchKernelGGL(class_attend_kernel<NT>, dim3((unsigned)F), dim3(256), lds, s, static_cast<const _Float16*>(x),
                       static_cast<const _Float16*>(g), G, partial, slots, rowstats, eps, z, ntok, D, heads);
    return check_launch(who);
}

}  // namespace

extern "C" int cflb_version(void) { return 100; /* 0.1.0 */ }
extern "C" int cflb_abi_version(void) { return CFLB_ABI_VERSION; }
extern "C" const char* cflb_last_error(void) { return g_err; }

extern "C" int cflb_key_fold(const void* q, int dtype, const void* wk_t, void* g, float* G, int F, int D, int heads, cflb_stream_t stream) {
    const char* who = "cflb_key_fold";
    SIDE_REQUIRE(q && wk_t && g && G, "%s: null pointer", who);
    if (check_dims(who, F, D, heads)) return 1;
    SIDE_REQUIRE(dtype == CFLB_BF16 || dtype == CFLB_F16, "%s: bad dtype %d", who, dtype);
    SIDE_REQUIRE(aligned16(q) && aligned16(wk_t) && aligned16(g), "%s: q, wk_t and g must be 16-byte aligned", who);
    const dim3 grid((unsigned)((F + FB - 1) / FB), (unsigned)heads);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (dtype == CFLB_BF16)
        hipLaunchKernelGGL(key_fold_kernel<__bf16>, grid, dim3(256), 0, s, static_cast<const __bf16*>(q), static_cast<const _Float16*>(wk_t),
                           static_cast<_Float16*>(g), G, F, D, heads);
    else
        hipLaunchKernelGGL(key_fold_kernel<_Float16>, grid, dim3(256), 0, s, static_cast<const _Float16*>(q),
                           static_cast<const _Float16*>(wk_t), static_cast<_Float16*>(g), G, F, D, heads);
    return check_launch(who);
}

extern "C" int cflb_class_attend(const void* x, const void* g, const float* G, const float* partial, int slots, const float* rowstats,
                                 float eps, float* z, int F, int ntok, int D, int heads, cflb_stream_t stream) {
    const char* who = "cflb_class_attend";
    SIDE_REQUIRE(x && g && G && z, "%s: null pointer", who);
    if (check_dims(who, F, D, heads)) return 1;
    SIDE_REQUIRE(ntok >= 1 && (long long)F * ntok <= 0x7fffffffLL, "%s: bad shape (ntok=%d F=%d; ntok >= 1, F * ntok below 2^31)", who, ntok, F);
    SIDE_REQUIRE((partial != nullptr) != (rowstats != nullptr), "%s: exactly one of partial and rowstats is needed", who);
    SIDE_REQUIRE(partial ? (slots >= 1 && slots <= 16) : slots == 0, "%s: slots=%d (1 .. 16 with partial, 0 with rowstats)", who, slots);
    SIDE_REQUIRE(eps > 0.f, "%s: eps must be > 0", who);
    SIDE_REQUIRE(aligned16(x) && aligned16(g) && aligned16(z) && aligned16(partial) && aligned16(rowstats),
                 "%s: x, g, z and the statistics must be 16-byte aligned", who);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (heads <= 2) return launch_attend<2>(who, x, g, G, partial, slots, rowstats, eps, z, F, ntok, D, heads, s);
    if (heads <= 12) return launch_attend<12>(who, x, g, G, partial, slots, rowstats, eps, z, F, ntok, D, heads, s);
    return launch_attend<16>(who, x, g, G, partial, slots, rowstats, eps, z, F, ntok, D, heads, s);
}

extern "C" int cflb_value_fold(const float* z, const void* wv, const float* d_v, void* oc, int dtype, int F, int D, int heads,
                               cflb_stream_t stream) {
    const char* who = "cflb_value_fold";
    SIDE_REQUIRE(z && wv && d_v && oc, "%s: null pointer", who);
    if (check_dims(who, F, D, heads)) return 1;
    SIDE_REQUIRE(dtype == CFLB_BF16 || dtype == CFLB_F16, "%s: bad dtype %d", who, dtype);
    SIDE_REQUIRE(aligned16(z) && aligned16(wv), "%s: z and wv must be 16-byte aligned", who);
    const dim3 grid((unsigned)((F + FB - 1) / FB), (unsigned)heads);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (dtype == CFLB_BF16)
        hipLaunchKernelGGL(value_fold_kernel<__bf16>, grid, dim3(256), 0, s, z, static_cast<const _Float16*>(wv), d_v,
                           static_cast<__bf16*>(oc), F, D, heads);
    else
        hipLaunchKernelGGL(value_fold_kernel<_Float16>, grid, dim3(256), 0, s, z, static_cast<const _Float16*>(wv), d_v,
                           static_cast<_Float16*>(oc), F, D, heads);
    return check_launch(who);
}
