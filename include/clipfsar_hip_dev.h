/*
 * clipfsar_hip_dev.h -- DEVELOPER hooks of libclipfsar_hip.so.  NOT part of the product ABI.
 *
 * These symbols exist only in a library built with `CFSAR_DEV=1 python clip-fsar_amd/build.py` (-DCFSAR_DEV).  The default
 * (product) build contains neither the hooks nor the ablation branches they switch: `nm -D libclipfsar_hip.so` shows the entry
 * points of clipfsar_hip.h only (tests/test_abi.py).  Users: tools/gemm_ab.py and friends (in-process, interleaved A/B of
 * kernel variants on the GPU box).
 */
#ifndef CLIPFSAR_HIP_DEV_H
#define CLIPFSAR_HIP_DEV_H
#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

/* Force the kernel cfsar_gemm / cfsar_gemm_ex dispatch to (variant) and set the ablation bits (dbg) of the next launches;
 * (0, 0) restores the product policy.  Every variant is a kernel the product library also runs (csrc/gemm.hip, dispatch comment):
 *   1 = v1 (128 x 128, also the fp32 path), 2 = p3 (256 x 128), 12 / 13 = p12 / p12 persistent,
 *   14 / 15 = skinny fp32 kernel always / never, 20 / 28 = the persistent ViT kernel (csrc/gemm_vit.hip) on any shape with the
 *   register-staged / the early-DMA operand path. */
void cfsar_debug_set_gemm_variant(int variant, int dbg);

/* Operand path of the persistent ViT kernel's launches (0 register-staged, 2 early LDS-DMA; 10 + path: K <= 1024 only);
 * -1 = the product policy.  The store policy stays the product's. */
void cfsar_debug_set_vit_paths(int opath);
/* ablation bits of the ViT GEMM launches (csrc/gemm_vit.hip: 4 no epilogue, 8 every workgroup reads tile (0, 0), 16 no global
 * stores, 128 start-time stagger, 1 << 17 / 1 << 18 192- / 256-row tiles, 1 << 21 / 1 << 22 forced paths skip the LN-folded / the
 * residual launches; a few more load-policy / priority A/B bits are commented at their use) */
void cfsar_debug_set_vit_dbg(int dbg);
/* per-tile time stamps of the persistent ViT GEMM (device buffer [grid][64][4] of int64: s_memrealtime at tile start, K-loop end,
 * epilogue end; NULL = off) and the unit (x 64 cycles) of the start-time stagger that dbg bit 128 switches on */
void cfsar_debug_set_vit_trace(void* trace, int stagger_unit);
/* workgroup shape of the bf16 attention kernel at 197 tokens (csrc/attention.hip); 0 = product */
void cfsar_debug_set_attn_variant(int v);
/* bit 0 clear: cfsar_conv3x3_nhwc routes Cin, Cout in {32, 64} through the implicit GEMM again instead of the direct kernel
 * (csrc/conv.hip); bits 8+: ablation bits of the direct kernel (1 no stores, 2 first tile's tap addresses, 4 no MFMAs, 8 no barrier) */
void cfsar_debug_set_direct_conv(int on);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* CLIPFSAR_HIP_DEV_H */
