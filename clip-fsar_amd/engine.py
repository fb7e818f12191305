"""Host-side orchestration of the HIP kernels: the CLIP ViT image tower (A1-A8) and the few-shot tail (A9-A15).

PyTorch is used only for device memory and the stream; every arithmetic step is a call into
libclipfsar_hip.so (clip_fsar_amd.hip).  Numerics modes (DESIGN.md (c) has what each guarantees, measured):

  * ``precision="bf16"``  -- throughput mode: bf16 MFMA GEMMs / attention with fp32 accumulation, residual
    stream in IEEE fp16 (as CLIP's own GPU path), fp32 LayerNorm / softmax statistics, the two LayerNorms of a block folded
    into the QKV / c_fc GEMMs (fp16 MFMA operands there, bf16 elsewhere); the tail (features -> logits) is always fp32;
  * ``precision="fp16"``  -- the fast 16-bit mode: fp16 operands everywhere, residual add in fp32 with a two-word fp16 stream, the weights' second fp16
    word applied to the per-frame token mean of each GEMM's operand; inside 1e-3 as a statistic;
  * ``precision="fp16_strict"`` (round 6, ViT towers) -- the fp16 mode + an exact patch-embedding front end + split QKV weights: every logit row of every
    reference golden inside 1e-3 (a bound on everything measured);
  * ``precision="fp32"``  -- validation mode: fp32-input MFMA GEMMs (exact fp32 FMA chains) and an fp32 VALU
    attention kernel; meets the 1e-3 logits tolerance against the reference's fp32 PyTorch path on any input.

Layout in HBM (row-major): tokens x [F*N, D] (fp32 in the validation mode, fp16 in the bf16 mode; frame-major, token-minor;
token 0 = class token),
packed qkv [F*N, 3D], MLP hidden [F*N, 4D] in the compute dtype; features [B, S+Q, T, E] fp32.
"""
from __future__ import annotations

import math

import os

import torch

from . import hip


# fp16 numerics mode (HipViT.__init__, profiles/r04_parity_table.md): the GEMMs whose weights' second fp16 word is applied to the per-frame
# token mean of the operand (MCORR: one pass over the operand + a 1 / tokens-size GEMM) or to the whole operand (SPLIT: a second MFMA pass).
# 16 fresh episodes per configuration against the fp32 mode, rms / max |dlogits| on cfg2, cfg3, cfg4:  mcorr all 2.4e-4 / 2.2e-4 / 2.5e-4 and
# 6.1e-4 / 6.7e-4 / 6.7e-4 at 276-288 episodes/s (64 episodes, final build: 2.7 / 2.1 / 2.3 and 11.4 / 7.3 / 10.2 at 284-298);  split qkv,out,pr 2.5 / 2.1 / 2.9 and 8.2 / 6.3 / 8.2 at 217;  split all 2.2 / 1.7 / 1.9 and
# 6.7 / 5.5 / 5.3 at 194;  neither 3.3 / 2.8 / 5.0 and 9.0 / 9.3 / 16.0 at 308.
FP16_SPLIT_DEFAULT = ""
FP16_MCORR_DEFAULT = "qkv,out,fc,pr"
# fp16_strict (round 6; profiles/r06_strict_eval.md): the QKV GEMM carries split weights, the other three keep the per-frame correction.  On high-contrast
# ViT-L/14 episodes and on outlier-channel weights a frame's tokens differ a lot from their mean, and what the correction leaves of the LN-folded QKV weights'
# rounding -- it reaches the logits through q k^T, twice -- is then the largest term: 13 reference episodes of hc_cfg4, max |dlogits| 1.06e-3 with the correction,
# 7.4e-4 with split QKV weights (split c_fc instead: 9.3e-4; both: 5.8e-4 at 0.57 x the bf16 rate).
FP16_STRICT_SPLIT_DEFAULT = "qkv"
FP16_STRICT_MCORR_DEFAULT = "out,fc,pr"
# Towers deeper than 12 blocks (ViT-L/14: 24) also split c_fc: 64 fresh HIGH-CONTRAST cfg4 episodes (logits spread 5.4), max |dlogits| 1.05e-3 / 2 episodes over
# 1e-3 with split QKV alone, 8.3e-4 / none with c_fc split as well (0.64 x instead of 0.75 x the tower's bf16 rate; profiles/r06_strict_eval.md).
FP16_STRICT_DEEP_LAYERS = 12
FP16_STRICT_SPLIT_DEEP_DEFAULT = "qkv,fc"
FP16_STRICT_MCORR_DEEP_DEFAULT = "out,pr"


def _round_up(x, m):
    return (x + m - 1) // m * m


class HipViT:
    """CLIP VisionTransformer.forward (reference few_shot.py:671-688) on the HIP kernels."""

    # developer options (tools/*.py; every default is the product setting and has a GPU test): ablations of the fp16 numerics mode and the
    # statistics fusion.  They are constructor arguments -- the product path reads four environment variables only (CFSAR_LN_FOLD,
    # CFSAR_FULL_LAST_BLOCK, CFSAR_FP16_SPLIT, CFSAR_FP16_MCORR).
    OPTIONS = {"fp16_wide": True, "fp16_lo": True, "fp16_rawmeans": True, "fused_umeans": True, "fused_omeans": True, "fuse_stats": True,
               "fused_patch": True, "strict_front": True, "strict_o_pair": False, "fold_last_kv": True}

    def __init__(self, arch: dict, sd: dict, prefix: str = "", precision: str = "bf16", device="cuda", stream_dtype=None, fp16_split=None, fp16_mcorr=None,
                 options=None):
        # "fp16_strict" (round 6): the fp16 mode with the cheap error sources of profiles/r06_strict_budget.md removed -- see self.strict below
        self.strict = precision == "fp16_strict"
        if self.strict:
            precision = "fp16"
        if precision not in ("bf16", "fp16", "fp32"):
            raise ValueError("precision must be 'bf16', 'fp16', 'fp16_strict' or 'fp32'")
        opt = dict(self.OPTIONS)
        for k, v in (options or {}).items():
            if k not in opt:
                raise ValueError("HipViT: unknown option %r (known: %s)" % (k, ", ".join(sorted(opt))))
            opt[k] = bool(v)
        self.arch = dict(arch)
        self.precision = precision
        self.dev = torch.device(device)
        # compute dtype of the 16-bit modes: bf16 = throughput mode; fp16 = the same kernels on IEEE half operands everywhere (weights,
        # patches, q / k / v, attention probabilities and output, MLP hidden): 3 more mantissa bits for ~3-6 % of the throughput (the
        # fp16 multipliers toggle more bits: the chip runs these kernels power-limited) -- the 16-bit mode that meets the 1e-3 logits
        # tolerance (profiles/r04_parity_table.md).  Range: |x| < 65 504; checked for the weights below, the LN-fold guard covers the
        # folded vectors, activations of CLIP-scale weights are O(1) ... O(100).
        self.cd = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}[precision]
        # residual stream: fp32 in the validation mode.  The bf16 mode keeps it in IEEE fp16, as CLIP's own GPU path does
        # (fp16 model, few_shot.py:605-611 casts LayerNorm to fp32 and back): out_proj / c_proj / LayerNorm are bound by the
        # stream's bytes, and on top of bf16 operands the fp16 rounding is not measurable (feature rms error 0.0064 with an
        # fp16 stream vs 0.0067 with an fp32 one, against 0.0092 for a bf16 stream; docs/history/design_r01-r03.md "Numerics modes").
        if stream_dtype is None:
            stream_dtype = "fp32" if precision == "fp32" else "fp16"
        if stream_dtype not in ("fp16", "fp32") or (precision == "fp32" and stream_dtype != "fp32") or (precision == "fp16" and stream_dtype != "fp16"):
            raise ValueError("stream_dtype must be 'fp32' (bf16 / fp32 precision) or 'fp16' (bf16 / fp16 precision)")
        self.xd = torch.float16 if stream_dtype == "fp16" else torch.float32
        D, P = arch["width"], arch["patch"]
        if D != arch["heads"] * 64:
            raise ValueError("HipViT needs head_dim == 64 (width %d, heads %d)" % (D, arch["heads"]))
        self.D, self.P, self.L, self.H, self.E = D, P, arch["layers"], arch["heads"], arch["embed"]
        self.grid = arch["res"] // P
        self.ntok = self.grid * self.grid + 1
        kq = 32 if precision == "fp32" else 64
        self.kpad = _round_up(3 * P * P, kq)

        def g(name):
            t = sd[prefix + name]
            if not isinstance(t, torch.Tensor):
                t = torch.from_numpy(t)
            return t.detach().to(device=self.dev, dtype=torch.float32).contiguous()

        cd = self.cd
        wc = torch.zeros(D, self.kpad, device=self.dev, dtype=torch.float32)
        wc[:, :3 * P * P] = g("conv1.weight").reshape(D, -1)
        self.w_patch = wc.to(cd).contiguous()
        # patch gather inside the patch-embed GEMM (16 x 16 and 14 x 14 patches, 16-bit operands, 16-bit stream); "fused_patch": False keeps
        # the three-launch form (the A/B and bit-equality tests)
        self.fused_patch = bool(opt["fused_patch"] and P in hip.PATCH_EMBED_SLOTS and cd in (torch.bfloat16, torch.float16)
                                and self.xd == torch.float16)
        if self.fused_patch:             # 14 x 14 patches (ViT-L/14, round 6): the kernel's padded-row column layout, [D, 704]
            self.w_patch_fused = self.w_patch if P == 16 else hip.patch_embed_weight(g("conv1.weight"), P, cd)
        self.cls = g("class_embedding")
        self.pos = g("positional_embedding")
        self.ln_pre = (g("ln_pre.weight"), g("ln_pre.bias"))
        self.ln_post = (g("ln_post.weight"), g("ln_post.bias"))
        self.w_proj_t = g("proj").t().contiguous()          # [E, D] fp32: final projection always in fp32
        self.blocks = []
        for i in range(self.L):
            b = "transformer.resblocks.%d." % i
            self.blocks.append(dict(
                ln1=(g(b + "ln_1.weight"), g(b + "ln_1.bias")),
                ln2=(g(b + "ln_2.weight"), g(b + "ln_2.bias")),
                w_qkv=g(b + "attn.in_proj_weight").to(cd).contiguous(), b_qkv=g(b + "attn.in_proj_bias"),
                w_out=g(b + "attn.out_proj.weight").to(cd).contiguous(), b_out=g(b + "attn.out_proj.bias"),
                w_fc=g(b + "mlp.c_fc.weight").to(cd).contiguous(), b_fc=g(b + "mlp.c_fc.bias"),
                w_pr=g(b + "mlp.c_proj.weight").to(cd).contiguous(), b_pr=g(b + "mlp.c_proj.bias")))
        # LayerNorm folding (bf16 mode with the fp16 stream): ln_1 / ln_2 never run as kernels.  QKV and c_fc take the raw fp16
        # residual stream and apply LN algebraically (include/clipfsar_hip.h: cfsar_gemm_lnfold):
        #     LN(x) W^T + b = (x (W diag(gamma))^T - mean c) / std + d,    c_n = sum_k Wg[n,k],   d = W beta + b;
        # out_proj / c_proj emit the row statistics of the stream they write (cfsar_gemm_residual_stats).  Weight folding is
        # init-time host logic (like the BatchNorm folding of the RN50 tower).  CFSAR_LN_FOLD=0 keeps the separate LN kernels.
        self.fold = (precision in ("bf16", "fp16") and self.xd == torch.float16 and D % 64 == 0 and D >= 128
                     and (precision == "fp16" or os.environ.get("CFSAR_LN_FOLD", "1") != "0"))
        if precision == "fp16":
            if not self.fold:
                raise ValueError("precision 'fp16' needs the LayerNorm-folded block (width a multiple of 64, >= 128)")
            wmax16 = max(float(blk[k].float().abs().max()) for blk in self.blocks for k in ("w_out", "w_pr"))
            wmax16 = max(wmax16, float(self.w_patch.float().abs().max()))
            if not wmax16 < 6.0e4:
                raise ValueError("precision 'fp16': a weight exceeds the fp16 range (max |w| = %.3g); use 'bf16' or 'fp32'" % wmax16)
        # fp16 numerics mode, round 4 (profiles/r04_parity_table.md; tools/numerics_lab.py is the CPU model that chose these):
        #   wide   -- out_proj / c_proj add their result to the stream in fp32 and round ONCE (cfsar_gemm_residual_wide; round 3 rounded
        #             the GEMM result to fp16 and added in fp16);
        #   two_word -- the stream is x_hi + x_lo (two fp16 words, ~22 bits): residual adds read and write both, the LN-folded GEMMs
        #             read x_hi and its statistics;
        #   split  -- which GEMMs carry their weights as fp16 hi + lo pairs [N, 2K] (the rounding of the WEIGHTS is the error that
        #             does not average out over tokens and frames): twice the MFMA work of each GEMM named.
        # options fp16_wide / fp16_lo and CFSAR_FP16_SPLIT override the defaults (ablation: tools/fp16_variants.py).
        self.wide = precision == "fp16" and opt["fp16_wide"]
        self.two_word = self.wide and opt["fp16_lo"]
        sp_default, mc_default = FP16_SPLIT_DEFAULT, FP16_MCORR_DEFAULT
        if self.strict:
            deep = self.L > FP16_STRICT_DEEP_LAYERS
            sp_default = FP16_STRICT_SPLIT_DEEP_DEFAULT if deep else FP16_STRICT_SPLIT_DEFAULT
            mc_default = FP16_STRICT_MCORR_DEEP_DEFAULT if deep else FP16_STRICT_MCORR_DEFAULT
        sp = os.environ.get("CFSAR_FP16_SPLIT", sp_default if fp16_split is None else fp16_split) if precision == "fp16" else ""
        self.split = set(t for t in sp.split(",") if t)
        #   mcorr  -- which GEMMs get the PER-FRAME LOW-WORD CORRECTION instead: the second weight word multiplies only the per-frame
        #             token mean of the GEMM's operand ([F, K] x W_lo^T, a 1 / tokens-size GEMM) and the [F, N] result is added to every row
        #             of its frame inside the main GEMM's tail MFMA.  It removes the part of the weight-rounding error that is common to a
        #             frame's tokens -- most of what the split buys (tools/numerics_lab.py, scheme "m") -- for one pass over the operand
        #             instead of a second MFMA pass.  Needs >= 128 tokens per frame (tiny test towers fall back to the split); the
        #             last block's class-token rows (one row per frame) use the split form.
        mc = os.environ.get("CFSAR_FP16_MCORR", mc_default if fp16_mcorr is None else fp16_mcorr) if precision == "fp16" else ""
        self.mcorr = set(t for t in mc.split(",") if t)
        if not (self.split | self.mcorr) <= {"qkv", "out", "fc", "pr"}:
            raise ValueError("CFSAR_FP16_SPLIT / CFSAR_FP16_MCORR: names out of qkv,out,fc,pr expected, got %r / %r" % (sp, mc))
        self.mcorr -= self.split                                  # a split GEMM needs no correction
        if self.mcorr and self.ntok < 128:
            self.split |= self.mcorr                              # frames too short for the kernel's two-frames-per-tile form: the exact form
            self.mcorr = set()
        if not self.wide and precision == "fp16" and (self.mcorr or self.split & {"out", "pr"}):
            # option fp16_wide = False is round 3's packed-fp16 residual add, kept as an ablation of the ONE-word mode: it has neither the
            # correction's k slot nor split residual weights (say so instead of silently promoting the correction to the split)
            import warnings
            warnings.warn("HipViT: option fp16_wide=False drops the per-frame correction / split residual weights (%s / %s)" % (
                ",".join(sorted(self.mcorr)) or "-", ",".join(sorted(self.split & {"out", "pr"})) or "-"))
            self.mcorr = set()
            self.split -= {"out", "pr"}

        def hilo(W32):
            """fp32 [N, K] -> fp16 [N, 2K] = [hi | lo]"""
            hi = W32.to(torch.float16)
            lo = (W32 - hi.float()).to(torch.float16)
            return torch.cat([hi, lo], 1).contiguous()

        def lo_word(W32):
            """fp32 [N, K] -> bf16 [N, K]: the remainder of the fp16 rounding (bf16: fp32's exponent range, 8 bits are plenty for a term
            2^-12 of the product)"""
            return (W32 - W32.to(torch.float16).float()).to(torch.bfloat16).contiguous()

        last = len(self.blocks) - 1
        for i, blk in enumerate(self.blocks if (self.split or self.mcorr) else []):
            b = "transformer.resblocks.%d." % i
            for key, name in (("out", "attn.out_proj.weight"), ("pr", "mlp.c_proj.weight")):
                if key in self.split:
                    blk["w_" + key] = hilo(g(b + name))
                elif key in self.mcorr:
                    blk["wlo_" + key] = lo_word(g(b + name))
                    if i == last:
                        blk["ws_" + key] = hilo(g(b + name))      # class-token rows of the last block: split form
        if self.fold:
            for i, blk in enumerate(self.blocks):
                b = "transformer.resblocks.%d." % i
                for tag, wname, bname, ln in (("qkv", "attn.in_proj_weight", "attn.in_proj_bias", "ln1"),
                                              ("fc", "mlp.c_fc.weight", "mlp.c_fc.bias", "ln2")):
                    W = g(b + wname)
                    gamma, beta = blk[ln]
                    if tag in self.split:
                        Wg = hilo(W * gamma[None, :])
                    else:
                        Wg = (W * gamma[None, :]).to(torch.float16).contiguous()
                    if tag in self.mcorr:
                        blk["wlo_" + tag] = lo_word(W * gamma[None, :])
                        if i == len(self.blocks) - 1:                                   # class-token rows of the last block: split form
                            Ws = hilo(W * gamma[None, :]) if tag == "fc" else hilo((W * gamma[None, :])[:D])
                            blk["wgs_" + tag] = Ws
                            blk["cs_" + tag] = Ws.double().sum(1).float().contiguous()
                    blk["wg_" + tag] = Wg
                    blk["c_" + tag] = Wg.double().sum(1).float().contiguous()          # of the ROUNDED folded weights (hi + lo when split)
                    blk["cx_" + tag] = (W * gamma[None, :]).double().sum(1).float().contiguous()   # of the exact ones (raw-stream correction)
                    blk["d_" + tag] = (W.double() @ beta.double() + g(b + bname).double()).float().contiguous()
            # the kernel feeds c, d, mean and std to the matrix pipe as fp16 hi + lo pairs and the folded weights as fp16: a checkpoint
            # whose folded quantities leave the fp16 range cannot use the folded block (CLIP's are O(1) ... O(10))
            big = max(float(max(blk[k].abs().max() for k in ("c_qkv", "d_qkv", "c_fc", "d_fc"))) for blk in self.blocks)
            wmax = max(float(max(blk[k].float().abs().max() for k in ("wg_qkv", "wg_fc"))) for blk in self.blocks)
            if not (big < 3.0e4 and wmax < 6.0e4):
                import warnings
                if precision == "fp16":
                    raise ValueError("precision 'fp16': folded weights / vectors exceed the fp16 range (max |c|,|d| = %.3g, "
                                     "max |W gamma| = %.3g); use 'bf16' or 'fp32'" % (big, wmax))
                warnings.warn("LayerNorm folding disabled: folded weights / vectors exceed the fp16 range (max |c|,|d| = %.3g, "
                              "max |W gamma| = %.3g); using the unfolded block" % (big, wmax))
                self.fold = False
            if self.fold:
                for blk in self.blocks:          # the unfolded 16-bit copies would only serve the fallback above: free ~1/3 of the tower's weights
                    blk["w_qkv"] = blk["w_fc"] = None
        # Last block, class token only.  VisionTransformer.forward reads x[:, 0] after the last block and nothing else of it
        # (few_shot.py:683), so in THAT block the attention output, out_proj and the MLP are needed for row 0 of every frame alone
        # (K and V still come from all tokens): -6.3 % of the tower's FLOPs (ViT-B/16, 12 layers), same class-token arithmetic.
        # CFSAR_FULL_LAST_BLOCK=1 computes the whole block like the reference's PyTorch code does (taps always do).
        self.prune_last = os.environ.get("CFSAR_FULL_LAST_BLOCK", "0") != "1"
        # Option fold_last_kv (bf16 mode, folded path): the pruned last block computes no K | V rows either.  Its one query per frame uses them
        # through two linear functionals per head, and both apply to the raw stream: g = Wk'^T q / 8, softmax of (x_t . g - mu_t G) / sd_t,
        # z = sum_t p_t (x_t - mu_t) / sd_t, o = Wv' z + d_v (include/clipfsar_lastblock.h; DESIGN.md "Last block").  Three launches of
        # libclipfsar_lastblock.so (loaded on the first forward that needs it) replace the K | V GEMM over all tokens and cfsar_vit_attention_cls.
        self.fold_last_kv = bool(opt["fold_last_kv"] and precision == "bf16" and self.fold and self.H <= 16)
        if self.fold_last_kv:
            blk = self.blocks[-1]
            blk["wk_t"] = blk["wg_qkv"][D:2 * D].view(self.H, 64, D).transpose(1, 2).contiguous()    # [heads, D, 64]: layout only
        # LN statistics finalized inside the consuming GEMM (ViT-B / ViT-L widths; CFSAR_FUSE_STATS=0: the separate finalize launches)
        self.fuse_stats = bool(self.fold) and hip.lnfold_partials_ok(self.D, self.D // 64) and opt["fuse_stats"]
        self.fused_umeans = opt["fused_umeans"]      # c_fc emits the hidden's per-frame means (A/B switch)
        self.fused_omeans = opt["fused_omeans"]      # the attention kernel emits its output's per-frame means
        # The LN-folded GEMMs' correction in its RAW-STREAM form: corr = xbar W_lo^T with xbar the per-frame token mean of the raw stream (the row
        # mean's share rides in cvec = the exact column sums of W gamma).  xbar needs no pass over x: the stream's update x += A W^T + b is linear
        # in the frame's token mean, so xbar += mean_t(A) W^T + b from the operand means the residual GEMMs' own corrections already have.
        # (needs the residual GEMMs' operand means -- "out" and "pr" corrected -- for the updates; an LN-folded GEMM that is SPLIT instead of corrected simply
        # takes no correction, and its cvec = the exact column sums serves the split weights as well: they differ from the hi + lo sums by 2^-22)
        self.rawmeans = (opt["fp16_rawmeans"] and self.fused_umeans and self.fused_omeans
                         and all(k in self.mcorr for k in ("out", "pr")) and all(k in self.mcorr | self.split for k in ("qkv", "fc"))
                         and bool(self.mcorr & {"qkv", "fc"}))
        if self.rawmeans:
            for i, blk in enumerate(self.blocks):
                bb = "transformer.resblocks.%d." % i
                blk["wb_out"] = g(bb + "attn.out_proj.weight").to(torch.bfloat16).contiguous()
                blk["wb_pr"] = g(bb + "mlp.c_proj.weight").to(torch.bfloat16).contiguous()
        if self.mcorr & {"qkv", "fc"}:
            self.fuse_stats = False          # the token means of LayerNorm(x) need the finalized statistics in front of the GEMM
        # fp16_strict (budget: tools/numerics_lab.py feats, profiles/r06_strict_budget.md).  Of the fp16 mode's feature-error variance
        # a third enters BEFORE the first block: the patch embedding's 11-bit pixels and weights (0.7 % of the tower's FLOPs) and the two one-word
        # stores of the stream in front of the blocks.  Strict: the patch-embed GEMM runs three fp16 passes [hi | lo | hi] x [W_hi | W_hi | W_lo]
        # into an fp32 token matrix, and class token + pos + ln_pre write the two-word stream directly (cfsar_embed_finish_pair).
        self.strict_front = self.o_pair = False
        if self.strict:
            if not (self.two_word and self.fold and D % 4 == 0 and D <= 1024):
                raise ValueError("precision 'fp16_strict' needs the two-word stream (options fp16_wide / fp16_lo) and a width <= 1024")
            self.strict_front = bool(opt["strict_front"])                             # (developer ablation of the two strict devices)
            if self.strict_front:
                self.fused_patch = False
                w32 = wc
                w_hi = w32.to(torch.float16)
                w_lo = (w32 - w_hi.float()).to(torch.float16)
                self.w_patch3 = torch.cat([w_hi, w_hi, w_lo], 1).contiguous()      # [D, 3 kpad]
            # Option strict_o_pair (built, measured, OFF): the attention output in two fp16 words and out_proj = [o_hi | o_lo] x [W_hi | W_hi | W_lo] (three
            # passes of the smallest block GEMM).  The CPU budget gave it a tenth (ViT-B/16) to a fifth (ViT-L/14) of what the front end leaves; measured it
            # moves the six reference sets by -4 ... +7 % in rms (hc_cfg4 3.64e-4 -> 3.61e-4) and fresh cfg4 episodes by -14 %, for 11 % of the step
            # (303.7 -> 270.8 episodes/s): profiles/r06_strict_eval.md.  Needs the attention kernel's means form.
            self.o_pair = bool(opt["strict_o_pair"]) and self.fused_omeans and "out" in self.mcorr and D % 128 == 0
            if self.o_pair:
                for i, blk in enumerate(self.blocks):
                    W = g("transformer.resblocks.%d.attn.out_proj.weight" % i)
                    Wh = W.to(torch.float16)
                    blk["w3_out"] = torch.cat([Wh, Wh, (W - Wh.float()).to(torch.float16)], 1).contiguous()
        self._slots = {}
        self.max_frames_32bit = (2 ** 32 - 1) // (self.ntok * 4 * self.D * 2) - 1
        if self.strict_front:                                                      # ... and of the three-word patch matrix [F (ntok - 1), 3 kpad]
            self.max_frames_32bit = min(self.max_frames_32bit, (2 ** 32 - 1) // ((self.ntok - 1) * 3 * self.kpad * 2) - 1)

    # ------------------------------------------------------------------ workspace (caller-owned device buffers)
    def _workspace(self, F_, slot=0):
        """Activation buffers for up to F_ frames.  `slot` names an independent set: two forwards that run concurrently on two
        streams (ClipFsarEngine's small-batch path) must not share one."""
        cap, ws = self._slots.get(slot, (0, None))
        if F_ > cap:
            M, D, cd, dev = F_ * self.ntok, self.D, self.cd, self.dev
            ws = dict(
                x=torch.empty(M, D, device=dev, dtype=self.xd),
                h=torch.empty(M, D, device=dev, dtype=cd),
                qkv=torch.empty(M, 3 * D, device=dev, dtype=cd),
                o=torch.empty(M, 2 * D if self.o_pair else D, device=dev, dtype=cd),
                u=torch.empty(M, 4 * D, device=dev, dtype=cd),
                c=torch.empty(F_, D, device=dev, dtype=torch.float32))
            if self.strict_front:                                                            # three-word patch matrix, fp32 patch tokens
                ws["patches"] = torch.empty(F_ * (self.ntok - 1), 3 * self.kpad, device=dev, dtype=cd)
                ws["tok32"] = torch.empty(F_ * (self.ntok - 1), D, device=dev, dtype=torch.float32)
            elif not self.fused_patch:                                                       # the im2col matrix of the unfused patch embedding
                ws["patches"] = torch.empty(F_ * (self.ntok - 1), self.kpad, device=dev, dtype=cd)
            if self.fold:
                ws["part"] = torch.empty(M, D // 64, 2, device=dev, dtype=torch.float32)    # partial row statistics
                ws["rstat"] = torch.empty(M, 4, device=dev, dtype=torch.float32)            # (mean, std, 1/std, -)
            # class-token rows of the last block (prune_last): [F, .]
            if self.mcorr:
                ws["colsum"] = torch.empty((M // 96 + 2) * 2 * 4 * D, device=dev, dtype=torch.int32)   # c_fc's per-wave-tile column sums (fixed point)
                ws["mU"] = torch.empty(F_ * 4 * D, device=dev, dtype=torch.bfloat16)         # per-frame token means of the MLP hidden
                ws["mX"] = torch.empty(F_, D, device=dev, dtype=torch.bfloat16)              # ... of the attention output
                ws["xbar"] = torch.empty(F_, D, device=dev, dtype=torch.bfloat16)            # ... of the residual stream (raw), kept current by mean_update_gemm
                ws["mA"] = torch.empty(F_ * 4 * D, device=dev, dtype=torch.bfloat16)         # per-frame token means of a GEMM operand
                ws["corr"] = torch.empty(F_ * 4 * D, device=dev, dtype=torch.float32)        # ... x W_lo^T
            if self.two_word:
                ws["xlo"] = torch.empty(M, D, device=dev, dtype=torch.float16)                # second word of the stream
                ws["xlc"] = torch.empty(F_, D, device=dev, dtype=torch.float16)
                ws["c32"] = torch.empty(F_, D, device=dev, dtype=torch.float32)
            if self.fold_last_kv:                                                            # key fold, its column sums, class attend
                ws["g"] = torch.empty(F_, self.H, D, device=dev, dtype=torch.float16)
                ws["G"] = torch.empty(F_, self.H, device=dev, dtype=torch.float32)
                ws["z"] = torch.empty(F_, self.H, D, device=dev, dtype=torch.float32)
            ws["xc"] = torch.empty(F_, D, device=dev, dtype=self.xd)
            ws["hc"] = torch.empty(F_, D, device=dev, dtype=cd)
            ws["oc"] = torch.empty(F_, D, device=dev, dtype=cd)
            ws["uc"] = torch.empty(F_, 4 * D, device=dev, dtype=cd)
            ws["partc"] = torch.empty(F_, D // 64 if D % 64 == 0 else 1, 2, device=dev, dtype=torch.float32)
            ws["rstatc"] = torch.empty(F_, 4, device=dev, dtype=torch.float32)
            self._slots[slot] = (F_, ws)
        return ws

    def forward(self, frame_sets, feats_out=None, row_maps=None, taps=None, slot=0):
        """frame_sets: tensor [F,3,H,W] or list of such tensors (processed as one concatenated batch).
        feats_out: optional fp32 [*, E] buffer; row_maps: per set (row_group, row_gap, row_off) mapping the set's
        frame index m to the output feature row  m + (m // row_group) * row_gap + row_off.
        Returns feats_out (fp32)."""
        if isinstance(frame_sets, torch.Tensor):
            frame_sets = [frame_sets]
        counts = [int(f.shape[0]) for f in frame_sets]
        F_ = sum(counts)
        if row_maps is None:
            row_maps, off = [], 0
            for c in counts:
                row_maps.append((0, 0, off))
                off += c
        if feats_out is None:
            feats_out = torch.empty(F_, self.E, device=self.dev, dtype=torch.float32)
        ws = self._workspace(F_, slot)
        N, D, npatch = self.ntok, self.D, self.ntok - 1
        M = F_ * N
        x, h, qkv, o, u = ws["x"], ws["h"], ws["qkv"], ws["o"], ws["u"]
        # A2 (few_shot.py:672-676).  16 x 16 / 14 x 14 patches, 16-bit operands: ONE launch per frame set -- the GEMM gathers its rows from the fp32
        # frames, adds pos[1 + p], scatters them behind each class token and writes the class-token rows (cfsar_patch_embed).  Otherwise
        # (the fp32 mode, other patch sizes): patch gather -> GEMM with the scattering epilogue -> class-token rows.  fp16_strict: its own front end below.
        off = 0
        for fr, c in zip(frame_sets, counts):
            if fr.shape[1:] != (3, self.arch["res"], self.arch["res"]):
                raise RuntimeError("frames must be [F,3,%d,%d], got %s" % (self.arch["res"], self.arch["res"], tuple(fr.shape)))
            if self.fused_patch:
                hip.patch_embed(fr, self.w_patch_fused, self.pos, self.cls, x[off * N:(off + c) * N], self.P)
            elif self.strict_front:
                hip.im2col_patches_split(fr, ws["patches"][off * npatch:(off + c) * npatch], self.P)
            else:
                hip.im2col_patches(fr, ws["patches"][off * npatch:(off + c) * npatch], self.P)
            off += c
        if self.strict_front:
            # fp16_strict: patches [hi | lo | hi] x [W_hi | W_hi | W_lo]^T -> fp32 tokens; class token + pos + ln_pre -> x_hi, x_lo in one pass
            hip.gemm(ws["patches"], self.w_patch3, ws["tok32"], M=F_ * npatch, N=D, K=3 * self.kpad, ldo=D)
            hip.embed_finish_pair(ws["tok32"], self.cls, self.pos, self.ln_pre[0], self.ln_pre[1], x, ws["xlo"], F_, N, D)
        else:
            if not self.fused_patch:
                hip.gemm(ws["patches"], self.w_patch, x, residual=self.pos, M=F_ * npatch, N=D, K=self.kpad, ldo=D, ldr=D,
                         row_group=npatch, row_gap=1, row_off=1, res_mod=npatch, res_off=1)
                hip.cls_rows(x, self.cls, self.pos, F_, N, D)
            hip.layernorm(x, x, self.ln_pre[0], self.ln_pre[1], M, D)                 # ln_pre (:677), in place
        if taps is not None:
            taps["ln_pre"] = (x[:M].float() + ws["xlo"][:M].float()) if self.strict_front else x[:M].clone()
        xc_final = None
        es = x.element_size()

        def class_rows(src, dst, row_elems, elem_bytes):
            """dst[f] = src[f * N] (row 0 of every frame): the class-token rows / their statistics (few_shot.py:683 reads nothing else)"""
            hip.copy_rows_strided(src, N * row_elems * elem_bytes, dst, row_elems * elem_bytes, F_, row_elems * elem_bytes)

        if self.fold:
            part, rstat, S = ws["part"], ws["rstat"], D // 64
            xlo = ws["xlo"] if self.two_word else None
            if xlo is not None and not self.strict_front:
                xlo[:M].zero_()                                                       # memset: the stream enters the blocks as ln_pre's fp16 output
            hip.row_stats(x, rstat, M, D)                                             # statistics of ln_pre's output
            prune = self.prune_last and taps is None
            # ViT-B / ViT-L widths: the LN-folded GEMMs finalize the producer's partial statistics themselves (cfsar_gemm_lnfold_partials):
            # no kernel between out_proj and c_fc, c_proj and the next block's QKV (46 launches per tower call; 8 % of a one-episode step)
            fuse = self.fuse_stats
            in_part = False                                                           # statistics of x: finalized in rstat / raw in part
            split = self.split

            mcorr = self.mcorr
            raw = self.rawmeans and bool(mcorr)
            xbar = ws["xbar"][:F_] if raw else None
            if raw:
                hip.frame_col_means(x, xbar, F_, N)                                   # the one pass: the stream as it enters the blocks

            def mc(blk, key, A, rs=None, wrows=None, means=None):
                """per-frame low-word correction of GEMM `key` for the full-size launch: token means of the operand x W_lo^T -> [F, N]
                (means: already produced by the GEMM that wrote the operand)"""
                if key not in mcorr:
                    return None
                wlo = blk["wlo_" + key] if wrows is None else blk["wlo_" + key][wrows]
                Kd, Nn = A.shape[1], wlo.shape[0]
                if raw and key in ("qkv", "fc"):
                    mA = xbar                                                         # raw-stream form: no pass over x
                elif means is not None:
                    mA = means
                else:
                    mA = ws["mA"][:F_ * Kd].view(F_, Kd)
                    hip.frame_col_means(A, mA, F_, N, rowstats=rs)
                cr = ws["corr"][:F_ * Nn].view(F_, Nn)
                hip.corr_gemm(mA, wlo, cr)
                return cr

            def fold(xx, wg, out, c, d, pt, rs, act=hip.ACT_NONE, rows=M, from_part=False, sp=False, corr=None, umeans=None, corr_raw=False):
                if sp or corr is not None or umeans is not None:                      # fp16 numerics mode: split weights [N, 2K] / correction
                    hip.gemm_lnfold_hp(xx, wg, out, c, d, rowstats=None if from_part else rs, partial=pt if from_part else None,
                                       slots=S if from_part else 0, rowstats_ws=rs, act=act, M=rows, wsplit=sp, corr=corr,
                                       corr_tokens=N if (corr is not None or umeans is not None) else 0, colmean_out=umeans,
                                       colsum_ws=ws["colsum"] if umeans is not None else None, corr_raw=corr_raw and corr is not None)
                elif from_part:
                    hip.gemm_lnfold_partials(xx, wg, out, c, d, pt, S, rs, act=act, M=rows)
                else:
                    hip.gemm_lnfold(xx, wg, out, c, d, rs, act=act, M=rows)

            def resid(A, blk, key, xx, xl, pt, rows, corr=None, cls=False):
                """xx (+ xl) += A W^T + bias, partial LayerNorm statistics of the new stream -> pt (cls: the last block's class-token rows)"""
                if self.o_pair and key == "out" and not cls:                          # fp16_strict: [o_hi | o_lo] x [W_hi | W_hi | W_lo]
                    hip.gemm_residual_wide(A, blk["w3_out"], xx, xl, blk["b_out"], pt, M=rows, wsplit=2)
                elif self.wide and cls and key in mcorr:
                    hip.gemm_residual_wide(A, blk["ws_" + key], xx, xl, blk["b_" + key], pt, M=rows, wsplit=True)
                elif self.wide:
                    hip.gemm_residual_wide(A, blk["w_" + key], xx, xl, blk["b_" + key], pt, M=rows, wsplit=key in split, corr=corr,
                                           corr_tokens=N if corr is not None else 0)
                else:
                    hip.gemm_residual_stats(A, blk["w_" + key], xx, blk["b_" + key], pt, M=rows)

            for i, b in enumerate(self.blocks):                                       # :679-681, LayerNorms folded away
                if prune and i == self.L - 1:
                    # last block: K / V from every token, everything behind the attention for the class-token rows only
                    xc, oc, uc, partc, rstatc = ws["xc"][:F_], ws["oc"][:F_], ws["uc"][:F_], ws["partc"][:F_], ws["rstatc"][:F_]
                    xlc = ws["xlc"][:F_] if xlo is not None else None
                    # ... and of q only the class-token rows: K | V for all M rows (N = 2 D: two thirds of the QKV GEMM), q for F rows
                    # (option fold_last_kv: no K | V rows at all, the query is folded into the stream's rows below)
                    kv = qkv.view(-1)[:M * 2 * D].view(M, 2 * D)
                    if not self.fold_last_kv:
                        fold(x, b["wg_qkv"][D:], kv, b["cx_qkv" if raw else "c_qkv"][D:], b["d_qkv"][D:], part, rstat, from_part=in_part,
                             sp="qkv" in split, corr=mc(b, "qkv", x, rstat, wrows=slice(D, 3 * D)), corr_raw=raw)
                    class_rows(x, xc, D, es)                                          # class-token rows of the stream
                    if xlo is not None:
                        class_rows(xlo, xlc, D, 2)
                    if in_part:
                        class_rows(part, partc, 2 * S, 4)
                    else:
                        class_rows(rstat, rstatc, 4, 4)
                    qc = ws["hc"][:F_]
                    if "qkv" in mcorr:
                        fold(xc, b["wgs_qkv"], qc, b["cs_qkv"], b["d_qkv"][:D], partc, rstatc, rows=F_, from_part=in_part, sp=True)
                    else:
                        fold(xc, b["wg_qkv"][:D], qc, b["c_qkv"][:D], b["d_qkv"][:D], partc, rstatc, rows=F_, from_part=in_part, sp="qkv" in split)
                    if self.fold_last_kv:
                        from . import lastblock_hip as lb
                        g_, G_, z_ = ws["g"][:F_], ws["G"][:F_], ws["z"][:F_]
                        lb.key_fold(qc, b["wk_t"], g_, G_)
                        lb.class_attend(x, g_, G_, z_, N, partial=part if in_part else None, rowstats=None if in_part else rstat)
                        lb.value_fold(z_, b["wg_qkv"][2 * D:], b["d_qkv"][2 * D:], oc)
                    else:
                        hip.vit_attention_cls(None, oc, F_, N, D, self.H, q=qc, kv=kv)
                    resid(oc, b, "out", xc, xlc, partc, F_, cls=True)
                    if not fuse:
                        hip.ln_stats_finalize(partc, rstatc, F_, S, D)
                    if "fc" in mcorr:
                        fold(xc, b["wgs_fc"], uc, b["cs_fc"], b["d_fc"], partc, rstatc, act=hip.ACT_QUICKGELU, rows=F_, from_part=fuse, sp=True)
                    else:
                        fold(xc, b["wg_fc"], uc, b["c_fc"], b["d_fc"], partc, rstatc, act=hip.ACT_QUICKGELU, rows=F_, from_part=fuse, sp="fc" in split)
                    resid(uc, b, "pr", xc, xlc, None, F_, cls=True)
                    xc_final = xc
                    break
                fold(x, b["wg_qkv"], qkv, b["cx_qkv" if raw else "c_qkv"], b["d_qkv"], part, rstat, from_part=in_part, sp="qkv" in split,
                     corr=mc(b, "qkv", x, rstat), corr_raw=raw)
                if self.o_pair:                                                    # fp16_strict: two-word attention output (+ its per-frame means)
                    mO = ws["mX"][:F_]
                    hip.vit_attention_pair(qkv, o, mO, F_, N, D, self.H)
                elif "out" in mcorr and self.fused_omeans:                         # the attention kernel emits its output's per-frame means
                    mO = ws["mX"][:F_]
                    hip.vit_attention_means(qkv, o, mO, F_, N, D, self.H)
                else:
                    mO = None
                    hip.vit_attention(qkv, o, F_, N, D, self.H)
                resid(o, b, "out", x, xlo, part, M, corr=None if self.o_pair else mc(b, "out", o, means=mO))   # x += out_proj(attn); stats of the new x
                if raw:
                    hip.mean_update_gemm(mO, b["wb_out"], b["b_out"], xbar)           # ... and its per-frame mean follows
                if not fuse:
                    hip.ln_stats_finalize(part, rstat, M, S, D)
                # c_fc also emits the per-frame token means of the hidden it writes: c_proj's correction needs no pass of its own over u
                um = ws["mU"][:F_ * 4 * D].view(F_, 4 * D) if ("pr" in mcorr and self.fused_umeans) else None
                fold(x, b["wg_fc"], u, b["cx_fc" if raw else "c_fc"], b["d_fc"], part, rstat, act=hip.ACT_QUICKGELU, from_part=fuse, sp="fc" in split,
                     corr=mc(b, "fc", x, rstat), umeans=um, corr_raw=raw)
                resid(u, b, "pr", x, xlo, part, M, corr=mc(b, "pr", u, means=um))      # x += c_proj(gelu(c_fc))
                if raw:
                    hip.mean_update_gemm(um, b["wb_pr"], b["b_pr"], xbar)
                if fuse:
                    in_part = True
                else:
                    hip.ln_stats_finalize(part, rstat, M, S, D)
                if taps is not None:
                    taps["block%d" % i] = (x[:M].float() + xlo[:M].float()) if xlo is not None else x[:M].clone()
        for i, b in enumerate(self.blocks if not self.fold else []):                  # :679-681
            if self.prune_last and taps is None and i == self.L - 1:
                xc, hc, oc, uc = ws["xc"][:F_], ws["hc"][:F_], ws["oc"][:F_], ws["uc"][:F_]
                hip.layernorm(x, h, b["ln1"][0], b["ln1"][1], M, D)
                hip.gemm(h, b["w_qkv"], qkv, bias=b["b_qkv"], M=M)
                hip.vit_attention_cls(qkv, oc, F_, N, D, self.H)
                class_rows(x, xc, D, es)
                hip.gemm(oc, b["w_out"], xc, bias=b["b_out"], residual=xc, M=F_)
                hip.layernorm(xc, hc, b["ln2"][0], b["ln2"][1], F_, D)
                hip.gemm(hc, b["w_fc"], uc, bias=b["b_fc"], act=hip.ACT_QUICKGELU, M=F_)
                hip.gemm(uc, b["w_pr"], xc, bias=b["b_pr"], residual=xc, M=F_)
                xc_final = xc
                break
            hip.layernorm(x, h, b["ln1"][0], b["ln1"][1], M, D)
            hip.gemm(h, b["w_qkv"], qkv, bias=b["b_qkv"], M=M)
            hip.vit_attention(qkv, o, F_, N, D, self.H)
            hip.gemm(o, b["w_out"], x, bias=b["b_out"], residual=x, M=M)              # x += out_proj(attn)
            hip.layernorm(x, h, b["ln2"][0], b["ln2"][1], M, D)
            hip.gemm(h, b["w_fc"], u, bias=b["b_fc"], act=hip.ACT_QUICKGELU, M=M)
            hip.gemm(u, b["w_pr"], x, bias=b["b_pr"], residual=x, M=M)                # x += c_proj(gelu(c_fc))
            if taps is not None:
                taps["block%d" % i] = x[:M].clone()
        # A8: ln_post on the class-token rows (stride N*D) then @ proj, fp32
        if self.fold and self.two_word:                                                # two-word stream: ln_post reads x_hi + x_lo
            if xc_final is None:
                xc_final = ws["xc"][:F_]
                class_rows(x, xc_final, D, es)
                class_rows(ws["xlo"], ws["xlc"][:F_], D, 2)
            hip.f16_pair_to_f32(xc_final, ws["xlc"][:F_], ws["c32"][:F_])
            hip.layernorm(ws["c32"], ws["c"], self.ln_post[0], self.ln_post[1], F_, D, in_stride=D, out_stride=D)
        elif xc_final is not None:
            hip.layernorm(xc_final, ws["c"], self.ln_post[0], self.ln_post[1], F_, D, in_stride=D, out_stride=D)
        else:
            hip.layernorm(x, ws["c"], self.ln_post[0], self.ln_post[1], F_, D, in_stride=N * D, out_stride=D)
        off = 0
        for c, (rg, gap, roff) in zip(counts, row_maps):
            hip.gemm(ws["c"][off:off + c], self.w_proj_t, feats_out, M=c, N=self.E, K=D, ldo=self.E,
                     row_group=rg, row_gap=gap, row_off=roff)
            off += c
        return feats_out


class HipResNet:
    """N3: CLIP ModifiedResNet.forward (reference few_shot.py:581-602) on the HIP kernels.

    NHWC activations; BatchNorm (eval, running statistics) folded into the conv weights and a per-channel bias on the
    host; 1x1 convs are cfsar_gemm rows, 3x3 convs a tap-major gather + cfsar_gemm; ReLU / identity-add are GEMM
    epilogues; avgpool anti-aliasing and the attention-pool token build are small NHWC kernels; the attention pool computes k/v
    for every token but q and the softmax only for the one query it keeps (the mean token)."""

    IMPLICIT_MIN_TILES = 128          # 256x256 output tiles below which the implicit-GEMM conv would leave CUs idle

    def __init__(self, arch: dict, sd: dict, prefix: str = "", precision: str = "bf16", device="cuda"):
        if precision == "fp16_strict":
            raise ValueError("precision 'fp16_strict' exists for the ViT towers; the RN50 tower's mode for the 1e-3 contract is 'fp32'")
        if precision not in ("bf16", "fp16", "fp32"):
            raise ValueError("precision must be 'bf16', 'fp16' or 'fp32'")
        self.arch = dict(arch)
        self.dev = torch.device(device)
        # fp16: the same graph on IEEE-half activations and weights (fp32 accumulation, one rounding per stored tensor) at 0.95 x the bf16
        # rate: feature error 8e-4 relative against bf16's 6e-3 (tools/numerics_lab_rn.py, tools/rn_fp16_probe.py); logits inside 1e-3 on
        # the goldens (3.7e-4) and the bench's episodes (1.7e-4), rms 8e-4 / max 2.5e-3 on high-contrast 8-frame episodes (tests/test_gpu_e2e.py::
        # test_rn50_fp16_mode_steady_parity_statistic) -- "fp32" is the mode for a strict 1e-3 there.  BatchNorm is folded, so the range
        # is that of the reference's own fp16 checkpoints (few_shot.py:258-262 convert_weights); checked per conv below
        self.cd = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}[precision]
        self.kq = 32 if precision == "fp32" else 64
        self.E = arch["embed"]
        self.width, self.layers, self.heads = arch["width"], arch["layers"], arch["heads"]
        # frames per tower launch: the widest activation (stem output / layer1 output: (res / 2)^2 x width, respectively (res / 4)^2 x 4 width
        # elements per frame) must stay addressable with 32-bit byte offsets -- beyond it the convs fall back to slower forms (36 cfg-rn50
        # episodes per call: 577 episodes/s against 635 at 32, profiles/r05_bench_rn50_epoch_size.txt); ClipFsarEngine chunks at this bound
        self.max_frames_32bit = (2 ** 32 - 1) // ((arch["res"] // 2) ** 2 * self.width * (4 if precision == "fp32" else 2)) - 1
        if (self.width * 32) % self.heads or (self.width * 32) // self.heads > 128:
            raise ValueError("attention-pool head_dim must be <= 128")

        def g(name):
            t = sd[prefix + name]
            if not isinstance(t, torch.Tensor):
                t = torch.from_numpy(t)
            return t.detach().to(device=self.dev, dtype=torch.float32)

        def fold(conv, bn):
            """conv (no bias) + BatchNorm(eval): W' = W * s, b' = beta - mean * s, s = gamma / sqrt(var + eps)."""
            w = g(conv + ".weight")
            s_ = g(bn + ".weight") / torch.sqrt(g(bn + ".running_var") + 1e-5)
            b = g(bn + ".bias") - g(bn + ".running_mean") * s_
            w = w * s_.reshape(-1, 1, 1, 1)
            cout, cin, k, _ = w.shape
            w2 = w.permute(0, 2, 3, 1).reshape(cout, k * k * cin)                 # tap-major: (ky, kx, cin)
            kpad = _round_up(w2.shape[1], self.kq)
            wp = torch.zeros(cout, kpad, device=self.dev, dtype=torch.float32)
            wp[:, :w2.shape[1]] = w2
            if self.cd == torch.float16 and float(wp.abs().max()) > 6.0e4:
                raise ValueError("precision 'fp16': the BatchNorm-folded weights of %s leave the fp16 range (max |w| = %.3g); use 'bf16' or "
                                 "'fp32'" % (conv, float(wp.abs().max())))
            return wp.to(self.cd).contiguous(), b.contiguous()

        self.stem = [fold("conv1", "bn1"), fold("conv2", "bn2"), fold("conv3", "bn3")]
        # bf16 mode: conv1 runs as a direct fp32 kernel on the NCHW frames (K = 27 is too short for the matrix cores and the
        # layer is HBM-bound); the fp32 validation mode keeps the gather + exact-fp32 MFMA GEMM
        self.stem_direct = None
        if self.cd != torch.float32 and (self.width // 2) in (8, 16, 32, 64):
            s1 = g("bn1.weight") / torch.sqrt(g("bn1.running_var") + 1e-5)
            self.stem_direct = ((g("conv1.weight") * s1.reshape(-1, 1, 1, 1)).contiguous(),
                                (g("bn1.bias") - g("bn1.running_mean") * s1).contiguous())
        self.blocks = []
        inplanes = self.width
        for li, (planes, nb) in enumerate(zip((self.width, self.width * 2, self.width * 4, self.width * 8), self.layers), 1):
            for bi in range(nb):
                stride = 2 if (li > 1 and bi == 0) else 1
                b = "layer%d.%d." % (li, bi)
                blk = dict(stride=stride, planes=planes, inplanes=inplanes, c1=fold(b + "conv1", b + "bn1"),
                           c2=fold(b + "conv2", b + "bn2"), c3=fold(b + "conv3", b + "bn3"), down=None)
                if stride > 1 or inplanes != planes * 4:
                    blk["down"] = fold(b + "downsample.0", b + "downsample.1")
                self.blocks.append(blk)
                inplanes = planes * 4
        self.C = inplanes
        self.pos = g("attnpool.positional_embedding").contiguous()
        self.w_q = g("attnpool.q_proj.weight").to(self.cd).contiguous()
        self.b_q = g("attnpool.q_proj.bias").contiguous()
        self.w_kv = torch.cat([g("attnpool.k_proj.weight"), g("attnpool.v_proj.weight")], 0).to(self.cd).contiguous()
        self.b_kv = torch.cat([g("attnpool.k_proj.bias"), g("attnpool.v_proj.bias")], 0).contiguous()
        self.w_c = g("attnpool.c_proj.weight").contiguous()                     # final projection in fp32
        self.b_c = g("attnpool.c_proj.bias").contiguous()

    def _conv3x3(self, x, F_, H, W, C, wb, stride):
        w, b = wb
        # implicit GEMM (no im2col matrix) when the tile grid fills the chip; the stem's first conv (C = 3, stride 2)
        # and small launches keep the explicit gather + GEMM
        if (stride == 1 and self.cd != torch.float32 and C >= 8 and (C & (C - 1)) == 0
                and ((F_ * H * W + 255) // 256) * ((w.shape[0] + 255) // 256) >= self.IMPLICIT_MIN_TILES):
            out = torch.empty(F_ * H * W, w.shape[0], device=self.dev, dtype=self.cd)
            hip.conv3x3(x, w, out, F_, H, W, C, bias=b, relu=True)
            return out, H, W
        Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
        cols = torch.empty(F_ * Ho * Wo, w.shape[1], device=self.dev, dtype=self.cd)
        hip.im2col3x3(x, cols, F_, H, W, C, stride)
        out = torch.empty(F_ * Ho * Wo, w.shape[0], device=self.dev, dtype=self.cd)
        hip.gemm(cols, w, out, bias=b, relu=True)
        return out, Ho, Wo

    def _pool(self, x, F_, H, W, C):
        out = torch.empty(F_ * (H // 2) * (W // 2), C, device=self.dev, dtype=self.cd)
        hip.avgpool2x2(x, out, F_, H, W, C)
        return out

    def forward(self, frame_sets, feats_out=None, row_maps=None, taps=None):
        if isinstance(frame_sets, torch.Tensor):
            frame_sets = [frame_sets]
        counts = [int(f.shape[0]) for f in frame_sets]
        F_ = sum(counts)
        if row_maps is None:
            row_maps, off = [], 0
            for c in counts:
                row_maps.append((0, 0, off))
                off += c
        if feats_out is None:
            feats_out = torch.empty(F_, self.E, device=self.dev, dtype=torch.float32)
        res = self.arch["res"]
        for fr in frame_sets:
            if fr.shape[1:] != (3, res, res):
                raise RuntimeError("frames must be [F,3,%d,%d], got %s" % (res, res, tuple(fr.shape)))
        H = W = res
        if self.stem_direct is not None:
            # stem conv1 (:582-586) straight from the fp32 NCHW frames: no layout pass, no im2col matrix
            Ho = (res - 1) // 2 + 1
            x = torch.empty(F_ * Ho * Ho, self.width // 2, device=self.dev, dtype=self.cd)
            off = 0
            for fr, c in zip(frame_sets, counts):
                hip.stem_conv(fr, self.stem_direct[0], self.stem_direct[1], x[off * Ho * Ho:(off + c) * Ho * Ho], relu=True)
                off += c
            H = W = Ho
        else:
            x = torch.empty(F_ * res * res, 3, device=self.dev, dtype=self.cd)
            off = 0
            for fr, c in zip(frame_sets, counts):
                hip.nchw_to_nhwc(fr, x[off * res * res:(off + c) * res * res])
                off += c
            x, H, W = self._conv3x3(x, F_, H, W, 3, self.stem[0], 2)                     # stem (:582-586)
        x, H, W = self._conv3x3(x, F_, H, W, self.width // 2, self.stem[1], 1)
        x, H, W = self._conv3x3(x, F_, H, W, self.width // 2, self.stem[2], 1)
        x = self._pool(x, F_, H, W, self.width)
        H, W = H // 2, W // 2
        for blk in self.blocks:                                                          # Bottleneck.forward (:213-226)
            p_, inp, st = blk["planes"], blk["inplanes"], blk["stride"]
            M = F_ * H * W
            o1 = torch.empty(M, p_, device=self.dev, dtype=self.cd)
            hip.gemm(x, blk["c1"][0], o1, bias=blk["c1"][1], relu=True)
            o2, _, _ = self._conv3x3(o1, F_, H, W, p_, blk["c2"], 1)
            xi = x
            if st > 1:
                o2 = self._pool(o2, F_, H, W, p_)
                xi = self._pool(x, F_, H, W, inp)
                H, W = H // 2, W // 2
                M = F_ * H * W
            if blk["down"] is not None:
                idn = torch.empty(M, 4 * p_, device=self.dev, dtype=self.cd)
                hip.gemm(xi, blk["down"][0], idn, bias=blk["down"][1])
            else:
                idn = xi
            out = torch.empty(M, 4 * p_, device=self.dev, dtype=self.cd)
            hip.gemm(o2, blk["c3"][0], out, bias=blk["c3"][1], residual=idn, relu=True)
            x = out
        if taps is not None:
            taps["layer4"] = x.clone()
        HW, C = H * W, self.C                                                            # AttentionPool2d (:446-538)
        tok = torch.empty(F_ * (HW + 1), C, device=self.dev, dtype=self.cd)
        hip.attnpool_tokens(x, self.pos, tok, F_, HW, C)
        T = HW + 1
        kv = torch.empty(F_ * T, 2 * C, device=self.dev, dtype=torch.float32)            # k and v of every token
        hip.gemm(tok, self.w_kv, kv, bias=self.b_kv)
        q = torch.empty(F_, C, device=self.dev, dtype=torch.float32)                      # q of the mean token only
        hip.gemm(tok, self.w_q, q, bias=self.b_q, M=F_, N=C, K=C, lda=T * C)
        hd = C // self.heads
        pooled = torch.empty(F_, C, device=self.dev, dtype=torch.float32)
        hip.attnpool_attend(q, kv, pooled, F_, T, self.heads, hd, hd ** -0.5)
        off = 0
        for c, (rg, gap, roff) in zip(counts, row_maps):
            hip.gemm(pooled[off:off + c], self.w_c, feats_out, bias=self.b_c, M=c, N=self.E, K=C, ldo=self.E,
                     row_group=rg, row_gap=gap, row_off=roff)
            off += c
        return feats_out


class HipTemporalHead:
    """context2 (Transformer_v1) + prototypes + cosine/OTAM -> logits, fp32 (few_shot.py:2937-2990)."""

    def __init__(self, sd: dict, dim: int, depth: int = 1, heads: int = 8, prefix: str = "context2.", device="cuda"):
        self.dev = torch.device(device)
        self.dim, self.depth, self.heads = dim, depth, heads

        def g(name):
            t = sd[prefix + name]
            if not isinstance(t, torch.Tensor):
                t = torch.from_numpy(t)
            return t.detach().to(device=self.dev, dtype=torch.float32).contiguous()

        self.layers = []
        for d in range(depth):
            p = "layers.%d." % d
            wq, wk, wv = g(p + "0.fn.to_q.weight"), g(p + "0.fn.to_k.weight"), g(p + "0.fn.to_v.weight")
            inner = wq.shape[0]
            self.layers.append(dict(
                norm=(g(p + "0.norm.weight"), g(p + "0.norm.bias")),
                w_qkv=torch.cat([wq, wk, wv], 0).contiguous(), inner=inner,
                w_out=g(p + "0.fn.to_out.0.weight"), b_out=g(p + "0.fn.to_out.0.bias"),
                w1=g(p + "1.net.0.weight"), b1=g(p + "1.net.0.bias"),
                w2=g(p + "1.net.3.weight"), b2=g(p + "1.net.3.bias")))
        self._ws_rows = 0
        self._ws = None

    def _workspace(self, rows):
        if rows > self._ws_rows:
            E, dev = self.dim, self.dev
            inner = max(l["inner"] for l in self.layers)
            hidden = max(l["w1"].shape[0] for l in self.layers)
            f = lambda *s: torch.empty(*s, device=dev, dtype=torch.float32)
            self._ws = dict(X=f(rows, E), n=f(rows, E), qkv=f(rows, 3 * inner), o=f(rows, inner), y=f(rows, E),
                            u=f(rows, hidden), z=f(rows, E))
            self._ws_rows = rows
        return self._ws

    def run_layers(self, rows, n_a, len_a, n_b, len_b):
        """context2's layer loop (few_shot.py:990-999) on the first `rows` rows of the workspace's X (_workspace(rows)["X"], written by the
        caller): n_a sequences of len_a rows, then n_b of len_b (either count may be 0).  Returns the workspace buffer that holds the
        output; it is overwritten by the next call."""
        E = self.dim
        ws = self._workspace(rows)
        cur, nxt = ws["X"], ws["z"]
        for l in self.layers:                                                            # few_shot.py:990-999
            inner = l["inner"]
            hd = inner // self.heads
            hip.layernorm(cur, ws["n"], l["norm"][0], l["norm"][1], rows, E)              # shared LN for q,k,v (:971-977)
            hip.gemm(ws["n"], l["w_qkv"], ws["qkv"], M=rows)                              # to_q|to_k|to_v, no bias
            hip.seq_attention(ws["qkv"], ws["o"], n_a, len_a, n_b, len_b, self.heads, hd, hd ** -0.5)
            hip.gemm(ws["o"], l["w_out"], ws["y"], bias=l["b_out"], residual=cur, M=rows)   # to_out + q residual
            hip.gemm(ws["y"], l["w1"], ws["u"], bias=l["b1"], act=hip.ACT_GELU_ERF, M=rows)
            hip.gemm(ws["u"], l["w2"], nxt, bias=l["b2"], residual=ws["y"], M=rows)         # ff(x) + x
            cur, nxt = nxt, cur
        return cur

    def forward(self, feats, text_test, support_labels, real_support_labels, B, S, Q, T, way, merge_before=False,
                single_direct=False, taps=None):
        """feats [B, S+Q, T, E] fp32 -> logits [B, Q, way] fp32."""
        E = self.dim
        Sp = way if merge_before else S
        rows_q, rows_s = B * Q * T, B * Sp * (T + 1)
        rows = rows_q + rows_s
        ws = self._workspace(rows)
        hip.build_sequences(feats, text_test, support_labels, real_support_labels, ws["X"], B, S, Q, T, E, way, merge_before)
        cur = self.run_layers(rows, B * Q, T, B * Sp, T + 1)
        protos = torch.empty(B, way, T, E, device=self.dev, dtype=torch.float32)
        hip.prototypes(cur[rows_q:], support_labels, protos, B, S, Sp, T, E, way, merge_before)
        logits = torch.empty(B, Q, way, device=self.dev, dtype=torch.float32)
        dists = torch.empty(B, Q, way, T, T, device=self.dev, dtype=torch.float32) if taps is not None else None
        hip.cos_otam_logits(cur[:rows_q], protos, logits, B, Q, way, T, E, 0.5, single_direct, dists_out=dists)
        if taps is not None:
            taps.update(ctx_q=cur[:rows_q].clone().reshape(B, Q, T, E), protos=protos, dists=dists)
        return logits


class ClipFsarEngine:
    """Full episodic forward A0 -> A15 for a batch of B episodes with identical (way, shot, query, T)."""

    def __init__(self, arch: dict, head_sd: dict, text_train, text_test, depth: int = 1, precision: str = "bf16",
                 device="cuda", max_frames: int = 2880, fp16_split=None, fp16_mcorr=None, vit_options=None):
        self.dev = torch.device(device)
        self.arch = dict(arch)
        if arch.get("kind") == "rn":
            self.vit = HipResNet(arch, head_sd, prefix="backbone.", precision=precision, device=device)
        else:
            self.vit = HipViT(arch, head_sd, prefix="backbone.", precision=precision, device=device, fp16_split=fp16_split,
                              fp16_mcorr=fp16_mcorr, options=vit_options)
        self.temporal = HipTemporalHead(head_sd, arch["embed"], depth=depth, device=device)
        f32 = lambda t: (t if isinstance(t, torch.Tensor) else torch.from_numpy(t)).detach().to(
            device=self.dev, dtype=torch.float32).contiguous()
        self.text_train, self.text_test = f32(text_train), f32(text_test)
        self.scale = f32(head_sd["scale"])
        # frames per tower launch: the kernels address an activation matrix with 32-bit byte offsets, the widest one is the MLP
        # hidden [F * tokens, 4 D] in 2 bytes (ViT-B/16: 3 548 frames fit; the engine keeps one frame of margin: 3 547); larger episode batches run the tower in chunks
        limit = getattr(self.vit, "max_frames_32bit", None)
        self.max_frames = min(max_frames, limit) if limit else max_frames

    def forward(self, support_set, target_set, support_labels, real_support_labels, way, T, merge_before=False,
                single_direct=False, taps=None, mode="otam", text_coff=0.9):
        """support_set [B, S*T, 3, H, W], target_set [B, Q*T, 3, H, W] fp32 device tensors (B may be folded in:
        4-D inputs mean B = 1); labels [B, S] fp32.  Returns (logits [B,Q,way], class_logits [B,S+Q,n_train])."""
        if support_set.dim() == 4:
            support_set, target_set = support_set.unsqueeze(0), target_set.unsqueeze(0)
            support_labels, real_support_labels = support_labels.reshape(1, -1), real_support_labels.reshape(1, -1)
        B = support_set.shape[0]
        S, Q = support_set.shape[1] // T, target_set.shape[1] // T
        E = self.arch["embed"]
        per_ep = (S + Q) * T
        feats = torch.empty(B, S + Q, T, E, device=self.dev, dtype=torch.float32)
        chunk = max(1, self.max_frames // per_ep)
        feats2d = feats.reshape(B * per_ep, E)
        for b0 in range(0, B, chunk):
            b1 = min(B, b0 + chunk)
            sup = support_set[b0:b1].reshape(-1, *support_set.shape[2:])
            tgt = target_set[b0:b1].reshape(-1, *target_set.shape[2:])
            self.vit.forward([sup, tgt], feats2d,
                             row_maps=[(S * T, Q * T, b0 * per_ep), (Q * T, S * T, b0 * per_ep + S * T)],
                             taps=taps if b0 == 0 else None)
        sl = support_labels.to(device=self.dev, dtype=torch.float32).contiguous()
        rl = real_support_labels.to(device=self.dev, dtype=torch.float32).contiguous()
        if mode in ("eval_text", "combine"):                     # N4: few_shot.py:2835-2852 / :2855-2930
            probs = torch.empty(B, Q, way, device=self.dev, dtype=torch.float32)
            hip.text_match_probs(feats, self.text_test, sl, rl, self.scale, probs, B, S, Q, T, E, way)
            if mode == "eval_text":
                return probs, None                               # logits = -cum_dists = softmax probs; class_logits None
            vis = self.temporal.forward(feats, self.text_test, sl, rl, B, S, Q, T, way, merge_before, single_direct)
            out = torch.empty_like(probs)
            hip.combine_logits(probs, vis, out, B * Q, way, text_coff)
            return out, None
        class_logits = torch.empty(B, S + Q, self.text_train.shape[0], device=self.dev, dtype=torch.float32)
        hip.class_text_logits(feats, self.text_train, self.scale, class_logits, B * (S + Q), T, E)
        logits = self.temporal.forward(feats, self.text_test, sl, rl, B, S, Q, T, way, merge_before, single_direct,
                                       taps=taps)
        if taps is not None:
            taps["feats"] = feats
        return logits, class_logits
