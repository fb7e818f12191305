"""Time the support gallery on the GPU (run as a fresh process; HIP events around every step).

    python tools/gallery_time.py [--out profiles/gallery_time.json] [--reps 10]

1. cfsg_otam_gallery (the gallery kernel) against cfsar_cos_otam_logits at B = 1 (the episode kernel) on the same operands, at
   (NQ, C) in {(1024, 24), (1024, 1024), (4096, 256)} for T = 8, E = 512 and T = 16, E = 768, plus a sweep of small C at
   (1024, C, 8, 512) for the crossover below which the episode kernel is faster;
2. the similarity GEMM's share of the 157.3 TF fp32 MFMA peak: 2 NQ T C T E FLOP over the gallery kernel's whole time (the DP epilogue
   included, so this is a lower bound of the GEMM's own rate);
3. end-to-end SupportGallery.classify queries/s at ViT-B/16 bf16 (tower + context2 + norms + the gallery kernel) for 100 classes x 5 shots,
   and the time to register them.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from _timing import _time_ms  # noqa: E402  (tools/_timing.py)

PEAK_F32_MFMA_TF = 157.3          # MI355X: f32-input MFMA = the f32 vector peak (64 FLOP / clk / SIMD)


def kernel_point(NQ, C, T, E, reps):
    from clip_fsar_amd import gallery_hip as gh
    from clip_fsar_amd import hip
    g = torch.Generator(device="cuda").manual_seed(NQ + C)
    base = torch.randn(E, device="cuda", generator=g)
    Xq = (base + torch.randn(NQ, T, E, device="cuda", generator=g)).contiguous()
    P = (base + torch.randn(C, T, E, device="cuda", generator=g)).contiguous()
    qn, pn = torch.empty(NQ * T, device="cuda"), torch.empty(C * T, device="cuda")
    gh.row_norms(Xq, qn)
    gh.row_norms(P, pn)
    lg, lg_ep = torch.empty(NQ, C, device="cuda"), torch.empty(1, NQ, C, device="cuda")
    t_g = _time_ms(lambda: gh.otam_gallery(Xq, qn, P, pn, lg), reps)
    t_n = _time_ms(lambda: gh.row_norms(Xq, qn), reps)
    t_e = _time_ms(lambda: hip.cos_otam_logits(Xq, P, lg_ep, 1, NQ, C, T, E), max(3, reps // 3))
    torch.cuda.synchronize()
    flop = 2.0 * NQ * T * C * T * E
    return {"NQ": NQ, "C": C, "T": T, "E": E, "gallery_ms": round(t_g, 4), "query_norms_ms": round(t_n, 4), "episode_kernel_ms": round(t_e, 4),
            "speedup": round(t_e / (t_g + t_n), 2), "sim_gflop": round(flop / 1e9, 2), "sim_tflops": round(flop / t_g / 1e9, 1),
            "frac_f32_mfma_peak": round(flop / t_g / 1e9 / PEAK_F32_MFMA_TF, 3),
            "max_abs_diff_vs_episode_kernel": float((lg - lg_ep[0]).abs().max())}


def classify_rate(reps, n_classes=100, shots=5, n_queries=256):
    from types import SimpleNamespace as NS
    import clip_fsar_amd.synth as synth
    from clip_fsar_amd.gallery import SupportGallery
    from clip_fsar_amd.models.base.few_shot import CNN_OTAM_CLIPFSAR
    T = 8
    cfg = NS(VIDEO=NS(HEAD=NS(NAME="CNN_OTAM_CLIPFSAR", BACKBONE_NAME="ViT-B/16", PRECISION="bf16"), BACKBONE=NS(META_ARCH="Identity")),
             TRAIN=NS(CLASS_NAME=["c%d" % i for i in range(64)], WAY=5), TEST=NS(CLASS_NAME=["t%d" % i for i in range(n_classes)]),
             DATA=NS(NUM_INPUT_FRAMES=T), MODEL=NS(NAME="BaseVideoModel", EMA=NS(ENABLE=False)), BN=NS(FREEZE=False), NUM_GPUS=1,
             NUM_SHARDS=1, RANDOM_SEED=18)
    head = CNN_OTAM_CLIPFSAR(cfg).eval()
    res = synth.ARCHS["ViT-B/16"]["res"]
    g = torch.Generator(device="cuda").manual_seed(1)
    V = torch.randn(n_classes * shots, T, 3, res, res, device="cuda", generator=g)
    Q = torch.randn(n_queries, T, 3, res, res, device="cuda", generator=g)
    ids = [i // shots for i in range(n_classes * shots)]
    with torch.no_grad():
        gal = SupportGallery(head, "cuda")
        gal.add_classes(V[:shots], ids[:shots])            # warm-up: engine, workspaces
        gal.clear()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        gal.add_classes(V, ids)
        torch.cuda.synchronize()
        t_reg = time.perf_counter() - t0
        t_cls = _time_ms(lambda: gal.classify(Q), reps)
    return {"arch": "ViT-B/16", "precision": "bf16", "classes": n_classes, "shots": shots, "register_s": round(t_reg, 3),
            "queries_per_call": n_queries, "classify_ms": round(t_cls, 2), "queries_per_s": round(n_queries / t_cls * 1e3, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gallery_time.json"))
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0), "kernel": [], "crossover_sweep": []}
    for T, E in ((8, 512), (16, 768)):
        for NQ, C in ((1024, 24), (1024, 1024), (4096, 256)):
            r = kernel_point(NQ, C, T, E, args.reps)
            print(json.dumps(r), flush=True)
            out["kernel"].append(r)
    for C in (5, 8, 16, 24, 32, 64):
        r = kernel_point(1024, C, 8, 512, args.reps)
        print(json.dumps(r), flush=True)
        out["crossover_sweep"].append(r)
    slower = [r["C"] for r in out["crossover_sweep"] if r["speedup"] < 1.0]
    out["episode_kernel_faster_below_C"] = (max(slower) + 1) if slower else 0
    out["classify"] = classify_rate(args.reps)
    print(json.dumps(out["classify"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
