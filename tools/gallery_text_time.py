"""Time the text gallery on the GPU (run as a fresh process; HIP events, medians over --reps timed calls after a warm-up call).

    python tools/gallery_text_time.py [--out profiles/gallery_text_time.json] [--reps 10]

1. cfgt_text_logits + cfgt_text_softmax (EVAL_TEXT) and cfgt_text_logits + cfgt_text_combine (COMBINE) at (NQ, C, E) in
   {(1024, 24, 512), (1024, 1024, 512), (4096, 10000, 768)}, beside cfsg_otam_gallery at the same NQ x C (T = 8) for scale;
2. the text GEMM's share of the 157.3 TF fp32 MFMA peak: 2 NQ C E FLOP over cfgt_text_logits' time (epilogue included);
3. end-to-end TextGallery.classify queries/s in both modes at ViT-B/16 bf16 for 100 classes x 5 shots.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from _timing import _time_ms  # noqa: E402  (tools/_timing.py)

PEAK_F32_MFMA_TF = 157.3          # MI355X: f32-input MFMA = the f32 vector peak (64 FLOP / clk / SIMD)


def kernel_point(NQ, C, E, reps, T=8):
    from clip_fsar_amd import gallery_hip as gh
    from clip_fsar_amd import gallery_text_hip as gt
    g = torch.Generator(device="cuda").manual_seed(NQ + C)
    base = torch.randn(E, device="cuda", generator=g)
    emb = (base + torch.randn(NQ, E, device="cuda", generator=g)).contiguous()
    text = (base + torch.randn(C, E, device="cuda", generator=g)).contiguous()
    vis = -(4.0 + 8.0 * torch.rand(NQ, C, device="cuda", generator=g))
    en, tn = torch.empty(NQ, device="cuda"), torch.empty(C, device="cuda")
    gh.row_norms(emb, en)
    gh.row_norms(text, tn)
    scale = torch.tensor([4.0], device="cuda")
    lg, out = torch.empty(NQ, C, device="cuda"), torch.empty(NQ, C, device="cuda")
    part = torch.empty(gt.workspace_floats(NQ, C), device="cuda")
    t_l = _time_ms(lambda: gt.text_logits(emb, en, text, tn, scale, lg, part), reps)
    t_s = _time_ms(lambda: (gt.text_logits(emb, en, text, tn, scale, lg, part), gt.text_softmax(lg, part, out)), reps)
    t_c = _time_ms(lambda: (gt.text_logits(emb, en, text, tn, scale, lg, part), gt.text_combine(lg, part, vis, out, 0.9)), reps)
    # the OTAM gallery kernel at the same NQ x C (T = 8), the other half of a COMBINE classify
    Xq = torch.randn(NQ, T, E, device="cuda", generator=g)
    P = torch.randn(C, T, E, device="cuda", generator=g)
    qn, pn = torch.empty(NQ * T, device="cuda"), torch.empty(C * T, device="cuda")
    gh.row_norms(Xq, qn)
    gh.row_norms(P, pn)
    t_o = _time_ms(lambda: gh.otam_gallery(Xq, qn, P, pn, lg), max(3, reps // 2))
    flop = 2.0 * NQ * C * E
    return {"NQ": NQ, "C": C, "E": E, "text_logits_ms": round(t_l, 4), "logits_softmax_ms": round(t_s, 4),
            "logits_combine_ms": round(t_c, 4), "otam_gallery_T8_ms": round(t_o, 4), "gemm_gflop": round(flop / 1e9, 3),
            "gemm_tflops": round(flop / t_l / 1e9, 1), "frac_f32_mfma_peak": round(flop / t_l / 1e9 / PEAK_F32_MFMA_TF, 3)}


def classify_rate(reps, n_classes=100, shots=5, n_queries=256):
    from types import SimpleNamespace as NS
    import clip_fsar_amd.synth as synth
    from clip_fsar_amd.gallery import SupportGallery
    from clip_fsar_amd.models.base.few_shot import CNN_OTAM_CLIPFSAR
    from clip_fsar_amd.text_gallery import TextGallery
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
    out = {"arch": "ViT-B/16", "precision": "bf16", "classes": n_classes, "shots": shots, "queries_per_call": n_queries}
    with torch.no_grad():
        for name, gal in (("otam", SupportGallery(head, "cuda")), ("eval_text", TextGallery(head, "cuda", mode="eval_text")),
                          ("combine", TextGallery(head, "cuda", mode="combine"))):
            gal.add_classes(V, ids)
            t = _time_ms(lambda: gal.classify(Q), reps)
            out[name] = {"classify_ms": round(t, 2), "queries_per_s": round(n_queries / t * 1e3, 1)}
            print(name, json.dumps(out[name]), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gallery_text_time.json"))
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0), "kernel": []}
    for NQ, C, E in ((1024, 24, 512), (1024, 1024, 512), (4096, 10000, 768)):
        r = kernel_point(NQ, C, E, args.reps)
        print(json.dumps(r), flush=True)
        out["kernel"].append(r)
    out["classify"] = classify_rate(args.reps)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
