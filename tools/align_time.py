"""Time the OTAM alignment on the GPU (run as a fresh process; HIP events around every leg).

    python tools/align_time.py [--out profiles/align_time.json] [--reps 10] [--classes 3200]

32 x 8 windows, T = 8, E = 512 (ViT-B/16 head, bf16 tower -- the tower does not run: the legs start from tower features), against a
LiveGallery of 3 200 classes of one shot each.  Two legs:

  topk        LiveGallery.classify_features over all classes and cfsg_topk with k = 5 of the same clips: what a caller who wants a
              window's best classes pays today, and the yardstick
  align       Aligner.align_features(feats, k=5): the same scoring and top-k, then the alignment of every clip against its five classes --
              1 280 pairs

The legs alternate three times (topk, align, topk, ...), every visit the median of `reps` calls after a warm-up call; a leg's figure is the
median of its three visits, and the spread of the topk leg's visits says what a difference is worth.  The alignment kernel is also timed
alone, on random rows: 1 280 pairs at T = 8 and at T = 32, both directions and one.  Nothing is asserted on time.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from _timing import _time_ms  # noqa: E402  (tools/_timing.py)
from shortlist_time import _head  # noqa: E402  (the same head)

G, NQ_G, T, K, FRAME, NOISE, BATCH = 32, 8, 8, 5, 0.5, 0.5, 1024


def end_to_end(head, C, reps, rounds=3):
    from clip_fsar_amd import gallery_hip as ghip
    from clip_fsar_amd.align import Aligner
    from clip_fsar_amd.live_gallery import LiveGallery
    live = LiveGallery(head, "cuda", capacity=C)
    E, N = live.E, G * NQ_G
    g = torch.Generator(device="cuda").manual_seed(C)
    base = torch.randn(E, device="cuda", generator=g)
    truth = torch.randperm(C, device="cuda", generator=g)[:G].tolist()       # the class every group's windows copy
    shots = torch.empty(G, T, E, device="cuda")
    for c0 in range(0, C, BATCH):                            # one shot per class, registered from features
        n = min(BATCH, C - c0)
        F = (base + torch.randn(n, 1, E, device="cuda", generator=g) + FRAME * torch.randn(n, T, E, device="cuda", generator=g)).contiguous()
        for i, c in enumerate(truth):
            if c0 <= c < c0 + n:
                shots[i] = F[c - c0]
        live.add_classes_features(F, list(range(c0, c0 + n)))
    feats = (shots[:, None] + NOISE * torch.randn(G, NQ_G, T, E, device="cuda", generator=g)).view(N, T, E).contiguous()
    al = Aligner(live)
    res = {}

    def topk():
        logits = live.classify_features(feats)
        values = torch.empty(N, K, device="cuda")
        index = torch.empty(N, K, device="cuda", dtype=torch.int32)
        ghip.topk(logits, K, values, index)
        res["topk"] = (values, index)

    def align():
        res["align"] = al.align_features(feats, k=K)

    legs = {"topk": topk, "align": align}
    visits = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            visits[k].append(_time_ms(fn, reps))
    ms = {k: statistics.median(v) for k, v in visits.items()}
    torch.cuda.synchronize()
    a = res["align"]
    same = torch.equal(a.pairs[:, 1].view(N, K), res["topk"][1])
    finite = bool(torch.isfinite(a.plan).all()) and bool(torch.isfinite(a.logits).all())
    top1 = float((res["topk"][1][:, 0].view(G, NQ_G) == torch.tensor(truth, device="cuda", dtype=torch.int32)[:, None]).float().mean())
    return {"classes": C, "windows": N, "T": T, "E": E, "k": K, "pairs": len(a),
            "topk_ms": round(ms["topk"], 4), "align_ms": round(ms["align"], 4), "align_minus_topk_ms": round(ms["align"] - ms["topk"], 4),
            "align_over_topk": round(ms["align"] / ms["topk"], 3),
            "topk_visit_spread": round((max(visits["topk"]) - min(visits["topk"])) / ms["topk"], 4),
            "visits_ms": {k: [round(t, 4) for t in v] for k, v in visits.items()},
            "align_classes_equal_topk_index": same, "plan_and_logits_finite": finite,
            "windows_whose_top1_is_the_copied_class": round(top1, 4)}


def kernel_alone(t, single_direct, reps, NP=G * NQ_G * K, NQ=G * NQ_G, cap=3200, E=512):
    from clip_fsar_amd import align_hip as ah
    g = torch.Generator(device="cuda").manual_seed(t)
    Xq = torch.randn(NQ, t, E, device="cuda", generator=g)
    P = torch.randn(cap, t, E, device="cuda", generator=g)
    qn, pn = Xq.norm(dim=-1).reshape(-1).contiguous(), P.norm(dim=-1).reshape(-1).contiguous()
    pair_q = (torch.arange(NP, device="cuda") // (NP // NQ)).to(torch.int32)
    pair_slot = torch.randint(0, cap, (NP,), device="cuda", generator=g).to(torch.int32)
    plan, dists, logits = torch.empty(NP, t, t, device="cuda"), torch.empty(NP, t, t, device="cuda"), torch.empty(NP, device="cuda")
    ms = _time_ms(lambda: ah.align(Xq, qn, P, pn, pair_q, pair_slot, 0.5, single_direct, plan, dists, logits), reps)
    torch.cuda.synchronize()
    return {"T": t, "E": E, "pairs": NP, "single_direct": bool(single_direct), "ms": round(ms, 4), "us_per_pair": round(1e3 * ms / NP, 4),
            "finite": bool(torch.isfinite(plan).all())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_time.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--classes", type=int, default=3200)
    args = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0), "reps": args.reps,
           "method": "one process; HIP events; median of `reps` timed calls after a warm-up call; the two legs alternating three times, a "
                     "leg's figure the median of its three visits; the kernel alone: one such median per point"}
    with torch.no_grad():
        out["end_to_end"] = end_to_end(_head(args.classes), args.classes, args.reps)
        print(json.dumps(out["end_to_end"]), flush=True)
        out["kernel_alone"] = [kernel_alone(t, sd, args.reps) for t in (8, 32) for sd in (False, True)]
        print(json.dumps(out["kernel_alone"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
