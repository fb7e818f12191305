"""Time two-stage scoring on the GPU and measure its recall (run as a fresh process; HIP events around every leg).

    python tools/shortlist_time.py [--out profiles/shortlist_time.json] [--reps 10] [--classes 3200 25600]

32 groups of 8 windows (the windows of one stream share a shortlist), T = 8, E = 512 (ViT-B/16 head, bf16 tower -- the tower does not run:
the legs start from tower features), keep = 64, against a LiveGallery of 3 200 and of 25 600 classes of one shot each.  Two ways to a
window's best classes:

  full        LiveGallery.classify_features over all classes: [256, C] logits
  shortlist   Shortlist.classify_features(counts=[8] * 32): [256, 64] logits and [32, 64] columns

The legs alternate three times (full, shortlist, full, ...), every visit the median of `reps` calls after a warm-up call; a leg's figure is
the median of its three visits, and the spread of the full leg's visits says what a ratio is worth.  The stages of the shortlist leg are
timed the same way, one after the other on the leg's own intermediate results: context2 + norms, the coarse rows and scores (no slot is
stale: the refresh is bookkeeping alone), the selection, the grouped OTAM launch.

Recall on a synthetic gallery: a class is one shot of tower features -- a direction all classes share, the class's own direction and
0.5 of frame noise, so that the frames of a shot resemble each other as a video's do --, and a group's 8 windows are copies of one
class's shot with 0.5 of noise on every value.  Per class count: the share of groups, and of windows, whose full-OTAM
top-1 and top-5 lie inside the group's shortlist.  Nothing is asserted on time or on recall.
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

G, NQ_G, T, KEEP, FRAME, NOISE, BATCH = 32, 8, 8, 64, 0.5, 0.5, 1024


def _head(n_test):
    from types import SimpleNamespace as NS
    from clip_fsar_amd.models.base.few_shot import CNN_OTAM_CLIPFSAR
    cfg = NS(VIDEO=NS(HEAD=NS(NAME="CNN_OTAM_CLIPFSAR", BACKBONE_NAME="ViT-B/16", PRECISION="bf16"), BACKBONE=NS(META_ARCH="Identity")),
             TRAIN=NS(CLASS_NAME=["c%d" % i for i in range(64)], WAY=5), TEST=NS(CLASS_NAME=["t%d" % i for i in range(n_test)]),
             DATA=NS(NUM_INPUT_FRAMES=T), MODEL=NS(NAME="BaseVideoModel", EMA=NS(ENABLE=False)), BN=NS(FREEZE=False), NUM_GPUS=1,
             NUM_SHARDS=1, RANDOM_SEED=18)
    return CNN_OTAM_CLIPFSAR(cfg).eval()


def point(head, C, reps, rounds=3):
    from clip_fsar_amd.live_gallery import LiveGallery
    from clip_fsar_amd.shortlist import NONE, Shortlist
    live = LiveGallery(head, "cuda", capacity=C)
    E = live.E
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
    feats = (shots[:, None] + NOISE * torch.randn(G, NQ_G, T, E, device="cuda", generator=g)).view(G * NQ_G, T, E).contiguous()
    counts = [NQ_G] * G
    sl = Shortlist(live, keep=KEEP)
    res = {}

    def full():
        res["full"] = live.classify_features(feats)

    def short():
        res["short"] = sl.classify_features(feats, counts=counts)

    legs = {"full": full, "shortlist": short}
    visits = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            visits[k].append(_time_ms(fn, reps))
    ms = {k: statistics.median(v) for k, v in visits.items()}
    # the stages, on the leg's own intermediate results
    eng = live._fresh_engine()
    slots = [live.slot_of(c) for c in live.class_ids]
    cols = live._columns(None)
    st = {}
    stages = {"context2_and_norms": lambda: st.update(q=sl._queries(eng, feats, False)),
              "coarse_rows_and_scores": lambda: st.update(S=sl._coarse_scores(st["q"][0], st["q"][1], sl._stale(slots), cols)),
              "select": lambda: st.update(sel=sl._select(st["S"], cols, counts, KEEP)),
              "grouped_otam": lambda: st.update(out=sl._exact(st["q"][0], st["q"][1], st["sel"][1], counts, KEEP))}
    stage_ms = {k: round(_time_ms(fn, reps), 4) for k, fn in stages.items()}
    torch.cuda.synchronize()
    # recall: the full-OTAM top-1 / top-5 of every window against its group's shortlist
    full_l, r = res["full"], res["short"]
    top5 = full_l.topk(5, dim=1).indices.view(G, NQ_G, 5)
    listed = torch.zeros(G, C + 1, dtype=torch.bool, device="cuda")
    listed.scatter_(1, r.columns.long().clamp(max=C), True)
    hit = torch.gather(listed[:, None, :].expand(G, NQ_G, C + 1), 2, top5)                  # [G, NQ_G, 5]
    in1, in5 = hit[:, :, 0], hit.all(2)
    true_top1 = float((top5[:, :, 0] == torch.tensor(truth, device="cuda")[:, None]).float().mean())
    return {"classes": C, "groups": G, "windows_per_group": NQ_G, "T": T, "E": E, "keep": KEEP, "query_noise": NOISE,
            "full_ms": round(ms["full"], 4), "shortlist_ms": round(ms["shortlist"], 4),
            "full_over_shortlist": round(ms["full"] / ms["shortlist"], 3),
            "full_visit_spread": round((max(visits["full"]) - min(visits["full"])) / ms["full"], 4),
            "visits_ms": {k: [round(t, 4) for t in v] for k, v in visits.items()}, "stages_ms": stage_ms,
            "coarse_rows_refreshed": sl.stats["refreshed"], "padded_places": int((r.columns == NONE).sum()),
            "recall": {"groups_top1_in_shortlist": round(float(in1.all(1).float().mean()), 4),
                       "groups_top5_in_shortlist": round(float(in5.all(1).float().mean()), 4),
                       "windows_top1_in_shortlist": round(float(in1.float().mean()), 4),
                       "windows_top5_in_shortlist": round(float(in5.float().mean()), 4),
                       "windows_whose_full_top1_is_the_copied_class": round(true_top1, 4)}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shortlist_time.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--classes", type=int, nargs="+", default=[3200, 25600])
    args = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "points": []}
    with torch.no_grad():
        head = _head(max(args.classes))
        for C in args.classes:
            p = point(head, C, args.reps)
            print(json.dumps(p), flush=True)
            out["points"].append(p)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
