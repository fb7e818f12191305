"""Time one enrolment against one add_shots of the same clip on the GPU (run as a fresh process; HIP events around every call).

    python tools/enroll_time.py [--out profiles/enroll_time.json] [--reps 10] [--classes 2000]

ViT-B/16 bf16, T = 8, a LiveGallery of `classes` classes (registered from random tower features: what is timed does not depend on how
they came about).  A session pushes 16 frames through the tower, then the two legs teach class 7 a further shot from the session's newest
window:

  enroll     StreamPool.enroll(h, 7): the window's tower rows out of the ring (one cfen_ring_sequences launch), context2, the running sum,
             the norms -- the tower does not run
  add_shots  LiveGallery.add_shots(clip, [7]) with the same 8 frames resident on the device as fp32: the tower over them, then the same

The legs alternate three times (enroll, add_shots, enroll, ...), every visit the median of `reps` calls between HIP events after a warm-up
call; a leg's figure is the median of its three visits.  Nothing is asserted on time.
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


def measure(reps, n_classes, rounds=3, batch=100):
    from types import SimpleNamespace as NS
    import clip_fsar_amd.synth as synth
    from clip_fsar_amd.live_gallery import LiveGallery
    from clip_fsar_amd.models.base.few_shot import CNN_OTAM_CLIPFSAR
    from clip_fsar_amd.pool import StreamPool
    T, cid = 8, 7
    cfg = NS(VIDEO=NS(HEAD=NS(NAME="CNN_OTAM_CLIPFSAR", BACKBONE_NAME="ViT-B/16", PRECISION="bf16"), BACKBONE=NS(META_ARCH="Identity")),
             TRAIN=NS(CLASS_NAME=["c%d" % i for i in range(64)], WAY=5), TEST=NS(CLASS_NAME=["t%d" % i for i in range(n_classes + 8)]),
             DATA=NS(NUM_INPUT_FRAMES=T), MODEL=NS(NAME="BaseVideoModel", EMA=NS(ENABLE=False)), BN=NS(FREEZE=False), NUM_GPUS=1,
             NUM_SHARDS=1, RANDOM_SEED=18)
    head = CNN_OTAM_CLIPFSAR(cfg).eval()
    res = synth.ARCHS["ViT-B/16"]["res"]
    g = torch.Generator(device="cuda").manual_seed(1)
    with torch.no_grad():
        live = LiveGallery(head, "cuda", capacity=n_classes + 64)
        F = torch.randn(batch, T, live.E, device="cuda", generator=g)
        for c0 in range(0, n_classes, batch):
            n = min(batch, n_classes - c0)
            live.add_classes_features(F[:n], list(range(c0, c0 + n)))
        pool = StreamPool(live, max_streams=4, stride=1, max_push=16)
        h = pool.open()
        frames = torch.randn(2 * T, 3, res, res, device="cuda", generator=g)
        pool.push({h: frames})
        w = pool.enrolable(h)[-1]
        clip = frames[w:w + T][None].contiguous()              # the newest complete window's frames (stride 1, rate 1)
        legs = {"enroll": lambda: pool.enroll(h, cid), "add_shots": lambda: live.add_shots(clip, [cid])}
        visits = {k: [] for k in legs}
        for _ in range(rounds):
            for k, fn in legs.items():
                visits[k].append(_time_ms(fn, reps))
        torch.cuda.synchronize()
    ms = {k: statistics.median(v) for k, v in visits.items()}
    return {"arch": "ViT-B/16", "precision": "bf16", "T": T, "classes": n_classes, "window": w, "shots_of_the_class_at_the_end": live.shots(cid),
            "enroll_ms": round(ms["enroll"], 4), "add_shots_ms": round(ms["add_shots"], 4),
            "add_shots_over_enroll": round(ms["add_shots"] / ms["enroll"], 3),
            "visits_ms": {k: [round(t, 4) for t in v] for k, v in visits.items()},
            "visit_spread": {k: round((max(v) - min(v)) / ms[k], 4) for k, v in visits.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "enroll_time.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--classes", type=int, default=2000)
    args = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "rounds": 3, "shot": measure(args.reps, args.classes)}
    prior = os.path.join(ROOT, "profiles", "live_gallery_time.json")
    if os.path.exists(prior):                                  # the figure of the run that measured add_shots first, to set beside
        out["live_gallery_time_add_one_shot_ms"] = json.load(open(prior))["mutation"]["live_add_one_shot_ms"]
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
