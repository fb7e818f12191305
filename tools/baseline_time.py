"""Time the baseline launch against the per-class smoothing launch it follows, and a pool tick with a baseline against one without (one
fresh process; HIP events, medians after warm-up; run it under a time limit of its own: `timeout -k 10 600 python tools/baseline_time.py`).

    python tools/baseline_time.py [--out profiles/baseline_time.json] [--reps 10] [--session NAME]

32 sessions x 8 windows per push, 3 200 classes, T = 8 (ViT-B/16 head, bf16; the classes are registered from random tower features, one
shot each: the tower is not the subject).  Two comparisons, the two legs of each alternating three times in this one process:

  a. the call: cfbl_normalize against cfcs_smooth_classes (one launch each) on the same scores, table, keys and generations, 20 calls
     between two events, the tables uploaded before; every cell is valid and past its warm-up, so every window is judged, and the scores
     are standard normal, so a window is gated now and then;
  b. the tick: StreamPool.push_features_packed in steady state, smooth_by="class", with a Baseline against without, over the same
     LiveGallery and the same features.

Recorded: both medians of each comparison, the three alternations of every leg, the spread (max - min) of the leg without a baseline,
whether the tick with a baseline exceeds the tick without by more than that spread, and the share of windows past warm-up and gated.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from class_smooth_time import build_gallery, summary  # noqa: E402  (tools/class_smooth_time.py: the same gallery and the same summary)
from events_time import alternate  # noqa: E402  (tools/events_time.py: the legs taking turns)

T, S, NW, C, ALPHA, LAUNCHES = 8, 32, 8, 3200, 0.5, 20
RULE = dict(rate=1 / 32, warm_rate=0.25, warmup=16, gate=3.0, floor=1e-6)


def call_point(reps):
    from clip_fsar_amd import baseline_hip as bh
    from clip_fsar_amd import class_smooth_hip as ch
    g = torch.Generator(device="cuda").manual_seed(3)
    x = torch.randn(S * NW * C, device="cuda", generator=g)
    out = torch.empty_like(x)
    cap = C + 64
    state = torch.zeros(S, cap, device="cuda")
    marks = torch.ones(S, cap, device="cuda", dtype=torch.int32)                  # every cell valid: both read their state
    gens = torch.ones(cap, device="cuda", dtype=torch.int32)
    keys = torch.randperm(cap, device="cuda", generator=g)[:C].to(torch.int32)
    plan = ch.plan_rows(list(range(S)), [NW] * S, [None] * S, C)
    table = ch.table_uploader("cuda", S).upload(plan.rows)
    mean = torch.zeros(S, cap, device="cuda")
    dev = torch.full((S, cap), 0.8, device="cuda")                                 # the mean absolute deviation of a standard normal
    count = torch.full((S, cap), RULE["warmup"], device="cuda", dtype=torch.int32)
    bl_marks = torch.ones(S, cap, device="cuda", dtype=torch.int32)
    z = torch.empty_like(x)
    rule = tuple(RULE.values())

    def smooth():
        for _ in range(LAUNCHES):
            ch.smooth_classes(x, state, marks, gens, keys, out, table, ALPHA)

    def normalize():
        for _ in range(LAUNCHES):
            bh.normalize(x, mean, dev, count, bl_marks, gens, keys, z, table, *rule)

    normalize()
    judged, gated = float((~z.isnan()).float().mean()), float((z >= RULE["gate"]).float().mean())
    ts = alternate({"cfcs_smooth_classes": smooth, "cfbl_normalize": normalize}, reps)
    # what a call must move: both read x and write one value of every window, and read key and generation; the smoothing reads and
    # writes its cell (4 bytes) and mark, the baseline its cell (12 bytes) and mark
    smooth_bytes, base_bytes = S * C * (8 * NW + 8 + 16), S * C * (8 * NW + 8 + 32)
    return {"shape": {"sessions": S, "windows_per_session": NW, "classes": C, "store_slots": cap}, "calls_per_timed_call": LAUNCHES,
            "launches_per_call": {"cfcs_smooth_classes": 1, "cfbl_normalize": 1}, "per_call": summary(ts, LAUNCHES),
            "bytes_per_call": {"cfcs_smooth_classes": smooth_bytes, "cfbl_normalize": base_bytes},
            "state_bytes_per_call": {"cfcs_smooth_classes": S * C * 16, "cfbl_normalize": S * C * 32}, "workgroups": plan.n_chunks,
            "baseline": RULE, "share_of_windows_judged": round(judged, 5), "share_of_windows_gated": round(gated, 5)}


def tick_point(live, reps):
    from clip_fsar_amd.baseline import Baseline
    from clip_fsar_amd.pool import StreamPool
    g = torch.Generator(device="cuda").manual_seed(2)
    feats = torch.randn(S * NW, live.E, device="cuda", generator=g)
    counts = [NW] * S

    def pool(base):
        p = StreamPool(live, max_streams=S, stride=1, max_push=NW, smooth=ALPHA, smooth_by="class", baseline=base)
        hs = [p.open() for _ in range(S)]
        p.push_features_packed(feats, hs, counts)          # the first push completes one window a session: steady state from the second
        for _ in range(2):                                 # 1 + 8 + 8 windows a pair: past the warm-up of 16
            out = p.push_features_packed(feats, hs, counts)
        return p, hs, out

    plain, plain_hs, first = pool(None)
    based, based_hs, again = pool(Baseline(**RULE))
    assert torch.equal(first.logits, again.logits) and torch.equal(first.smoothed, again.smoothed)
    legs = {"without_baseline": lambda: plain.push_features_packed(feats, plain_hs, counts),
            "with_baseline": lambda: based.push_features_packed(feats, based_hs, counts)}
    ts = alternate(legs, reps)
    z = based.push_features_packed(feats, based_hs, counts).deviation
    r = summary(ts)
    excess = r["with_baseline"]["median_ms"] - r["without_baseline"]["median_ms"]
    return {"windows_per_tick": S * NW, "tick": r, "with_minus_without_ms": round(excess, 5),
            "exceeds_the_spread_of_the_leg_without": bool(excess > r["without_baseline"]["spread_ms"]), "baseline": RULE,
            "share_of_windows_judged_in_one_steady_tick": round(float((~z.isnan()).float().mean()), 5),
            "share_of_windows_gated_in_one_steady_tick": round(float((z >= RULE["gate"]).float().mean()), 5),
            "cells_of_one_session": len(based.baseline(based_hs[0])), "outputs_bit_equal": True}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "baseline_time.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--session", default=time.strftime("%Y-%m-%d %H:%M:%S"), help="label of the measuring session, stored in the JSON")
    args = ap.parse_args()
    with torch.no_grad():
        out = {"device": torch.cuda.get_device_name(0), "session": args.session,
               "method": "one process; HIP events; median of %d timed calls after a warm-up call; the two legs of each comparison "
                         "alternating three times; spread = max - min of a leg's three medians" % args.reps,
               "arch": "ViT-B/16", "precision": "bf16", "T": T, "alpha": ALPHA}
        out["call"] = call_point(args.reps)
        print(json.dumps(out["call"]), flush=True)
        out["tick"] = tick_point(build_gallery(), args.reps)
        print(json.dumps(out["tick"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
