"""Time the contest against the per-class smoothing launch, and a pool tick with rule and contest against the tick with the rule alone;
count the events both report (one fresh process; HIP events, medians after warm-up; run it under a time limit of its own:
`timeout -k 10 600 python tools/contest_time.py`).

    python tools/contest_time.py [--out profiles/contest_time.json] [--reps 10] [--session NAME]

32 sessions x 8 windows per push, 3 200 classes, T = 8 (ViT-B/16 head, bf16; the classes are registered from random tower features, one
shot each: the tower is not the subject).  Two comparisons, the legs of each alternating three times in this one process:

  a. the call: cfct_contest (one launch, a workgroup per window) against cfcs_smooth_classes (one launch) on the same scores, table and
     keys, 20 calls between two events, the tables uploaded before -- the yardstick tools/events_time.py and tools/baseline_time.py
     use; at top = 1 and top = 3, without and with leader lists;
  b. the tick: StreamPool.push_features_packed in steady state with an EventRule and a Contest against the rule alone, over the same
     LiveGallery and the same features; the rule is the one of tools/evidence_time.py -- the 0.9995 / 0.999 quantiles of one tick's
     logits, min_on = min_off = 1 -- at top = 1 and top = 3.  The queue is drained by take_events() between the timed rounds, outside
     the timing.

Recorded: the medians of each comparison, the three alternations of every leg, the spread (max - min) of the leg with the rule alone,
whether a tick with the contest exceeds it by more than that spread, and the events of one steady tick of every leg -- that count is the
point of the feature.  Nothing is asserted on time.
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
from events_time import ALPHA, LAUNCHES, NW, C, S, T, alternate  # noqa: E402  (tools/events_time.py: the same shape and alternation)

TOPS = (1, 3)


def call_point(reps):
    from clip_fsar_amd import class_smooth_hip as ch
    from clip_fsar_amd import contest_hip as ct
    g = torch.Generator(device="cuda").manual_seed(3)
    x = torch.randn(S * NW * C, device="cuda", generator=g)
    out = torch.empty_like(x)
    cap = C + 64
    state = torch.zeros(S, cap, device="cuda")
    marks = torch.ones(S, cap, device="cuda", dtype=torch.int32)                  # every cell valid: the smoothing reads its state
    gens = torch.ones(cap, device="cuda", dtype=torch.int32)
    keys = torch.randperm(cap, device="cuda", generator=g)[:C].to(torch.int32)
    plan = ch.plan_rows(list(range(S)), [NW] * S, [None] * S, C)
    table = ch.table_uploader("cuda", S).upload(plan.rows)
    work = torch.empty(ct.workspace_words(x.numel()), device="cuda", dtype=torch.int32)
    leaders = {top: (torch.empty(S * NW, top, device="cuda", dtype=torch.int32), torch.empty(S * NW, device="cuda", dtype=torch.int32))
               for top in TOPS}

    def smooth():
        for _ in range(LAUNCHES):
            ch.smooth_classes(x, state, marks, gens, keys, out, table, ALPHA)

    def contest(top, lists):
        def run():
            for _ in range(LAUNCHES):
                ct.contest(x, keys, out, *(leaders[top] if lists else (None, None)), work, table, cap, top, None)
        return run

    legs = {"cfcs_smooth_classes": smooth}
    for top in TOPS:
        legs["cfct_contest_top%d" % top] = contest(top, False)
        legs["cfct_contest_top%d_with_leaders" % top] = contest(top, True)
    ts = alternate(legs, reps)
    demoted = int(torch.isneginf(out).sum())               # of the last leg: top = 3 with lists
    # what a call must move: the smoothing reads x and writes y of every window, its cell and mark, key and generation; the contest
    # reads x three times (keys, plane, leaders' own) and the row's keys five times (four passes and the scan; L2 serves them), and
    # writes the keys and the plane once
    smooth_bytes, contest_bytes = S * C * (8 * NW + 8 + 16), S * NW * C * (4 + 4 + 4)
    return {"shape": {"sessions": S, "windows_per_session": NW, "classes": C, "store_slots": cap}, "calls_per_timed_call": LAUNCHES,
            "launches_per_call": {"cfcs_smooth_classes": 1, "cfct_contest": 1}, "per_call": summary(ts, LAUNCHES),
            "bytes_per_call_from_hbm": {"cfcs_smooth_classes": smooth_bytes, "cfct_contest": contest_bytes}, "workgroups": S * NW,
            "cells_demoted_at_top3": demoted, "cells": x.numel()}


def tick_point(live, reps):
    from clip_fsar_amd.contest import Contest
    from clip_fsar_amd.events import EventRule
    from clip_fsar_amd.pool import StreamPool
    g = torch.Generator(device="cuda").manual_seed(2)
    feats = torch.randn(S * NW, live.E, device="cuda", generator=g)
    counts = [NW] * S

    def pool(**kw):
        p = StreamPool(live, max_streams=S, stride=1, max_push=NW, **kw)
        hs = [p.open() for _ in range(S)]
        p.push_features_packed(feats, hs, counts)          # the first push completes one window a session: steady state from the second
        return p, hs, p.push_features_packed(feats, hs, counts)

    first = pool()[2]
    on, off = (float(torch.quantile(first.logits.view(-1).float().cpu(), q)) for q in (0.9995, 0.999))
    rule = EventRule(on, off, 1, 1, max_events=1 << 16)
    pools = {"rule_alone": pool(events=rule)}
    for top in TOPS:
        pools["contest_top%d" % top] = pool(events=rule, contest=Contest(top=top))
    for p, _, again in pools.values():
        assert torch.equal(first.logits, again.logits)
        p.take_events()
    legs = {k: (lambda p=p, hs=hs: p.push_features_packed(feats, hs, counts)) for k, (p, hs, _) in pools.items()}
    taken = {k: [] for k in pools}
    ts = alternate(legs, reps, after=lambda k: taken[k].append(len(pools[k][0].take_events())))
    steady = {}
    for k, (p, hs, _) in pools.items():
        p.push_features_packed(feats, hs, counts)
        steady[k] = len(p.take_events())
    r = summary(ts)
    base = r["rule_alone"]
    return {"windows_per_tick": S * NW, "tick": r,
            "contest_minus_rule_alone_ms": {k: round(v["median_ms"] - base["median_ms"], 5) for k, v in r.items() if k != "rule_alone"},
            "exceeds_the_spread_of_the_leg_with_the_rule_alone": {k: bool(v["median_ms"] - base["median_ms"] > base["spread_ms"])
                                                                  for k, v in r.items() if k != "rule_alone"},
            "thresholds": {"on": on, "off": off, "min_on": 1, "min_off": 1}, "events_per_timed_round": taken,
            "events_of_one_steady_tick": steady, "events_dropped": {k: p.stats()["events_dropped"] for k, (p, _, _) in pools.items()},
            "outputs_bit_equal": True}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "contest_time.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--session", default=time.strftime("%Y-%m-%d %H:%M:%S"), help="label of the measuring session, stored in the JSON")
    args = ap.parse_args()
    with torch.no_grad():
        out = {"device": torch.cuda.get_device_name(0), "session": args.session,
               "method": "one process; HIP events; median of %d timed calls after a warm-up call; the legs of each comparison "
                         "alternating three times; spread = max - min of a leg's three medians" % args.reps,
               "arch": "ViT-B/16", "precision": "bf16", "T": T}
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
