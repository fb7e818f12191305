"""Time the event detector against the per-class smoothing launch it follows, and a pool tick with a rule against one without (one fresh
process; HIP events, medians after warm-up; run it under a time limit of its own: `timeout -k 10 600 python tools/events_time.py`).

    python tools/events_time.py [--out profiles/events_time.json] [--reps 10] [--session NAME]

32 sessions x 8 windows per push, 3 200 classes, T = 8 (ViT-B/16 head, bf16; the classes are registered from random tower features, one
shot each: the tower is not the subject).  Two comparisons, the two legs of each alternating three times in this one process:

  a. the call: cfev_detect (three launches: count, scan, emit) against cfcs_smooth_classes (one launch) on the same scores, table, keys and
     generations, 20 calls between two events, the tables uploaded before; the thresholds fire on under 1 % of the cells;
  b. the tick: StreamPool.push_features_packed in steady state, smooth_by="class", with an EventRule against without, over the same
     LiveGallery and the same features; the rule's thresholds are quantiles of the smoothed scores, again under 1 % of the cells.  The
     queue is drained by take_events() between the timed rounds, outside the timing.

Recorded: both medians of each comparison, the three alternations of every leg, the spread (max - min) of the leg without a rule, whether
the tick with a rule exceeds the tick without by more than that spread, the share of cells that fired, and the host time of take_events().
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
from class_smooth_time import build_gallery, summary  # noqa: E402  (tools/class_smooth_time.py: the same gallery and the same summary)

T, S, NW, C, ALPHA, LAUNCHES = 8, 32, 8, 3200, 0.5, 20


def alternate(legs, reps, rounds=3, after=None):
    """{name: fn} -> {name: [median ms of reps calls, per round]}, the legs taking turns; after(name) runs behind every timed round"""
    ts = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            ts[k].append(_time_ms(fn, reps))
            if after is not None:
                after(k)
    return ts


def call_point(reps):
    from clip_fsar_amd import class_smooth_hip as ch
    from clip_fsar_amd import events_hip as eh
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
    streak, length = (torch.zeros(S, cap, device="cuda", dtype=torch.int32) for _ in range(2))
    peak, ev_marks = torch.zeros(S, cap, device="cuda"), torch.ones(S, cap, device="cuda", dtype=torch.int32)
    max_events = 1 << 16
    events = torch.empty(max_events, eh.EVENT_COLS, device="cuda", dtype=torch.int32)
    values = torch.empty(max_events, eh.VALUE_COLS, device="cuda")
    n_events = torch.zeros(1, device="cuda", dtype=torch.int32)
    work = torch.empty(eh.workspace_ints(plan.n_chunks), device="cuda", dtype=torch.int32)
    on, off = 2.8, 2.3                                     # standard normal scores: s >= on in 0.26 % of the cells

    def smooth():
        for _ in range(LAUNCHES):
            ch.smooth_classes(x, state, marks, gens, keys, out, table, ALPHA)

    def detect():
        for _ in range(LAUNCHES):
            eh.detect(x, streak, length, peak, ev_marks, gens, keys, events, values, n_events, work, table, on, off, 1, 1)

    detect()
    fired = int(n_events.cpu()) / x.numel()
    ts = alternate({"cfcs_smooth_classes": smooth, "cfev_detect": detect}, reps)
    # what a call must move: the smoothing reads x and writes y of every window, its cell and mark, key and generation; the detector
    # reads the scores twice (count, emit) and the cell (12 bytes), mark, key and generation twice, writes cell and mark once and a
    # count per thread twice
    smooth_bytes, detect_bytes = S * C * (8 * NW + 8 + 16), S * C * (8 * NW + 2 * 24 + 16 + 8)
    return {"shape": {"sessions": S, "windows_per_session": NW, "classes": C, "store_slots": cap}, "calls_per_timed_call": LAUNCHES,
            "launches_per_call": {"cfcs_smooth_classes": 1, "cfev_detect": 3}, "per_call": summary(ts, LAUNCHES),
            "bytes_per_call": {"cfcs_smooth_classes": smooth_bytes, "cfev_detect": detect_bytes}, "workgroups": plan.n_chunks,
            "thresholds": {"on": on, "off": off, "min_on": 1, "min_off": 1}, "share_of_cells_with_a_record": round(fired, 5)}


def tick_point(live, reps):
    from clip_fsar_amd.events import EventRule
    from clip_fsar_amd.pool import StreamPool
    g = torch.Generator(device="cuda").manual_seed(2)
    feats = torch.randn(S * NW, live.E, device="cuda", generator=g)
    counts = [NW] * S

    def pool(rule):
        p = StreamPool(live, max_streams=S, stride=1, max_push=NW, smooth=ALPHA, smooth_by="class", events=rule)
        hs = [p.open() for _ in range(S)]
        p.push_features_packed(feats, hs, counts)          # the first push completes one window a session: steady state from the second
        return p, hs, p.push_features_packed(feats, hs, counts)

    plain, plain_hs, first = pool(None)
    on, off = (float(torch.quantile(first.smoothed.reshape(-1)[:1 << 22].float(), q)) for q in (0.997, 0.99))
    ruled, ruled_hs, again = pool(EventRule(on, off, 1, 1, max_events=1 << 16))
    assert torch.equal(first.logits, again.logits) and torch.equal(first.smoothed, again.smoothed)
    warm = ruled.take_events()
    legs = {"without_rule": lambda: plain.push_features_packed(feats, plain_hs, counts),
            "with_rule": lambda: ruled.push_features_packed(feats, ruled_hs, counts)}
    taken = []
    ts = alternate(legs, reps, after=lambda k: taken.append(len(ruled.take_events())) if k == "with_rule" else None)
    ruled.push_features_packed(feats, ruled_hs, counts)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    last = ruled.take_events()
    take_us = (time.perf_counter() - t0) * 1e6
    r = summary(ts)
    excess = r["with_rule"]["median_ms"] - r["without_rule"]["median_ms"]
    return {"windows_per_tick": S * NW, "tick": r, "with_minus_without_ms": round(excess, 5),
            "exceeds_the_spread_of_the_leg_without": bool(excess > r["without_rule"]["spread_ms"]),
            "thresholds": {"on": on, "off": off, "min_on": 1, "min_off": 1}, "events_of_the_warm_up_pushes": len(warm),
            "events_per_timed_round": taken, "events_of_one_steady_tick": len(last),
            "share_of_cells_with_an_event_in_one_steady_tick": round(len(last) / (S * NW * C), 5),
            "take_events_of_one_tick_host_us": round(take_us, 1), "events_dropped": ruled.stats()["events_dropped"],
            "outputs_bit_equal": True}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "events_time.json"))
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
