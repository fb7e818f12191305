"""Time a stream pool's tick with event evidence on the GPU (run as a fresh process; HIP events around every leg).

    python tools/evidence_time.py [--out profiles/evidence_time.json] [--reps 10] [--classes 3200]

One tick is one push_features_packed: 32 sessions pushing 8 frames each at stride 1, so every session completes 8 windows -- 256 windows,
T = 8, E = 512 (ViT-B/16 head, bf16 tower -- the tower does not run: the legs start from tower features), against a LiveGallery of
3 200 classes of one shot each, with an EventRule whose thresholds are the 0.9995 and 0.999 quantiles of one tick's logits (min_on =
min_off = 1), so that every tick reports some hundreds of onsets and offsets out of its 819 200 cells.  Two legs, both pools warmed past
their first window before anything is timed:

  rule        StreamPool(events=rule): the code path of the pool without the option, and the yardstick
  evidence    StreamPool(events=rule, evidence=Evidence(256, ("onset", "offset"))): the same tick with the capture behind the detector

The legs alternate three times (rule, evidence, rule, ...), every visit the median of `reps` ticks after a warm-up tick; a leg's figure is
the median of its three visits, and the spread of a leg's visits says what a difference is worth.  Neither leg reads its events inside
the timed region: the 34 pushes of a pool stay below the queue's 64.  cfed_capture is also timed alone at the tick's
shape, max_events = 4 096: with n_events = 0 -- the placement pass over every record slot and a copy pass that finds no descriptor --
and with 256 qualifying records into a store of 256 slots, whose 2 * 256 * T * E * 4 bytes over the call's time, its two launches
included, are quoted as a rate.  Nothing is asserted on time.
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
from tempo_time import NW_S, STRIDE, S, T, _gallery  # noqa: E402  (the same gallery and tick)

CAPACITY, MAX_EVENTS = 256, 4096


def ticks(head, C, reps, rounds=3):
    from clip_fsar_amd.events import EventRule
    from clip_fsar_amd.evidence import Evidence
    from clip_fsar_amd.pool import StreamPool
    live = _gallery(head, C)
    g = torch.Generator(device="cuda").manual_seed(C + 1)
    n = NW_S * STRIDE                                        # frames per session and tick: 8 windows each once a session is warm
    feats = [torch.randn(S * n, live.E, device="cuda", generator=g) for _ in range(4)]       # the ticks differ, so that scores cross the thresholds
    counts = [n] * S

    def pool(**kw):
        p = StreamPool(live, max_streams=S, stride=STRIDE, max_push=n, **kw)
        hs = [p.open() for _ in range(S)]
        for i in range(-(-(T - 1) // n) + 1):                # past every session's first window
            out = p.push_features_packed(feats[i % 4], hs, counts)
        return p, hs, out

    _, _, out = pool()
    on, off = (float(torch.quantile(out.logits.view(-1).float().cpu(), q)) for q in (0.9995, 0.999))
    rule = EventRule(on, off, 1, 1, max_events=MAX_EVENTS)
    plain, plain_h, _ = pool(events=rule)
    kept, kept_h, _ = pool(events=rule, evidence=Evidence(CAPACITY, ("onset", "offset")))
    res, turn = {}, {"rule": 0, "evidence": 0}

    def leg(name, p, hs):
        def fn():
            turn[name] += 1
            res[name] = p.push_features_packed(feats[turn[name] % 4], hs, counts)
        return fn

    legs = {"rule": leg("rule", plain, plain_h), "evidence": leg("evidence", kept, kept_h)}
    visits = {k: [] for k in legs}
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)     # records beyond max_events are dropped in both legs alike
        for _ in range(rounds):
            for k, fn in legs.items():
                visits[k].append(_time_ms(fn, reps))
        ms = {k: statistics.median(v) for k, v in visits.items()}
        torch.cuda.synchronize()
        a, b = plain.take_events(), kept.take_events()
    spread = {k: round((max(v) - min(v)) / ms[k], 4) for k, v in visits.items()}
    stats = kept.stats()
    return {"classes": C, "sessions": S, "windows": res["evidence"].logits.shape[0], "T": T, "E": live.E, "stride": STRIDE,
            "capacity": CAPACITY, "max_events": MAX_EVENTS, "rule_ms": round(ms["rule"], 4), "evidence_ms": round(ms["evidence"], 4),
            "evidence_over_rule": round(ms["evidence"] / ms["rule"], 4), "visit_spread": spread,
            "visits_ms": {k: [round(t, 4) for t in v] for k, v in visits.items()},
            "events_equal": [tuple(e[:8]) for e in b] == [tuple(e) for e in a], "events": stats["events"],
            "events_dropped": stats["events_dropped"], "captured": stats["evidence"], "missed": stats["evidence_missed"],
            "logits_equal": bool(torch.equal(res["rule"].logits, res["evidence"].logits))}


def capture_alone(reps, E=512):
    from clip_fsar_amd import evidence_hip as eh
    cap = (T - 1) + NW_S * STRIDE
    g = torch.Generator(device="cuda").manual_seed(7)
    ring = torch.randn(S, cap, E, device="cuda", generator=g)
    table = eh.table_uploader("cuda", S).upload([[s, 0, NW_S, 0, s * NW_S * 4, 4] for s in range(S)])
    events = torch.tensor([[i % S, i % 4, (i // S) % NW_S, 1, 1] for i in range(MAX_EVENTS)], dtype=torch.int32, device="cuda")
    n = torch.zeros(1, dtype=torch.int32, device="cuda")
    store = torch.zeros(CAPACITY, T, E, device="cuda")
    head = torch.zeros(1, dtype=torch.int32, device="cuda")
    where = torch.empty(MAX_EVENTS, 2, dtype=torch.int32, device="cuda")
    work = torch.empty(eh.workspace_ints(CAPACITY), dtype=torch.int32, device="cuda")
    call = lambda: eh.capture(ring, events, n, None, store, head, where, work, table, 1, STRIDE, 1)
    idle_ms = _time_ms(call, reps)
    n.fill_(CAPACITY)
    full_ms = _time_ms(call, reps)
    torch.cuda.synchronize()
    moved = 2 * CAPACITY * T * E * 4
    return {"max_events": MAX_EVENTS, "capacity": CAPACITY, "T": T, "E": E, "no_records_ms": round(idle_ms, 4),
            "captures_256_ms": round(full_ms, 4), "copy_bytes": moved,
            "captures_256_GBps_launches_included": round(moved / full_ms / 1e6, 1),
            "all_captured": bool((where[:CAPACITY, 0] >= 0).all()) and bool((where[CAPACITY:, 0] == -1).all())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "evidence_time.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--classes", type=int, default=3200)
    args = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0), "reps": args.reps,
           "method": "one process; HIP events; median of `reps` timed ticks after a warm-up tick; the two legs alternating three times, a "
                     "leg's figure the median of its three visits; cfed_capture alone: one such median each, both launches included"}
    with torch.no_grad():
        out["tick"] = ticks(_head(args.classes), args.classes, args.reps)
        print(json.dumps(out["tick"]), flush=True)
        out["capture_alone"] = capture_alone(args.reps)
        print(json.dumps(out["capture_alone"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
