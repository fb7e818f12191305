"""Time what StreamPool(timeline=) costs a push, cftl_fold against the launch that reads the same plane, and a recall (one fresh process;
HIP events, medians after warm-up; run it under a time limit of its own: `timeout -k 10 600 python tools/timeline_time.py`).

    python tools/timeline_time.py [--out profiles/timeline_time.json] [--reps 10] [--session NAME]

ViT-B/16 head, bf16, T = 8, 3 200 classes registered from random tower features (tools/class_smooth_time.py's gallery: the tower is not
the subject).  Three comparisons, the legs of each alternating three times in this one process:

  a. the fold: cftl_fold alone at 32 sessions x 8 windows x 3 200 classes into cells [32, 256, 3 264] (span = 16, a level), 20 calls
     between two events, against cfcs_smooth_classes on the same table, keys and scores -- the yardstick reads the same plane and writes
     one as large, the fold reads it and writes a cell per column;
  b. the tick: StreamPool.push_features_packed in steady state, 32 sessions x 8 windows per push, with timeline=Timeline(16, 256, level)
     against the same pool without the option, over the same gallery and features;
  c. the recall: recall() of 4 classes over 32 sessions x 256 held buckets, top = 16, whole (with its one synchronisation), and its
     cftl_read and cfhs_peaks on their own over the same table and buffers.  The buckets are filled at span = 1, 256 windows a session:
     what a recall costs depends on the buckets it scans, not on the windows behind them.

Recorded: the medians of each comparison, the three alternations of every leg, the spread (max - min) of the leg without the option and
whether the difference exceeds that spread.  Nothing is asserted on time.
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

SPAN, BUCKETS, LEVEL, CLASSES, TOP = 16, 256, 0.0, (7, 100, 1500, 3199), 16


def fold_point(reps):
    from clip_fsar_amd import class_smooth_hip as ch
    from clip_fsar_amd import timeline_hip as th
    from clip_fsar_amd.pool_hip import TableUploader
    g = torch.Generator(device="cuda").manual_seed(3)
    x = torch.randn(S * NW * C, device="cuda", generator=g)
    out = torch.empty_like(x)
    cap = C + 64
    plan = ch.plan_rows(list(range(S)), [NW] * S, [None] * S, C)
    keys = torch.arange(C, device="cuda", dtype=torch.int32)
    gens = torch.ones(cap, device="cuda", dtype=torch.int32)
    table = ch.table_uploader("cuda", S).upload(plan.rows)
    state, marks = torch.zeros(S, cap, device="cuda"), torch.ones(S, cap, device="cuda", dtype=torch.int32)
    cells = (torch.zeros(S, BUCKETS, cap, device="cuda"), torch.zeros(S, BUCKETS, cap, device="cuda", dtype=torch.int32),
             torch.zeros(S, BUCKETS, cap, device="cuda", dtype=torch.int32), torch.ones(S, BUCKETS, cap, device="cuda", dtype=torch.int32))
    f = TableUploader("cuda", S, cols=1).upload([[SPAN * 3 + 4]] * S)          # every row's 8 windows inside one bucket: a cell per column
    first = th.Table(f.host.view(-1), f.dev.view(-1), S)
    f = TableUploader("cuda", S, cols=1).upload([[SPAN * 3 + 12]] * S)         # and across a bucket boundary: two cells per column
    across = th.Table(f.host.view(-1), f.dev.view(-1), S)

    def smooth():
        for _ in range(LAUNCHES):
            ch.smooth_classes(x, state, marks, gens, keys, out, table, ALPHA)

    def fold(where):
        def run():
            for _ in range(LAUNCHES):
                th.fold(x, *cells, gens, keys, table, where, SPAN, LEVEL)
        return run

    r = summary(alternate({"cfcs_smooth_classes": smooth, "cftl_fold": fold(first), "cftl_fold_across_a_bucket": fold(across)}, reps), LAUNCHES)
    base = r["cfcs_smooth_classes"]
    return {"sessions": S, "windows": NW, "classes": C, "span": SPAN, "buckets": BUCKETS, "cells_bytes": sum(t.numel() * 4 for t in cells),
            "plane_bytes": x.numel() * 4, "launches_per_timed_call": LAUNCHES, "fold": r,
            "fold_over_smooth": round(r["cftl_fold"]["median_ms"] / base["median_ms"], 3),
            "fold_minus_smooth_ms": round(r["cftl_fold"]["median_ms"] - base["median_ms"], 5),
            "exceeds_the_spread_of_the_yardstick": bool(abs(r["cftl_fold"]["median_ms"] - base["median_ms"]) > base["spread_ms"])}


def tick_point(live, reps):
    from clip_fsar_amd.pool import StreamPool
    from clip_fsar_amd.timeline import Timeline
    g = torch.Generator(device="cuda").manual_seed(2)
    feats = torch.randn(S * NW, live.E, device="cuda", generator=g)
    counts = [NW] * S

    def pool(**kw):
        p = StreamPool(live, max_streams=S, stride=1, max_push=NW, **kw)
        hs = [p.open() for _ in range(S)]
        p.push_features_packed(feats, hs, counts)          # the first push completes one window a session: steady state from the second
        return p, hs, p.push_features_packed(feats, hs, counts)

    pools = {"without_timeline": pool(), "with_timeline": pool(timeline=Timeline(SPAN, BUCKETS, LEVEL))}
    assert torch.equal(pools["without_timeline"][2].logits, pools["with_timeline"][2].logits)
    legs = {k: (lambda p=p, hs=hs: p.push_features_packed(feats, hs, counts)) for k, (p, hs, _) in pools.items()}
    r = summary(alternate(legs, reps))
    base = r["without_timeline"]
    return {"windows_per_tick": S * NW, "classes": len(live), "tick": r,
            "timeline_minus_plain_ms": round(r["with_timeline"]["median_ms"] - base["median_ms"], 5),
            "exceeds_the_spread_of_the_leg_without_timeline": bool(r["with_timeline"]["median_ms"] - base["median_ms"] > base["spread_ms"]),
            "uploads_per_tick": 1, "outputs_bit_equal": True}


def recall_point(live, reps):
    from clip_fsar_amd import history_hip as hh
    from clip_fsar_amd import timeline_hip as th
    from clip_fsar_amd.pool import StreamPool
    from clip_fsar_amd.pool_hip import TableUploader
    from clip_fsar_amd.timeline import Timeline, read_rows
    ids = list(CLASSES)
    K = len(ids)
    p = StreamPool(live, max_streams=S, stride=1, max_push=64, timeline=Timeline(1, BUCKETS, LEVEL))
    hs = [p.open() for _ in range(S)]
    g = torch.Generator(device="cuda").manual_seed(4)
    for n in (T - 1 + 64, 64, 64, 64):                     # 256 windows a session: every bucket of the ring is filled by ordinary pushes
        p.push_features_packed(torch.randn(S * n, live.E, device="cuda", generator=g), hs, [n] * S)
    res = p.recall(ids, top=TOP)
    NB = res.buckets
    assert NB == S * BUCKETS and all(len(v) == TOP for v in res.hits.values())
    gens = live.slot_generations()
    keys = torch.tensor([live.slot_of(c) for c in ids], device="cuda", dtype=torch.int32)
    rows, n_out = read_rows(list(range(S)), [range(0, BUCKETS)] * S, [K] * S, [0] * S)
    rtable = th.read_uploader("cuda", S).upload(rows)
    ptable = TableUploader("cuda", S).upload([[s, 0, 0, 0, 0, BUCKETS, s * BUCKETS, 0] for s in range(S)])
    peak = torch.empty(NB, K, device="cuda")
    at, above = (torch.empty(NB, K, device="cuda", dtype=torch.int32) for _ in range(2))
    work = torch.empty(hh.workspace_words(NB, K), device="cuda", dtype=torch.int32)
    hrows, vals = torch.empty(K, TOP, device="cuda", dtype=torch.int32), torch.empty(K, TOP, device="cuda")
    n_hits, n_peaks = (torch.empty(K, device="cuda", dtype=torch.int32) for _ in range(2))
    cells = p._tl_cells.planes
    legs = {"recall": lambda: p.recall(ids, top=TOP),
            "cftl_read": lambda: th.read(*cells, gens, keys, peak.view(-1), at.view(-1), above.view(-1), rtable, 1),
            "cfhs_peaks": lambda: hh.peaks(peak, work, hrows, vals, n_hits, n_peaks, ptable, 1, None, TOP)}
    r = summary(alternate(legs, reps))
    return {"sessions": S, "buckets_per_session": BUCKETS, "buckets": NB, "classes": K, "top": TOP, "separation": 1,
            "launches": {"cftl_read": 1, "cfhs_peaks": 2}, "peaks_per_class": [res.peaks[c] for c in ids], "recall": r,
            "the_search_it_stands_beside_ms": 73.5, "plane_bytes": NB * K * 4}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "timeline_time.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--session", default=time.strftime("%Y-%m-%d %H:%M:%S"), help="label of the measuring session, stored in the JSON")
    args = ap.parse_args()
    with torch.no_grad():
        out = {"device": torch.cuda.get_device_name(0), "session": args.session,
               "method": "one process; HIP events; median of %d timed calls after a warm-up call; the legs of each comparison "
                         "alternating three times; spread = max - min of a leg's three medians" % args.reps,
               "arch": "ViT-B/16", "precision": "bf16", "T": T}
        out["fold"] = fold_point(args.reps)
        print(json.dumps(out["fold"]), flush=True)
        live = build_gallery()
        out["tick"] = tick_point(live, args.reps)
        print(json.dumps(out["tick"]), flush=True)
        out["recall"] = recall_point(live, args.reps)
        print(json.dumps(out["recall"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
