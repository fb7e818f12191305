"""Time per-class smoothing against the column mode it generalises (one fresh process; HIP events, medians after warm-up; run it under a
time limit of its own: `timeout -k 10 600 python tools/class_smooth_time.py`).

    python tools/class_smooth_time.py [--out profiles/class_smooth_time.json] [--reps 10] [--session NAME]

32 sessions x 8 windows per push, 3 200 classes, T = 8 (ViT-B/16 head, bf16; the classes are registered from random tower features, one
shot each: the tower is not the subject).  Two comparisons, the two legs of each alternating three times in this one process:

  a. the launch: cfcs_smooth_classes (state by (session slot, store slot), marks, generations, one "every class" key list) against
     cfsp_smooth_logits at the same dense shape, 20 launches between two events, the tables uploaded before;
  b. the tick: StreamPool.push_features_packed in steady state with smooth_by="class" against smooth_by="column" over the same
     LiveGallery and the same features (table upload, ring write, gather, context2, scoring, smoothing).

Recorded: both medians of each comparison, the three alternations of every leg, the spread (max - min) of the column leg, the host time of
the class mode's plan, and whether the class-mode tick exceeds the column-mode tick by more than that spread.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from _timing import _time_ms  # noqa: E402  (tools/_timing.py)

T, S, NW, C, ALPHA, LAUNCHES = 8, 32, 8, 3200, 0.5, 20


def alternate(legs, reps, rounds=3):
    """{name: fn} -> {name: [median ms of reps calls, per round]}, the legs taking turns so that drift of the box lands on all of them"""
    ts = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            ts[k].append(_time_ms(fn, reps))
    return ts


def summary(ts, per=1.0):
    return {k: {"median_ms": round(statistics.median(v) / per, 5), "rounds_ms": [round(x / per, 5) for x in v],
                "spread_ms": round((max(v) - min(v)) / per, 5)} for k, v in ts.items()}


def launch_point(reps):
    from clip_fsar_amd import class_smooth_hip as ch
    from clip_fsar_amd import pool_hip as ph
    g = torch.Generator(device="cuda").manual_seed(3)
    x = torch.randn(S * NW, C, device="cuda", generator=g)
    out = torch.empty_like(x)
    col_state = torch.zeros(S, C, device="cuda")
    col_table = ph.TableUploader("cuda", S).upload([[s, 0, 0, 0, 0, NW, s * NW, 1] for s in range(S)])
    cap = C + 64
    state = torch.zeros(S, cap, device="cuda")
    marks = torch.ones(S, cap, device="cuda", dtype=torch.int32)                  # every cell valid: the recurrence reads its state
    gens = torch.ones(cap, device="cuda", dtype=torch.int32)
    keys = torch.randperm(cap, device="cuda", generator=g)[:C].to(torch.int32)
    plan = ch.plan_rows(list(range(S)), [NW] * S, [None] * S, C)
    table = ch.table_uploader("cuda", S).upload(plan.rows)
    xf, of = x.view(-1), out.view(-1)

    def column():
        for _ in range(LAUNCHES):
            ph.smooth_logits(x, col_state, out, col_table, ALPHA)

    def by_class():
        for _ in range(LAUNCHES):
            ch.smooth_classes(xf, state, marks, gens, keys, of, table, ALPHA)

    ts = alternate({"column_cfsp_smooth_logits": column, "class_cfcs_smooth_classes": by_class}, reps)
    # what a launch must move: x and y of every window, and the cell -- the class mode adds the mark (read and written), the key and the
    # generation per (session, class)
    col_bytes, cls_bytes = S * C * (8 * NW + 8), S * C * (8 * NW + 8 + 16)
    return {"shape": {"sessions": S, "windows_per_session": NW, "classes": C, "store_slots": cap}, "launches_per_timed_call": LAUNCHES,
            "per_launch": summary(ts, LAUNCHES), "bytes_per_launch": {"column": col_bytes, "class": cls_bytes}, "workgroups": plan.n_chunks}


def build_gallery():
    from types import SimpleNamespace as NS
    from clip_fsar_amd.live_gallery import LiveGallery
    from clip_fsar_amd.models.base.few_shot import CNN_OTAM_CLIPFSAR
    cfg = NS(VIDEO=NS(HEAD=NS(NAME="CNN_OTAM_CLIPFSAR", BACKBONE_NAME="ViT-B/16", PRECISION="bf16"), BACKBONE=NS(META_ARCH="Identity")),
             TRAIN=NS(CLASS_NAME=["c%d" % i for i in range(64)], WAY=5), TEST=NS(CLASS_NAME=["t%d" % i for i in range(C)]),
             DATA=NS(NUM_INPUT_FRAMES=T), MODEL=NS(NAME="BaseVideoModel", EMA=NS(ENABLE=False)), BN=NS(FREEZE=False), NUM_GPUS=1,
             NUM_SHARDS=1, RANDOM_SEED=18)
    head = CNN_OTAM_CLIPFSAR(cfg).eval()
    live = LiveGallery(head, "cuda", capacity=C + 64)
    g = torch.Generator(device="cuda").manual_seed(1)
    for c0 in range(0, C, 100):
        live.add_classes_features(torch.randn(100, T, live.E, device="cuda", generator=g), list(range(c0, c0 + 100)))
    return live


def tick_point(live, reps):
    from clip_fsar_amd import class_smooth_hip as ch
    from clip_fsar_amd.pool import StreamPool
    g = torch.Generator(device="cuda").manual_seed(2)
    feats = torch.randn(S * NW, live.E, device="cuda", generator=g)
    pools = {"column": StreamPool(live, max_streams=S, stride=1, max_push=NW, smooth=ALPHA),
             "class": StreamPool(live, max_streams=S, stride=1, max_push=NW, smooth=ALPHA, smooth_by="class")}
    handles = {k: [p.open() for _ in range(S)] for k, p in pools.items()}
    counts = [NW] * S
    outs = {}
    for k, p in pools.items():                             # the first push completes one window a session: steady state from the second
        p.push_features_packed(feats, handles[k], counts)
        outs[k] = p.push_features_packed(feats, handles[k], counts)
        assert outs[k].logits.shape == (S * NW, C)
    assert torch.equal(outs["column"].logits, outs["class"].logits) and torch.equal(outs["column"].smoothed, outs["class"].smoothed)
    ts = alternate({k: (lambda k=k: pools[k].push_features_packed(feats, handles[k], counts)) for k in pools}, reps)
    t0 = time.perf_counter()
    for _ in range(200):
        ch.plan_rows(list(range(S)), counts, [None] * S, C)
    plan_us = (time.perf_counter() - t0) / 200 * 1e6
    r = summary(ts)
    excess = r["class"]["median_ms"] - r["column"]["median_ms"]
    return {"windows_per_tick": S * NW, "tick": r, "class_minus_column_ms": round(excess, 5),
            "exceeds_the_column_legs_spread": bool(excess > r["column"]["spread_ms"]), "class_mode_host_plan_us": round(plan_us, 1),
            "outputs_bit_equal": True}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "class_smooth_time.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--session", default=time.strftime("%Y-%m-%d %H:%M:%S"), help="label of the measuring session, stored in the JSON")
    args = ap.parse_args()
    with torch.no_grad():
        out = {"device": torch.cuda.get_device_name(0), "session": args.session,
               "method": "one process; HIP events; median of %d timed calls after a warm-up call; the two legs of each comparison "
                         "alternating three times; spread = max - min of a leg's three medians" % args.reps,
               "arch": "ViT-B/16", "precision": "bf16", "T": T, "alpha": ALPHA}
        out["launch"] = launch_point(args.reps)
        print(json.dumps(out["launch"]), flush=True)
        out["tick"] = tick_point(build_gallery(), args.reps)
        print(json.dumps(out["tick"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
