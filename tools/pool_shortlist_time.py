"""Time a stream pool's push with and without a shortlist on the GPU (run as a fresh process; HIP events around every leg).

    python tools/pool_shortlist_time.py [--out profiles/pool_shortlist_time.json] [--reps 10] [--classes 3200 25600]

32 sessions that each complete 8 windows per push (stride = T = 8, 64 frames a session), E = 512 (ViT-B/16 head, bf16 tower -- the tower
does not run: a tick is one push_features_packed), against a LiveGallery of 3 200 and of 25 600 classes of one shot each, with per-class
smoothing (0.5), a baseline and an event rule on in both pools:

  full        StreamPool(...): every window against every class
  shortlist   StreamPool(..., shortlist=Shortlist(g, keep=64), shortlist_hold=2)

The legs alternate three times (full, shortlist, full, ...), every visit the median of `reps` ticks after a warm-up tick; a leg's figure is
the median of its three visits, and the spread of the full leg's visits says what a ratio is worth.  The full leg is the pool as it was
before the option existed: the yardstick.  The stages of the shortlist leg are timed the same way, one after the other on the leg's own
intermediate results -- the gather of the windows aside: context2 + norms, the coarse rows and scores, cfps_select_pinned (on copies of the
pool's planes, the tick advancing with every call, so every call finds the previous call's list held) beside cfsh_select on the same
scores, the grouped OTAM launch, smoothing, the baselines, the detector.  The gallery is tools/shortlist_time.py's synthetic one, and a
session's windows are noisy copies of one class's shot.  Nothing is asserted on time.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

from _timing import _time_ms  # noqa: E402  (tools/_timing.py)
from shortlist_time import BATCH, FRAME, NOISE, _head  # noqa: E402  (tools/shortlist_time.py: the head and the gallery's recipe)

SESSIONS, NW_S, T, KEEP, HOLD, ALPHA = 32, 8, 8, 64, 2, 0.5


def point(head, C, reps, rounds=3):
    from clip_fsar_amd import class_smooth_hip as cship
    from clip_fsar_amd import pool_select_hip as pship
    from clip_fsar_amd.baseline import Baseline
    from clip_fsar_amd.events import EventRule
    from clip_fsar_amd.live_gallery import LiveGallery
    from clip_fsar_amd.pool import StreamPool
    from clip_fsar_amd.shortlist import Shortlist
    live = LiveGallery(head, "cuda", capacity=C)
    E = live.E
    g = torch.Generator(device="cuda").manual_seed(C)
    base = torch.randn(E, device="cuda", generator=g)
    truth = torch.randperm(C, device="cuda", generator=g)[:SESSIONS].tolist()        # the class every session's windows copy
    shots = torch.empty(SESSIONS, T, E, device="cuda")
    for c0 in range(0, C, BATCH):                            # one shot per class, registered from features
        n = min(BATCH, C - c0)
        F = (base + torch.randn(n, 1, E, device="cuda", generator=g) + FRAME * torch.randn(n, T, E, device="cuda", generator=g)).contiguous()
        for i, c in enumerate(truth):
            if c0 <= c < c0 + n:
                shots[i] = F[c - c0]
        live.add_classes_features(F, list(range(c0, c0 + n)))
    # a tick's frames: per session 8 windows of T tower rows each, one after the other (stride = T: a window is T consecutive frames)
    frames = (shots[:, None] + NOISE * torch.randn(SESSIONS, NW_S, T, E, device="cuda", generator=g)).view(SESSIONS * NW_S * T, E).contiguous()
    kw = dict(max_streams=SESSIONS, stride=T, rate=1, max_push=NW_S * T, smooth=ALPHA, smooth_by="class",
              baseline=Baseline(), events=EventRule(on=4.0, off=2.0, min_on=2, min_off=2))
    sl = Shortlist(live, keep=KEEP)
    pools = {"full": StreamPool(live, **kw), "shortlist": StreamPool(live, shortlist=sl, shortlist_hold=HOLD, **kw)}
    handles = {k: [p.open() for _ in range(SESSIONS)] for k, p in pools.items()}
    counts = [NW_S * T] * SESSIONS
    res = {}

    def tick(k):
        def fn():
            res[k] = pools[k].push_features_packed(frames, handles[k], counts)
        return fn

    visits = {k: [] for k in pools}
    events = {k: 0 for k in pools}
    for _ in range(rounds):
        for k in pools:
            visits[k].append(_time_ms(tick(k), reps))
            events[k] += len(pools[k].take_events())         # between the visits: the queue of pushes never fills
    ms = {k: statistics.median(v) for k, v in visits.items()}
    # ---- the stages of the shortlist leg, on its own intermediate results
    p = pools["shortlist"]
    eng = live._fresh_engine()
    slots = [live.slot_of(c) for c in live.class_ids]
    cols = live._columns(None)
    gens = live.slot_generations()
    W = frames.view(SESSIONS * NW_S, T, E)
    n_w = [NW_S] * SESSIONS
    K = min(KEEP, C)
    recs = [p._sessions[h] for h in handles["shortlist"]]
    cap = gens.shape[0]
    planes = [t.clone() for t in (p._ev_cells.at(cap)[0], p._ev_cells.at(cap)[3], *p._sl_cells.planes,
                                  p._smooth_cells.at(cap)[1], p._bl_cells.at(cap)[3])]
    uploader = pship.table_uploader("cuda", SESSIONS)
    now = {"tick": recs[0].tick}
    st = {}

    def select_pinned():
        now["tick"] += 1
        rows, _ = pship.table_rows(n_w, [s.slot for s in recs], [now["tick"]] * SESSIONS)
        out = [torch.empty(SESSIONS, K, device="cuda", dtype=torch.int32) for _ in range(3)]
        n_pins = torch.empty(SESSIONS, device="cuda", dtype=torch.int32)
        work = torch.empty(pship.workspace_floats(SESSIONS, C), device="cuda", dtype=torch.float32)
        pship.select_pinned(st["S"], cols, gens, *planes, uploader.upload(rows), KEEP, HOLD, *out, n_pins, work)
        st["pinned"], st["n_pins"] = out, n_pins

    chunks = -(-K // cship.CHUNK)
    key_rows = [[s.slot, NW_S, j * NW_S * K, K, j * K, j * chunks] for j, s in enumerate(recs)]
    cplan = cship.SmoothPlan(key_rows, [], False, SESSIONS * NW_S * K, SESSIONS * chunks)

    def keyed():
        return cplan, gens, st["sel"][1].view(-1), p._smooth_tables.upload(key_rows)

    stages = {"context2_and_norms": lambda: st.update(q=sl._queries(eng, W, False)),
              "coarse_rows_and_scores": lambda: st.update(S=sl._coarse_scores(st["q"][0], st["q"][1], sl._stale(slots), cols)),
              "select_pinned": select_pinned,
              "cfsh_select_on_the_same_scores": lambda: st.update(sel=sl._select(st["S"], cols, n_w, K)),
              "grouped_otam": lambda: st.update(out=sl._exact(st["q"][0], st["q"][1], st["sel"][1], n_w, K)),
              "smooth_classes": lambda: st.update(y=p._smooth_classes(keyed(), st["out"][0])),
              "baselines": lambda: st.update(z=p._normalize(keyed(), st["y"])),
              "detector": lambda: p._detect(handles["shortlist"], recs, res["shortlist"].first_window, st["z"], keyed(), columns=st["sel"][0])}
    stage_ms = {}
    for k, fn in stages.items():
        stage_ms[k] = round(_time_ms(fn, reps), 4)
        if k == "detector":
            p.take_events()
    torch.cuda.synchronize()
    stats = p.stats()
    return {"classes": C, "sessions": SESSIONS, "windows_per_session": NW_S, "T": T, "E": E, "keep": KEEP, "hold": HOLD, "smooth": ALPHA,
            "full_ms": round(ms["full"], 4), "shortlist_ms": round(ms["shortlist"], 4),
            "full_over_shortlist": round(ms["full"] / ms["shortlist"], 3),
            "full_visit_spread": round((max(visits["full"]) - min(visits["full"])) / ms["full"], 4),
            "visits_ms": {k: [round(t, 4) for t in v] for k, v in visits.items()}, "stages_ms": stage_ms,
            "events": events, "pins_per_session_in_the_stage_run": round(float(st["n_pins"].float().mean()), 2),
            "pins": stats["pins"], "pins_dropped": stats["pins_dropped"], "coarse_rows_refreshed": sl.stats["refreshed"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pool_shortlist_time.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--classes", type=int, nargs="+", default=[3200, 25600])
    args = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "points": []}
    with torch.no_grad():
        head = _head(max(args.classes))
        for C in args.classes:
            pt = point(head, C, args.reps)
            print(json.dumps(pt), flush=True)
            out["points"].append(pt)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
