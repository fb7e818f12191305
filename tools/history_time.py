"""Time what StreamPool(history=) costs a push, what a search costs and where it goes, and cfhs_peaks against two yardsticks (one fresh
process; HIP events, medians after warm-up; run it under a time limit of its own: `timeout -k 10 900 python tools/history_time.py`).

    python tools/history_time.py [--out profiles/history_time.json] [--reps 10] [--session NAME]

ViT-B/16 head, bf16, T = 8, 3 200 classes registered from random tower features (tools/class_smooth_time.py's gallery: the tower is not
the subject).  Three comparisons, the legs of each alternating three times in this one process:

  a. the tick: StreamPool.push_features_packed in steady state, 32 sessions x 8 windows per push as in profiles/contest_time.json, with
     history=History(4096) against the same pool without the option, over the same gallery and features; and cfsp_ring_put alone on the
     same rows into a store of that size, 20 calls between two events -- what the option adds to a push is one such launch and its table;
  b. the search: one search() of 32 sessions x 4 096 held frames at stride = 2 (2 045 windows a session) against 4 classes, top = 16,
     whole (with its one synchronisation), and its three parts on their own over the same table and buffers: every chunk's gather
     (cfsp_window_sequences out of the store), every chunk's classify_features(classes=), and cfhs_peaks;
  c. cfhs_peaks alone on a tie-free plane of that shape (a permutation of 0 .. NW * K - 1), at the default separation, against a device
     copy of the plane's bytes -- what any pass over it must at least move -- and against a restatement in torch on the device:
     max_pool1d per session row and class, then topk over the local maxima.  On tie-free data the two agree, which is asserted.

Recorded: the medians of each comparison, the three alternations of every leg, the spread (max - min) of the tick without the option and
whether the tick with it exceeds that spread.  Nothing is asserted on time.
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
from events_time import LAUNCHES, NW, S, T, alternate  # noqa: E402  (tools/events_time.py: the same shape and alternation)

FRAMES, STRIDE, CLASSES, TOP = 4096, 2, (7, 100, 1500, 3199), 16


def tick_point(live, reps):
    from clip_fsar_amd import pool_hip as ph
    from clip_fsar_amd.history import History
    from clip_fsar_amd.pool import StreamPool
    g = torch.Generator(device="cuda").manual_seed(2)
    feats = torch.randn(S * NW, live.E, device="cuda", generator=g)
    counts = [NW] * S

    def pool(**kw):
        p = StreamPool(live, max_streams=S, stride=1, max_push=NW, **kw)
        hs = [p.open() for _ in range(S)]
        p.push_features_packed(feats, hs, counts)          # the first push completes one window a session: steady state from the second
        return p, hs, p.push_features_packed(feats, hs, counts)

    pools = {"without_history": pool(), "with_history": pool(history=History(FRAMES))}
    assert torch.equal(pools["without_history"][2].logits, pools["with_history"][2].logits)
    legs = {k: (lambda p=p, hs=hs: p.push_features_packed(feats, hs, counts)) for k, (p, hs, _) in pools.items()}
    r = summary(alternate(legs, reps))
    store = torch.empty(S, FRAMES, live.E, device="cuda")
    table = ph.TableUploader("cuda", S).upload([[s, 16, NW, s * NW, 0, 0, 0, 0] for s in range(S)])

    def put():
        for _ in range(LAUNCHES):
            ph.ring_put(feats, store, table)
    r.update(summary(alternate({"cfsp_ring_put_alone": put}, reps), LAUNCHES))
    base = r["without_history"]
    return {"windows_per_tick": S * NW, "frames_per_tick": S * NW, "store_bytes": store.numel() * 4, "tick": r,
            "history_minus_plain_ms": round(r["with_history"]["median_ms"] - base["median_ms"], 5),
            "exceeds_the_spread_of_the_leg_without_history": bool(r["with_history"]["median_ms"] - base["median_ms"] > base["spread_ms"]),
            "bytes_a_tick_writes_into_the_store": S * NW * live.E * 4, "outputs_bit_equal": True}


def search_point(live, reps):
    from clip_fsar_amd import history_hip as hh
    from clip_fsar_amd import pool_hip as ph
    from clip_fsar_amd.history import History, device_separation, plan_search
    from clip_fsar_amd.pool import StreamPool
    ids = list(CLASSES)
    p = StreamPool(live, max_streams=S, stride=STRIDE, max_push=1024, history=History(FRAMES))
    hs = [p.open() for _ in range(S)]
    g = torch.Generator(device="cuda").manual_seed(4)
    for _ in range(FRAMES // 1024):                        # the store is filled by ordinary pushes, 1 024 frames a session each
        p.push_features_packed(torch.randn(S * 1024, live.E, device="cuda", generator=g), hs, [1024] * S)
    res = p.search(ids, top=TOP)
    NWs, K = res.windows, len(ids)
    assert NWs == S * ((FRAMES - T) // STRIDE + 1) and all(len(v) == TOP for v in res.hits.values())
    plan = plan_search([(p._sessions[h].slot, p._sessions[h].t) for h in hs], T, STRIDE, 1, FRAMES)
    table = ph.TableUploader("cuda", S).upload(plan.rows)
    eng = live._fresh_engine()
    per = max(1, eng.max_frames // T)
    X = torch.empty(min(NWs, per), T, live.E, device="cuda")
    plane = res.scores.clone()
    sep = device_separation(((T - 1) * 1) // STRIDE, plan.n_windows)
    work = torch.empty(hh.workspace_words(NWs, K), device="cuda", dtype=torch.int32)
    rows, vals = torch.empty(K, TOP, device="cuda", dtype=torch.int32), torch.empty(K, TOP, device="cuda")
    n_hits, n_peaks = (torch.empty(K, device="cuda", dtype=torch.int32) for _ in range(2))

    def gather():
        for w0 in range(0, NWs, per):
            w1 = min(NWs, w0 + per)
            ph.window_sequences(p._hs_store, X[:w1 - w0], table, NWs, w0, w1, T, STRIDE, 1)

    def score():
        for w0 in range(0, NWs, per):
            live.classify_features(X[:min(NWs, w0 + per) - w0], classes=ids)

    legs = {"search": lambda: p.search(ids, top=TOP), "gather": gather, "classify_features": score,
            "cfhs_peaks": lambda: hh.peaks(plane, work, rows, vals, n_hits, n_peaks, table, sep, None, TOP)}
    r = summary(alternate(legs, reps))
    return {"sessions": S, "held_frames": FRAMES, "stride": STRIDE, "windows": NWs, "classes": K, "top": TOP, "separation": sep,
            "chunks": -(-NWs // per), "windows_per_chunk": per, "launches": {"gather": -(-NWs // per), "cfhs_peaks": 2},
            "peaks_per_class": [res.peaks[c] for c in ids], "search": r,
            "parts_sum_ms": round(sum(r[k]["median_ms"] for k in ("gather", "classify_features", "cfhs_peaks")), 5),
            "bytes_gathered": NWs * T * live.E * 4, "plane_bytes": NWs * K * 4}, (plan, table, sep)


def peaks_point(shape, reps):
    from clip_fsar_amd import history_hip as hh
    from clip_fsar_amd.history import reference_search
    plan, table, sep = shape
    NWs, K, n = plan.offsets[-1], len(CLASSES), plan.n_windows[0]
    assert all(m == n for m in plan.n_windows)
    g = torch.Generator(device="cuda").manual_seed(5)
    plane = torch.randperm(NWs * K, device="cuda", generator=g).float().view(NWs, K)          # tie-free, every value exact in fp32
    work = torch.empty(hh.workspace_words(NWs, K), device="cuda", dtype=torch.int32)
    rows, vals = torch.empty(K, TOP, device="cuda", dtype=torch.int32), torch.empty(K, TOP, device="cuda")
    n_hits, n_peaks = (torch.empty(K, device="cuda", dtype=torch.int32) for _ in range(2))
    copy = torch.empty_like(plane)
    NEG = float("-inf")

    def restated():
        x = plane.view(S, n, K).transpose(1, 2)                                               # [S, K, n]: a session row and class per line
        top = torch.nn.functional.max_pool1d(x, 2 * sep + 1, 1, sep)
        peak = torch.where(x == top, x, torch.full_like(x, NEG)).transpose(0, 1).reshape(K, S * n)      # plane rows again, per class
        v, at = peak.topk(TOP, dim=1)
        return v, at, (peak > NEG).sum(1)

    hh.peaks(plane, work, rows, vals, n_hits, n_peaks, table, sep, None, TOP)
    v, at, count = restated()
    agree = bool(torch.equal(at.sort(1).values.int(), rows)) and count.tolist() == n_peaks.tolist() \
        and bool(torch.equal(vals, plane.t().gather(1, rows.long())))
    want_rows, want_peaks = reference_search(plane.cpu(), plan.n_windows, sep, None, TOP)
    assert agree and rows.tolist() == want_rows and n_peaks.tolist() == want_peaks
    legs = {"cfhs_peaks": lambda: hh.peaks(plane, work, rows, vals, n_hits, n_peaks, table, sep, None, TOP),
            "device_copy_of_the_plane": lambda: copy.copy_(plane), "torch_max_pool1d_topk": restated}
    r = summary(alternate(legs, reps))
    return {"windows": NWs, "classes": K, "separation": sep, "top": TOP, "plane_bytes": NWs * K * 4, "peaks_per_class": n_peaks.tolist(),
            "agrees_with_the_torch_restatement_and_the_reference": agree, "peaks": r,
            "cfhs_peaks_over_copy": round(r["cfhs_peaks"]["median_ms"] / r["device_copy_of_the_plane"]["median_ms"], 3),
            "cfhs_peaks_over_torch": round(r["cfhs_peaks"]["median_ms"] / r["torch_max_pool1d_topk"]["median_ms"], 3),
            "kernel_loses_to_the_torch_restatement": bool(r["cfhs_peaks"]["median_ms"] > r["torch_max_pool1d_topk"]["median_ms"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "history_time.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--session", default=time.strftime("%Y-%m-%d %H:%M:%S"), help="label of the measuring session, stored in the JSON")
    args = ap.parse_args()
    with torch.no_grad():
        out = {"device": torch.cuda.get_device_name(0), "session": args.session,
               "method": "one process; HIP events; median of %d timed calls after a warm-up call; the legs of each comparison "
                         "alternating three times; spread = max - min of a leg's three medians" % args.reps,
               "arch": "ViT-B/16", "precision": "bf16", "T": T}
        live = build_gallery()
        out["tick"] = tick_point(live, args.reps)
        print(json.dumps(out["tick"]), flush=True)
        out["search"], shape = search_point(live, args.reps)
        print(json.dumps(out["search"]), flush=True)
        out["peaks"] = peaks_point(shape, args.reps)
        print(json.dumps(out["peaks"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
