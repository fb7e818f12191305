"""Time a stream pool's tick with tempo windows on the GPU (run as a fresh process; HIP events around every leg).

    python tools/tempo_time.py [--out profiles/tempo_time.json] [--reps 10] [--classes 3200]

One tick is one push_features_packed: 32 sessions pushing 8 frames each at stride 1, so every session completes 8 windows -- 256 windows,
T = 8, E = 512 (ViT-B/16 head, bf16 tower -- the tower does not run: the legs start from tower features), against a LiveGallery of
3 200 classes of one shot each.  Three legs, every pool warmed past its first window before anything is timed:

  rate3       one StreamPool(rate=3): what a tick costs today, and the yardstick
  per_rate    three StreamPools with rate 1, 2 and 3 pushed the same features, then torch.stack(...).max(0) of their logits: today's
              workaround for a search over tempos (its windows of different rates end on different frames; only the cost is compared)
  rates       one StreamPool(rates=(1, 2, 3)): every window gathered at three tempos, scored, reduced

The legs alternate three times (rate3, per_rate, rates, rate3, ...), every visit the median of `reps` ticks after a warm-up tick; a leg's
figure is the median of its three visits, and the spread of a leg's visits says what a difference is worth.  The two kernels are also timed
alone at the tick's shape: cftp_window_sequences for 256 windows x 3 tempos, and cftp_reduce of [256 x 3, 3 200] scores, whose
(R + 2) * NW * C * 4 bytes over its time are quoted as a rate.  Nothing is asserted on time.
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

S, NW_S, T, FRAME, BATCH = 32, 8, 8, 0.5, 1024
RATES = (1, 2, 3)
STRIDE = 1


def _gallery(head, C):
    from clip_fsar_amd.live_gallery import LiveGallery
    live = LiveGallery(head, "cuda", capacity=C)
    g = torch.Generator(device="cuda").manual_seed(C)
    base = torch.randn(live.E, device="cuda", generator=g)
    for c0 in range(0, C, BATCH):                            # one shot per class, registered from features
        n = min(BATCH, C - c0)
        F = (base + torch.randn(n, 1, live.E, device="cuda", generator=g) + FRAME * torch.randn(n, T, live.E, device="cuda", generator=g))
        live.add_classes_features(F.contiguous(), list(range(c0, c0 + n)))
    return live


def ticks(head, C, reps, rounds=3):
    from clip_fsar_amd.pool import StreamPool
    live = _gallery(head, C)
    g = torch.Generator(device="cuda").manual_seed(C + 1)
    n = NW_S * STRIDE                                        # frames per session and tick: 8 windows each once a session is warm
    feats = torch.randn(S * n, live.E, device="cuda", generator=g)
    counts = [n] * S

    def pool(**kw):
        p = StreamPool(live, max_streams=S, stride=STRIDE, max_push=n, **kw)
        hs = [p.open() for _ in range(S)]
        for _ in range(-(-(T - 1) * RATES[-1] // n) + 1):    # past every session's first window, at any of the rates
            p.push_features_packed(feats, hs, counts)
        return p, hs

    one, one_h = pool(rate=RATES[-1])
    each = [pool(rate=r) for r in RATES]
    tempo, tempo_h = pool(rates=RATES)
    res = {}

    def rate3():
        res["rate3"] = one.push_features_packed(feats, one_h, counts)

    def per_rate():
        outs = [p.push_features_packed(feats, hs, counts) for p, hs in each]
        res["per_rate"] = torch.stack([o.logits for o in outs]).max(0).values

    def rates():
        res["rates"] = tempo.push_features_packed(feats, tempo_h, counts)

    legs = {"rate3": rate3, "per_rate": per_rate, "rates": rates}
    visits = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            visits[k].append(_time_ms(fn, reps))
    ms = {k: statistics.median(v) for k, v in visits.items()}
    torch.cuda.synchronize()
    out = res["rates"]
    spread = {k: round((max(v) - min(v)) / ms[k], 4) for k, v in visits.items()}
    share = torch.bincount(out.tempo.view(-1).long(), minlength=len(RATES)).float() / out.tempo.numel()
    return {"classes": C, "sessions": S, "windows": out.logits.shape[0], "T": T, "E": live.E, "stride": STRIDE, "rates": list(RATES),
            "rate3_ms": round(ms["rate3"], 4), "per_rate_ms": round(ms["per_rate"], 4), "rates_ms": round(ms["rates"], 4),
            "rates_over_rate3": round(ms["rates"] / ms["rate3"], 3), "rates_over_per_rate": round(ms["rates"] / ms["per_rate"], 3),
            "visit_spread": spread, "visits_ms": {k: [round(t, 4) for t in v] for k, v in visits.items()},
            "windows_per_tick_equal": out.logits.shape[0] == res["rate3"].logits.shape[0] == res["per_rate"].shape[0] == S * NW_S,
            "logits_finite": bool(torch.isfinite(out.logits).all()), "share_of_cells_per_tempo": [round(float(x), 4) for x in share]}


def kernels_alone(C, reps, E=512):
    from clip_fsar_amd import pool_hip as ph
    from clip_fsar_amd import tempo_hip as th
    R, rmax = len(RATES), RATES[-1]
    NW = S * NW_S
    cap = (T - 1) * rmax + NW_S * STRIDE
    g = torch.Generator(device="cuda").manual_seed(7)
    ring = torch.randn(S, cap, E, device="cuda", generator=g)
    rows = [[s, 0, NW_S * STRIDE, s * NW_S * STRIDE, 0, NW_S, s * NW_S, 0] for s in range(S)]
    table = ph.TableUploader("cuda", S).upload(rows)
    X = torch.empty(NW * R, T, E, device="cuda")
    gather_ms = _time_ms(lambda: th.window_sequences(ring, X, table, NW, 0, NW, T, STRIDE, RATES), reps)
    scores = torch.randn(NW * R, C, device="cuda", generator=g)
    out, tempo = torch.empty(NW, C, device="cuda"), torch.empty(NW, C, device="cuda", dtype=torch.int32)
    reduce_ms = _time_ms(lambda: th.reduce(scores, out, tempo, R), reps)
    torch.cuda.synchronize()
    gather_bytes, reduce_bytes = 2 * NW * R * T * E * 4, (R + 2) * NW * C * 4
    return {"windows": NW, "R": R, "T": T, "E": E, "classes": C,
            "gather_ms": round(gather_ms, 4), "gather_bytes": gather_bytes, "gather_GBps": round(gather_bytes / gather_ms / 1e6, 1),
            "reduce_ms": round(reduce_ms, 4), "reduce_bytes": reduce_bytes, "reduce_GBps": round(reduce_bytes / reduce_ms / 1e6, 1),
            "reduce_equals_torch_max": bool(torch.equal(out, scores.view(NW, R, C).max(1).values))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tempo_time.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--classes", type=int, default=3200)
    args = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0), "reps": args.reps,
           "method": "one process; HIP events; median of `reps` timed ticks after a warm-up tick; the three legs alternating three times, a "
                     "leg's figure the median of its three visits; the kernels alone: one such median each, launch included"}
    with torch.no_grad():
        out["tick"] = ticks(_head(args.classes), args.classes, args.reps)
        print(json.dumps(out["tick"]), flush=True)
        out["kernels_alone"] = kernels_alone(args.classes, args.reps)
        print(json.dumps(out["kernels_alone"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
