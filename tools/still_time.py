"""Time the still-frame gate: the pixel tick of tools/ingest_time.py (its leg (a): push_packed on resident fp32 frames) with 0 %, 50 % and
90 % of the frames repeating their predecessor, through a pool without still= and through a pool with still=StillGate() (one fresh
process; HIP events, medians after warm-up; run it under a time limit of its own: `timeout -k 10 900 python tools/still_time.py`).

    python tools/still_time.py [--out profiles/still_time.json] [--reps 10] [--ticks 12] [--session NAME]

ViT-B/16, bf16, T = 8, 100 classes x 5 shots, 32 sessions, the uneven 12-tick schedule of tools/pool_time.py.  Frame k of a session (k
counts from its reset) is new when k % period == 0 and repeats frame k - 1 otherwise: period 1, 2 and 10.  Seven legs in this one
process, each timing the whole schedule per repetition from reset sessions: gate off and gate on at each of the three repeat rates, and
push_features_packed of precomputed tower rows -- the tick a gated pool approaches when nothing moves.  The legs alternate three times;
per leg the median of the three medians and their spread are kept.  cfsk_changed alone is timed on the side at the largest tick's shape,
against the bytes it requests (2 N L 4: the form that was built reads a frame as x and again as the next frame's y) and against the floor
((N + S) L 4).
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
from pool_time import PUSH, S, T, schedule  # noqa: E402  (tools/pool_time.py: the same schedule)
from stream_time import build_gallery  # noqa: E402  (tools/stream_time.py: the same gallery)

PERIODS = {"repeat_0": 1, "repeat_50": 2, "repeat_90": 10}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "still_time.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--ticks", type=int, default=12)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--session", default=time.strftime("%Y-%m-%d %H:%M:%S"), help="label of the measuring session, stored in the JSON")
    args = ap.parse_args()
    from clip_fsar_amd import pool_hip as php
    from clip_fsar_amd import still_hip as skhip
    from clip_fsar_amd.pool import StreamPool
    from clip_fsar_amd.still import StillGate
    with torch.no_grad():
        gal, res = build_gallery(100, 5)
        L = 3 * res * res
        g = torch.Generator().manual_seed(2)
        distinct = (torch.randn(S, PUSH, 3, res, res, generator=g) * 0.5).cuda()       # consecutive ones differ everywhere
        sched = schedule(args.ticks, args.seed)
        off = StreamPool(gal, max_streams=S, stride=1, max_push=PUSH)
        on = StreamPool(gal, max_streams=S, stride=1, max_push=PUSH, still=StillGate())
        hs = [off.open() for _ in range(S)]
        assert hs == [on.open() for _ in range(S)]
        ticks = {}                                         # per repeat rate, per tick: (handles, counts, packed fp32 frames)
        for name, period in PERIODS.items():
            t, ticks[name] = [0] * S, []
            for tick in sched:
                m = [s for s in range(S) if tick[s]]
                parts = []
                for s in m:
                    parts.append(distinct[s, [(k // period) % PUSH for k in range(t[s], t[s] + tick[s])]])
                    t[s] += tick[s]
                ticks[name].append(([hs[s] for s in m], [tick[s] for s in m], torch.cat(parts)))
        eng = gal._fresh_engine()
        feats = []                                         # the feature-push tick: the tower rows of the 0 % frames, computed once
        for handles, counts, packed in ticks["repeat_0"]:
            f = torch.empty(packed.shape[0], gal.E, device="cuda")
            for f0 in range(0, packed.shape[0], eng.max_frames):
                eng.vit.forward(packed[f0:f0 + eng.max_frames], f[f0:f0 + eng.max_frames])
            feats.append(f)
        windows, towers = {}, {}

        def run(pool, name):
            def fn():
                for h in hs:
                    pool.reset(h)
                before = pool.stats()["tower_frames"]
                n = 0
                for i, (handles, counts, packed) in enumerate(ticks[name if name != "features" else "repeat_0"]):
                    po = pool.push_features_packed(feats[i], handles, counts) if name == "features" else pool.push_packed(packed, handles, counts)
                    n += po.logits.shape[0]
                windows[(pool is on, name)] = n
                towers[(pool is on, name)] = pool.stats()["tower_frames"] - before
            return fn

        legs = [(gate, name) for name in PERIODS for gate in (False, True)] + [(False, "features")]
        ts = {leg: [] for leg in legs}
        for _ in range(3):                                 # alternate the legs: drift of the box lands on all of them
            for gate, name in legs:
                ts[(gate, name)].append(_time_ms(run(on if gate else off, name), args.reps))
        assert len(set(windows.values())) == 1, windows
        n_frames, n_ticks = sum(map(sum, sched)), len(sched)
        leg = lambda v: {"ms_per_tick": round(statistics.median(v) / n_ticks, 3),
                         "ms_per_tick_of_the_three_visits": [round(x / n_ticks, 3) for x in v],
                         "spread_over_median": round((max(v) - min(v)) / statistics.median(v), 4)}
        # the compare alone: the largest tick's frames (0 % repeats: every element differs, nothing short-circuits anyway), one table
        big = max(range(n_ticks), key=lambda i: sum(ticks["repeat_0"][i][1]))
        handles, counts, packed = ticks["repeat_0"][big]
        n = packed.shape[0]
        rows, f0 = [], 0
        for i, c in enumerate(counts):
            rows.append([i, f0, c, 0])
            f0 += c
        up = php.TableUploader("cuda", S, cols=skhip.TABLE_COLS)
        prev = torch.randn(S, L, device="cuda")
        out = torch.empty(n, dtype=torch.int32, device="cuda")
        work = torch.empty(skhip.workspace_ints(n, L), dtype=torch.int32, device="cuda")
        flat = packed.view(n, L)
        t_changed = _time_ms(lambda: skhip.changed(flat, prev, out, work, up.upload(rows), 0.0), 50)
        t_upload = _time_ms(lambda: up.upload(rows), 50)
        t_sync = _time_ms(lambda: (skhip.changed(flat, prev, out, work, up.upload(rows), 0.0), out.cpu()), 50)
        requested, floor = 2 * n * L * 4, (n + len(counts)) * L * 4
        kernel_ms = max(t_changed - t_upload, 1e-6)
        result = {
            "device": torch.cuda.get_device_name(0), "session": args.session,
            "method": "one process, all legs in it; HIP events; median of %d timed schedules of %d ticks after a warm-up schedule, the "
                      "legs alternating three times (median of the three medians, their spread beside it); every repetition starts "
                      "from reset sessions; frames resident as fp32" % (args.reps, n_ticks),
            "arch": "ViT-B/16", "precision": "bf16", "T": T, "classes": 100, "shots": 5, "sessions": S, "stride": 1,
            "schedule_seed": args.seed, "frames": n_frames, "windows": windows[(False, "repeat_0")], "frame_elements": L,
            "feature_push_tick": leg(ts[(False, "features")])}
        for name in PERIODS:
            a, b = ts[(False, name)], ts[(True, name)]
            result[name] = {"gate_off": leg(a), "gate_on": leg(b), "on_over_off": round(statistics.median(b) / statistics.median(a), 4),
                            "tower_frames_gate_off": towers[(False, name)], "tower_frames_gate_on": towers[(True, name)]}
        result["changed_alone"] = {"frames": n, "sessions": len(counts), "bytes_requested": requested, "bytes_floor": floor,
                                   "two_launches_and_table_upload_ms": round(t_changed, 4), "table_upload_ms": round(t_upload, 4),
                                   "with_counts_to_host_ms": round(t_sync, 4),
                                   "requested_TBps": round(requested / kernel_ms / 1e9, 3), "floor_TBps": round(floor / kernel_ms / 1e9, 3)}
    print(json.dumps(result), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
