"""Time the stream pool against what a caller has without it (one fresh process; HIP events, medians after warm-up; run it under a time
limit of its own: `timeout -k 10 900 python tools/pool_time.py`).

    python tools/pool_time.py [--out profiles/pool_time.json] [--reps 10] [--ticks 12] [--strides 1,8] [--session NAME]

ViT-B/16, bf16, T = 8, 100 classes x 5 shots, 32 sessions.  Three legs per stride, in this one process on the same frames:

  1. uneven: a seeded schedule of --ticks service ticks, every session delivering 0 to 8 frames per tick (mean about 4), through ONE
     StreamPool.push per tick;
  2. the same frames through 32 WindowStream(n_streams=1) objects pushed one after the other -- what a caller has without the pool;
  3. lockstep: WindowStream(n_streams=32) at 8 frames per stream per push against the pool fed the same input through push_packed: the
     check that the pool's indexing (the plan, the table upload, the table-driven kernels) costs nothing.

Legs 1 and 2 time the whole schedule per repetition (every repetition starts from reset sessions, so all of them do the same work) and
report ms per tick, windows/s and frames/s; leg 3 times single pushes in steady state.  The table upload alone is timed on the side.
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from _timing import _time_ms  # noqa: E402  (tools/_timing.py)
from stream_time import build_gallery  # noqa: E402  (tools/stream_time.py: the same gallery)

T, S, PUSH = 8, 32, 8


def schedule(ticks, seed):
    """per tick, per session: frames delivered, 0 .. PUSH, uniform (mean PUSH / 2)"""
    rng = random.Random(seed)
    return [[rng.randint(0, PUSH) for _ in range(S)] for _ in range(ticks)]


def uneven_point(gal, frames, stride, sched, reps):
    """frames [S, PUSH, 3, H, W]: a tick's n frames of a session are frames[s, :n] (the content does not change the work)"""
    from clip_fsar_amd.pool import StreamPool
    from clip_fsar_amd.stream import WindowStream
    pool = StreamPool(gal, max_streams=S, stride=stride, max_push=PUSH)
    hs = [pool.open() for _ in range(S)]
    streams = [WindowStream(gal, n_streams=1, stride=stride, max_push=PUSH) for _ in range(S)]
    packed = []                                            # the pool's input of every tick, packed outside the timed region
    for tick in sched:
        members = [s for s in range(S) if tick[s]]
        packed.append((torch.cat([frames[s, :tick[s]] for s in members]), [hs[s] for s in members], [tick[s] for s in members]))
    windows = [0, 0]

    def run_pool():
        for h in hs:
            pool.reset(h)
        windows[0] = sum(pool.push_packed(*p).logits.shape[0] for p in packed)

    def run_streams():
        n = 0
        for s in range(S):
            streams[s].reset()
        for tick in sched:
            for s in range(S):
                if tick[s]:
                    n += streams[s].push(frames[s:s + 1, :tick[s]]).logits.shape[1]
        windows[1] = n

    t_pool = _time_ms(run_pool, reps)
    t_streams = _time_ms(run_streams, reps)
    assert windows[0] == windows[1], windows
    n_frames, ticks = sum(map(sum, sched)), len(sched)
    leg = lambda t: {"ms_per_tick": round(t / ticks, 3), "windows_per_s": round(windows[0] / t * 1e3, 1),
                     "frames_per_s": round(n_frames / t * 1e3, 1)}
    return {"stride": stride, "ticks": ticks, "frames": n_frames, "windows": windows[0], "mean_frames_per_session_per_tick":
            round(n_frames / ticks / S, 2), "pool": leg(t_pool), "one_stream_per_session": leg(t_streams),
            "pool_over_one_stream_per_session": round(t_streams / t_pool, 3)}


def lockstep_point(gal, frames, stride, reps):
    from clip_fsar_amd.pool import StreamPool
    from clip_fsar_amd.stream import WindowStream
    ws = WindowStream(gal, n_streams=S, stride=stride, max_push=PUSH)
    pool = StreamPool(gal, max_streams=S, stride=stride, max_push=PUSH)
    hs = [pool.open() for _ in range(S)]
    flat = frames.reshape(S * PUSH, *frames.shape[2:])
    counts = [PUSH] * S
    ws.push(frames)                                        # the first push completes fewer windows: steady state from the second on
    pool.push_packed(flat, hs, counts)
    nW = ws.push(frames).logits.shape[1]
    assert pool.push_packed(flat, hs, counts).logits.shape[0] == S * nW
    ts = {"stream": [], "pool": []}
    for _ in range(3):                                     # alternate the two sides: drift of the box lands on both
        ts["stream"].append(_time_ms(lambda: ws.push(frames), reps))
        ts["pool"].append(_time_ms(lambda: pool.push_packed(flat, hs, counts), reps))
    t_ws, t_pool = statistics.median(ts["stream"]), statistics.median(ts["pool"])
    leg = lambda t: {"ms_per_push": round(t, 3), "windows_per_s": round(S * nW / t * 1e3, 1), "frames_per_s": round(S * PUSH / t * 1e3, 1)}
    return {"stride": stride, "windows_per_push": S * nW, "window_stream": leg(t_ws), "pool": leg(t_pool),
            "pool_over_window_stream_time": round(t_pool / t_ws, 4),
            "alternating_medians_ms": {k: [round(v, 3) for v in vs] for k, vs in ts.items()}}


def upload_cost(reps):
    """the descriptor table of 32 sessions: pinned ring + asynchronous copy + event, host time per upload and device time between events"""
    from clip_fsar_amd import pool_hip as php
    up = php.TableUploader("cuda", S)
    rows = [[s, 0, PUSH, s * PUSH, 0, 1, s, 0] for s in range(S)]
    for _ in range(8):
        up.upload(rows)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(200):
        up.upload(rows)
    host_us = (time.perf_counter() - t0) / 200 * 1e6
    torch.cuda.synchronize()
    return {"host_us_per_upload": round(host_us, 1), "device_ms_per_upload": round(_time_ms(lambda: up.upload(rows), 50), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pool_time.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--ticks", type=int, default=12)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--session", default=time.strftime("%Y-%m-%d %H:%M:%S"), help="label of the measuring session, stored in the JSON")
    ap.add_argument("--strides", default="1,8")
    args = ap.parse_args()
    n_classes, shots = 100, 5
    with torch.no_grad():
        gal, res = build_gallery(n_classes, shots)
        g = torch.Generator(device="cuda").manual_seed(2)
        frames = torch.randn(S, PUSH, 3, res, res, device="cuda", generator=g)
        sched = schedule(args.ticks, args.seed)
        out = {"device": torch.cuda.get_device_name(0), "session": args.session,
               "method": "one process, all legs in it; HIP events; median of %d timed calls after a warm-up call; legs 1 and 2 time a whole "
                         "schedule of %d ticks per call, leg 3 single pushes, the two sides alternating three times" % (args.reps, args.ticks),
               "arch": "ViT-B/16", "precision": "bf16", "T": T, "classes": n_classes, "shots": shots, "sessions": S,
               "max_frames_per_session_per_tick": PUSH, "schedule_seed": args.seed, "table_upload": upload_cost(args.reps),
               "uneven": [], "lockstep": []}
        for stride in [int(v) for v in args.strides.split(",")]:
            for key, r in (("uneven", uneven_point(gal, frames, stride, sched, args.reps)),
                           ("lockstep", lockstep_point(gal, frames, stride, args.reps))):
                print(json.dumps(r), flush=True)
                out[key].append(r)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
