"""Time the pool's ingest: decoded uint8 clips of mixed geometry -> a StreamPool tick (one fresh process; HIP events, medians after
warm-up; run it under a time limit of its own: `timeout -k 10 900 python tools/ingest_time.py`).

    python tools/ingest_time.py [--out profiles/ingest_time.json] [--reps 10] [--ticks 12] [--stride 1] [--session NAME]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/ingest_time.py --profile-ticks 50      # one leg-(c) tick, repeated, small gallery

ViT-B/16, bf16, T = 8, 100 classes x 5 shots, 32 sessions, the uneven 12-tick schedule of tools/pool_time.py; every session has a source
resolution of its own.  Four legs in this one process on the same frames, each timing the whole schedule per repetition:

  (a) push_packed on resident fp32 frames: the pool without any ingest, the floor;
  (b) today's route from pinned host uint8: per session .cuda() + preprocess_video, then cat + push_packed
      (b_nb: the same with .cuda(non_blocking=True));
  (c) push_u8_packed from the same pinned host uint8;
  (d) push_u8_packed from resident device uint8.

The transform kernel alone is timed on the side, on the clips of the schedule's largest tick, against the bytes it moves.
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

import clip_fsar_amd.synth as synth  # noqa: E402

SIZES = [(240, 320), (256, 340), (360, 640), (480, 640), (270, 480), (224, 224), (288, 352), (97, 131)]
SCALE, CROP = 256, 224
DEVICE_COPY_TBPS = 4.7    # what a device-to-device copy reaches on these boxes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ingest_time.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--ticks", type=int, default=12)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--stride", type=int, default=1)
    ap.add_argument("--session", default=time.strftime("%Y-%m-%d %H:%M:%S"), help="label of the measuring session, stored in the JSON")
    ap.add_argument("--profile-ticks", type=int, default=0, help="no timing: a small gallery and that many repetitions of one leg-(c) tick")
    args = ap.parse_args()
    from clip_fsar_amd.ingest import FrameIngest
    from clip_fsar_amd.pool import StreamPool
    from clip_fsar_amd.preprocess import preprocess_video
    mean, std = synth.CLIP_MEAN, synth.CLIP_STD
    n_classes, shots = (10, 1) if args.profile_ticks else (100, 5)
    with torch.no_grad():
        gal, res = build_gallery(n_classes, shots)
        assert res == CROP
        g = torch.Generator().manual_seed(2)
        host = [torch.randint(0, 256, (PUSH,) + SIZES[s % len(SIZES)] + (3,), dtype=torch.uint8, generator=g).pin_memory() for s in range(S)]
        dev_u8 = [h.cuda() for h in host]
        fp32 = [preprocess_video(d, SCALE, CROP, mean, std) for d in dev_u8]
        sched = schedule(args.ticks, args.seed)
        pool = StreamPool(gal, max_streams=S, stride=args.stride, max_push=PUSH, ingest=FrameIngest("cuda", SCALE, CROP, mean, std))
        hs = [pool.open() for _ in range(S)]
        ticks = []                                         # per tick: (members, handles, counts, packed fp32 frames)
        for tick in sched:
            m = [s for s in range(S) if tick[s]]
            ticks.append((m, [hs[s] for s in m], [tick[s] for s in m], torch.cat([fp32[s][:tick[s]] for s in m])))
        windows = {}

        def run(leg):
            def fn():
                for h in hs:
                    pool.reset(h)
                n = 0
                for m, handles, counts, packed in ticks:
                    if leg == "a":
                        po = pool.push_packed(packed, handles, counts)
                    elif leg in ("b", "b_nb"):
                        up = [host[s][:c].cuda(non_blocking=leg == "b_nb") for s, c in zip(m, counts)]
                        po = pool.push_packed(torch.cat([preprocess_video(u, SCALE, CROP, mean, std) for u in up]), handles, counts)
                    else:
                        src = host if leg == "c" else dev_u8
                        po = pool.push_u8_packed([src[s][:c] for s, c in zip(m, counts)], handles)
                    n += po.logits.shape[0]
                windows[leg] = n
            return fn

        if args.profile_ticks:
            big = max(range(len(ticks)), key=lambda i: sum(ticks[i][2]))
            m, handles, counts, _ = ticks[big]
            for _ in range(3 + args.profile_ticks):
                pool.push_u8_packed([host[s][:c] for s, c in zip(m, counts)], handles)
            torch.cuda.synchronize()
            print(json.dumps({"profiled_ticks": 3 + args.profile_ticks, "frames_per_tick": sum(counts), "sessions_in_tick": len(m)}))
            return
        legs = ("a", "b", "b_nb", "c", "d")
        ts = {leg: [] for leg in legs}
        for _ in range(3):                                 # alternate the legs: drift of the box lands on all of them
            for leg in legs:
                ts[leg].append(_time_ms(run(leg), args.reps))
        assert len(set(windows.values())) == 1, windows
        n_frames, n_ticks = sum(map(sum, sched)), len(sched)
        med = {leg: statistics.median(v) for leg, v in ts.items()}
        # the kernel alone: the largest tick's clips, resident, through FrameIngest.transform (staging copy + table upload + kernel) and
        # through the binding on a prepared staging buffer (kernel + table upload only)
        big = max(range(len(ticks)), key=lambda i: sum(ticks[i][2]))
        m, _, counts, _ = ticks[big]
        clips = [dev_u8[s][:c] for s, c in zip(m, counts)]
        fi = pool.ingest
        from clip_fsar_amd import ingest_hip as ihp
        from clip_fsar_amd.ingest import plan_ingest
        plan = plan_ingest([c.shape[:3] for c in clips], SCALE, CROP)
        staged = torch.empty(plan.total_bytes, dtype=torch.uint8, device="cuda")
        for off, c in zip(plan.offsets, clips):
            staged[off:off + c.numel()].copy_(c.reshape(-1))
        out = torch.empty(plan.n_frames, 3, CROP, CROP, device="cuda")
        up = ihp.table_uploader("cuda", 64)
        t_kernel = _time_ms(lambda: ihp.transform_frames(staged, out, up.upload(plan.rows), CROP, mean, std), 50)
        t_transform = _time_ms(lambda: fi.transform(clips), 50)
        t_upload = _time_ms(lambda: up.upload(plan.rows), 50)
        t_per_clip = _time_ms(lambda: [preprocess_video(c, SCALE, CROP, mean, std) for c in clips], 50)
        src_bytes, out_bytes = sum(c.numel() for c in clips), out.numel() * 4
        floor_ms = (src_bytes + out_bytes) / (DEVICE_COPY_TBPS * 1e12) * 1e3
        leg = lambda t: {"ms_per_tick": round(t / n_ticks, 3), "frames_per_s": round(n_frames / t * 1e3, 1)}
        result = {
            "device": torch.cuda.get_device_name(0), "session": args.session,
            "method": "one process, all legs in it; HIP events; median of %d timed schedules of %d ticks after a warm-up schedule, the "
                      "legs alternating three times (median of the three medians); every repetition starts from reset sessions" % (
                          args.reps, n_ticks),
            "arch": "ViT-B/16", "precision": "bf16", "T": T, "classes": n_classes, "shots": shots, "sessions": S, "stride": args.stride,
            "schedule_seed": args.seed, "frames": n_frames, "windows": windows["a"], "source_sizes": SIZES, "scale": SCALE, "crop": CROP,
            "a_push_packed_resident_fp32": leg(med["a"]), "b_per_session_cuda_preprocess_cat_push": leg(med["b"]),
            "b_nb_the_same_non_blocking": leg(med["b_nb"]), "c_push_u8_packed_pinned_host": leg(med["c"]),
            "d_push_u8_packed_resident_u8": leg(med["d"]),
            "c_over_a": round(med["c"] / med["a"], 4), "d_over_a": round(med["d"] / med["a"], 4), "b_over_c": round(med["b"] / med["c"], 4),
            "b_nb_over_c": round(med["b_nb"] / med["c"], 4),
            "alternating_medians_ms_per_schedule": {k: [round(v, 3) for v in vs] for k, vs in ts.items()},
            "bytes_per_tick_mean": {"uint8_source": round(sum(host[s][:c].numel() for tick in sched for s, c in enumerate(tick) if c) / n_ticks),
                                    "fp32_frames": round(n_frames * 3 * CROP * CROP * 4 / n_ticks)},
            "transform_alone": {"frames": plan.n_frames, "groups": len(clips), "source_bytes": src_bytes, "out_bytes": out_bytes,
                                "kernel_and_table_upload_ms": round(t_kernel, 4), "table_upload_ms": round(t_upload, 4),
                                "transform_with_device_staging_ms": round(t_transform, 4),
                                "preprocess_video_clip_by_clip_ms": round(t_per_clip, 4),
                                "bytes_at_%.1f_TBps_ms" % DEVICE_COPY_TBPS: round(floor_ms, 4),
                                "kernel_over_copy_floor": round((t_kernel - t_upload) / floor_ms, 2)}}
    print(json.dumps(result), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
