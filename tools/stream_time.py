"""Time window streams against SupportGallery.classify on the GPU (one fresh process; HIP events, medians over --reps timed calls after
warm-up calls; run it under a time limit of its own: `timeout -k 10 600 python tools/stream_time.py`).

    python tools/stream_time.py [--out profiles/stream_time.json] [--reps 10] [--session NAME]

ViT-B/16, bf16, T = 8, 100 classes x 5 shots, B = 32 lockstep streams, pushes of 8 frames.  At strides 1, 2, 4 and T, in steady state
(every push completes 8 / stride windows per stream), at EQUAL window counts and in this one process:

  * WindowStream.push of [32, 8, 3, 224, 224]: the tower on 256 frames, the ring write, the gather, context2 + the gallery kernels on
    32 * 8 / stride windows;
  * SupportGallery.classify on the same windows materialised as clips [32 * 8 / stride, 8, 3, 224, 224] -- the path a caller without the
    stream has: the tower on every frame of every clip.

Written per stride: windows/s of both, their ratio, tower frames per window of both, and the share of the stream's step outside the tower
(1 - the tower's own time on the push's 256 frames / the push), beside the push_features time (the step without the tower).
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

T, B, PUSH = 8, 32, 8


def build_gallery(n_classes, shots):
    from types import SimpleNamespace as NS
    import clip_fsar_amd.synth as synth
    from clip_fsar_amd.gallery import SupportGallery
    from clip_fsar_amd.models.base.few_shot import CNN_OTAM_CLIPFSAR
    cfg = NS(VIDEO=NS(HEAD=NS(NAME="CNN_OTAM_CLIPFSAR", BACKBONE_NAME="ViT-B/16", PRECISION="bf16"), BACKBONE=NS(META_ARCH="Identity")),
             TRAIN=NS(CLASS_NAME=["c%d" % i for i in range(64)], WAY=5), TEST=NS(CLASS_NAME=["t%d" % i for i in range(n_classes)]),
             DATA=NS(NUM_INPUT_FRAMES=T), MODEL=NS(NAME="BaseVideoModel", EMA=NS(ENABLE=False)), BN=NS(FREEZE=False), NUM_GPUS=1,
             NUM_SHARDS=1, RANDOM_SEED=18)
    head = CNN_OTAM_CLIPFSAR(cfg).eval()
    res = synth.ARCHS["ViT-B/16"]["res"]
    g = torch.Generator(device="cuda").manual_seed(1)
    gal = SupportGallery(head, "cuda")
    for c0 in range(0, n_classes, 20):                     # registration in pieces: the support pixels need not be resident at once
        c1 = min(n_classes, c0 + 20)
        V = torch.randn((c1 - c0) * shots, T, 3, res, res, device="cuda", generator=g)
        gal.add_classes(V, [c0 + i // shots for i in range((c1 - c0) * shots)])
    return gal, res


def stride_point(gal, frames, stride, reps):
    from clip_fsar_amd.stream import WindowStream
    eng = gal._fresh_engine()
    s = WindowStream(gal, n_streams=B, stride=stride, max_push=PUSH)
    halves = [frames[:, :PUSH].contiguous(), frames[:, PUSH:].contiguous()]
    state = {"i": 0}

    def push():
        out = s.push(halves[state["i"] & 1])
        state["i"] += 1
        return out

    push()                                                 # the first push completes fewer windows: steady state from the second on
    nW = push().logits.shape[1]
    assert nW == PUSH // stride, (nW, stride)
    t_push = _time_ms(push, reps)
    feats = torch.empty(B, PUSH, gal.E, device="cuda")
    flat = halves[0].reshape(B * PUSH, *frames.shape[2:])
    t_tower = _time_ms(lambda: eng.vit.forward(flat, feats.view(B * PUSH, gal.E)), reps)
    sf = WindowStream(gal, n_streams=B, stride=stride, max_push=PUSH)
    sf.push_features(feats)
    t_feat = _time_ms(lambda: sf.push_features(feats), reps)
    # the same number of windows as clips: windows 0 .. nW-1 of the 16-frame pool of every stream
    idx = torch.tensor([[k * stride + j for j in range(T)] for k in range(nW)], device="cuda")
    clips = frames[:, idx].reshape(B * nW, T, *frames.shape[2:]).contiguous()
    t_cls = _time_ms(lambda: gal.classify(clips), reps)
    windows = B * nW
    del clips
    return {"stride": stride, "windows_per_step": windows,
            "stream_push_ms": round(t_push, 3), "stream_windows_per_s": round(windows / t_push * 1e3, 1),
            "classify_ms": round(t_cls, 3), "classify_windows_per_s": round(windows / t_cls * 1e3, 1),
            "stream_over_classify": round(t_cls / t_push, 3), "frame_count_ratio": T / stride,
            "tower_frames_per_window": {"stream": B * PUSH / windows, "classify": float(T)},
            "tower_ms_on_the_push_frames": round(t_tower, 3), "push_features_ms": round(t_feat, 3),
            "share_outside_tower": round(1.0 - t_tower / t_push, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_time.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--session", default=time.strftime("%Y-%m-%d %H:%M:%S"), help="label of the measuring session, stored in the JSON")
    ap.add_argument("--strides", default="1,2,4,8")
    args = ap.parse_args()
    n_classes, shots = 100, 5
    with torch.no_grad():
        gal, res = build_gallery(n_classes, shots)
        g = torch.Generator(device="cuda").manual_seed(2)
        frames = torch.randn(B, 2 * PUSH, 3, res, res, device="cuda", generator=g)
        out = {"device": torch.cuda.get_device_name(0), "session": args.session,
               "method": "one process, both sides in it; HIP events; median of %d timed calls after warm-up calls" % args.reps,
               "arch": "ViT-B/16", "precision": "bf16", "T": T, "classes": n_classes, "shots": shots, "streams": B,
               "frames_per_push": PUSH, "points": []}
        for stride in [int(v) for v in args.strides.split(",")]:
            r = stride_point(gal, frames, stride, args.reps)
            print(json.dumps(r), flush=True)
            out["points"].append(r)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
