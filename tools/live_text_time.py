"""Time the grouped text kernels and the live text gallery on the GPU (run as a fresh process; HIP events around every step).

    python tools/live_text_time.py [--out profiles/live_text_time.json] [--reps 20] [--classes 2000]

1. at the shape of profiles/grouped_time.json -- 32 groups of 8 windows, each against its own 100 of 3 200 stored classes, E = 512 --
   one cflt_text_logits_grouped + cflt_text_softmax_grouped against the loop a caller of the dense library has: per group an
   index_select of its text rows and norms, cfgt_text_logits and cfgt_text_softmax.  The same for COMBINE (the OTAM logits are given: both
   legs read them).  Tables and slot lists are uploaded outside the timed region.  The legs alternate three times, every visit the median
   of `reps` runs after a warm-up; a leg's figure is the median of its visits.  The results of the two legs are compared for equality.
2. removing one class from `classes` registered ones (LiveTextGallery.remove_classes, wall time, COMBINE, ViT-B/16 bf16, 5 shots) against
   what a TextGallery has for it: clear() and the registration of all the others again, timed once.
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

GROUPS, WINDOWS, WIDTH, STORED, E = 32, 8, 100, 3200, 512


def kernel_legs(reps, rounds=3):
    from clip_fsar_amd import gallery_hip as gh
    from clip_fsar_amd import gallery_text_hip as gt
    from clip_fsar_amd import live_text_hip as lt
    g = torch.Generator(device="cuda").manual_seed(32)
    NQ = GROUPS * WINDOWS
    base = torch.randn(E, device="cuda", generator=g)
    emb = (base + torch.randn(NQ, E, device="cuda", generator=g)).contiguous()
    text = (base + torch.randn(STORED, E, device="cuda", generator=g)).contiguous()
    en, tn = torch.empty(NQ, device="cuda"), torch.empty(STORED, device="cuda")
    gh.row_norms(emb, en)
    gh.row_norms(text, tn)
    scale = torch.tensor([4.0], device="cuda")
    lists = [torch.randperm(STORED, device="cuda", generator=g)[:WIDTH] for _ in range(GROUPS)]
    cols = torch.cat(lists).to(torch.int32).contiguous()
    rows, (_, _, tiles, n_out, n_part) = lt.table_rows([WINDOWS] * GROUPS, [WIDTH] * GROUPS)
    table = lt.table_uploader("cuda", GROUPS).upload(rows)
    vis = -(4.0 + 8.0 * torch.rand(n_out, device="cuda", generator=g))
    out_g, out_l = torch.empty(n_out, device="cuda"), torch.empty(n_out, device="cuda")
    part_g = torch.empty(2 * n_part, device="cuda")
    part_l = torch.empty(gt.workspace_floats(WINDOWS, WIDTH), device="cuda")
    vis_l = [vis[i * WINDOWS * WIDTH:(i + 1) * WINDOWS * WIDTH].view(WINDOWS, WIDTH) for i in range(GROUPS)]

    def grouped(combine):
        lt.text_logits_grouped(emb, en, text, tn, cols, scale, out_g, part_g, table, n_out, n_part)
        if combine:
            lt.text_combine_grouped(out_g, part_g, vis, out_g, table, NQ, n_out, n_part, 0.9)
        else:
            lt.text_softmax_grouped(out_g, part_g, out_g, table, NQ, n_out, n_part)

    def loop(combine):
        for i, idx in enumerate(lists):
            o = out_l[i * WINDOWS * WIDTH:(i + 1) * WINDOWS * WIDTH].view(WINDOWS, WIDTH)
            q = slice(i * WINDOWS, (i + 1) * WINDOWS)
            gt.text_logits(emb[q], en[q], text.index_select(0, idx), tn.index_select(0, idx), scale, o, part_l)
            if combine:
                gt.text_combine(o, part_l, vis_l[i], o, 0.9)
            else:
                gt.text_softmax(o, part_l, o)

    res = {"groups": GROUPS, "windows_per_group": WINDOWS, "classes_per_group": WIDTH, "stored_classes": STORED, "E": E, "tiles": tiles}
    for mode, combine in (("eval_text", False), ("combine", True)):
        legs = {"grouped": lambda: grouped(combine), "loop": lambda: loop(combine)}
        visits = {k: [] for k in legs}
        for _ in range(rounds):
            for k, fn in legs.items():
                visits[k].append(_time_ms(fn, reps))
        torch.cuda.synchronize()
        ms = {k: statistics.median(v) for k, v in visits.items()}
        res[mode] = {"grouped_ms": round(ms["grouped"], 4), "loop_ms": round(ms["loop"], 4),
                     "loop_over_grouped": round(ms["loop"] / ms["grouped"], 2),
                     "visits_ms": {k: [round(t, 4) for t in v] for k, v in visits.items()},
                     "bit_equal": bool(torch.equal(out_g, out_l))}
    return res


def mutation_cost(n_classes, shots=5, batch=100):
    from types import SimpleNamespace as NS
    import clip_fsar_amd.synth as synth
    from clip_fsar_amd.live_text_gallery import LiveTextGallery
    from clip_fsar_amd.models.base.few_shot import CNN_OTAM_CLIPFSAR
    from clip_fsar_amd.text_gallery import TextGallery
    T = 8
    cfg = NS(VIDEO=NS(HEAD=NS(NAME="CNN_OTAM_CLIPFSAR", BACKBONE_NAME="ViT-B/16", PRECISION="bf16"), BACKBONE=NS(META_ARCH="Identity")),
             TRAIN=NS(CLASS_NAME=["c%d" % i for i in range(64)], WAY=5, COMBINE=True),
             TEST=NS(CLASS_NAME=["t%d" % i for i in range(n_classes + 8)]), DATA=NS(NUM_INPUT_FRAMES=T),
             MODEL=NS(NAME="BaseVideoModel", EMA=NS(ENABLE=False)), BN=NS(FREEZE=False), NUM_GPUS=1, NUM_SHARDS=1, RANDOM_SEED=18)
    head = CNN_OTAM_CLIPFSAR(cfg).eval()
    res = synth.ARCHS["ViT-B/16"]["res"]
    g = torch.Generator(device="cuda").manual_seed(1)
    V = torch.randn(batch * shots, T, 3, res, res, device="cuda", generator=g)     # one batch of videos serves every batch of classes
    Q = torch.randn(4, T, 3, res, res, device="cuda", generator=g)

    def register(gal, ids):
        for c0 in range(0, len(ids), batch):
            part = ids[c0:c0 + batch]
            gal.add_classes(V[:len(part) * shots], [part[i // shots] for i in range(len(part) * shots)])

    ids, gone = list(range(n_classes)), n_classes - 1           # the last one: the others keep their places in the batches, and so their videos
    with torch.no_grad():
        live, dense = LiveTextGallery(head, "cuda", capacity=n_classes + 64), TextGallery(head, "cuda")
        register(live, ids)
        register(dense, ids)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        live.remove_classes([gone])
        torch.cuda.synchronize()
        t_remove = (time.perf_counter() - t0) * 1e3
        rest = [c for c in ids if c != gone]
        t0 = time.perf_counter()
        dense.clear()
        register(dense, rest)
        torch.cuda.synchronize()
        t_rereg = (time.perf_counter() - t0) * 1e3
        equal = bool(torch.equal(live.classify(Q), dense.classify(Q))) and live.class_ids == dense.class_ids
    return {"arch": "ViT-B/16", "precision": "bf16", "T": T, "mode": "combine", "classes": n_classes, "shots": shots,
            "live_text_remove_one_class_ms_once": round(t_remove, 4), "text_gallery_clear_and_reregister_ms_once": round(t_rereg, 1),
            "reregister_over_remove": round(t_rereg / t_remove, 1), "classify_bit_equal_afterwards": equal}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "live_text_time.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--classes", type=int, default=2000)
    args = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "kernel": kernel_legs(args.reps)}
    print(json.dumps(out["kernel"]), flush=True)
    out["mutation"] = mutation_cost(args.classes)
    print(json.dumps(out["mutation"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
