"""Time the live gallery on the GPU (run as a fresh process; HIP events around every step).

    python tools/live_gallery_time.py [--out profiles/live_gallery_time.json] [--reps 10] [--classes 2000]

1. cfsl_otam_indexed with identity cols and with a random permutation against cfsg_otam_gallery on the same data, at the six shapes of
   profiles/gallery_time.json.  The three legs alternate three times (dense, identity, permuted, dense, ...), every visit the median of
   `reps` launches after a warm-up launch; a leg's figure is the median of its three visits, and the spread of the dense leg's visits says
   what a ratio near 1 is worth.
2. the cost of mutation at `classes` classes x 5 shots (ViT-B/16 bf16, T = 8): LiveGallery add one class / remove one class / add one
   shot against SupportGallery.add_classes of one class at that size (the one of the three operations it has), and clear() +
   re-registration of everything, today's alternative for the other two, timed once.
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

SHAPES = [(NQ, C, T, E) for T, E in ((8, 512), (16, 768)) for NQ, C in ((1024, 24), (1024, 1024), (4096, 256))]


def kernel_point(NQ, C, T, E, reps, rounds=3):
    from clip_fsar_amd import gallery_hip as gh
    from clip_fsar_amd import live_hip as lh
    g = torch.Generator(device="cuda").manual_seed(NQ + C)
    base = torch.randn(E, device="cuda", generator=g)
    Xq = (base + torch.randn(NQ, T, E, device="cuda", generator=g)).contiguous()
    P = (base + torch.randn(C, T, E, device="cuda", generator=g)).contiguous()
    qn, pn = torch.empty(NQ * T, device="cuda"), torch.empty(C * T, device="cuda")
    gh.row_norms(Xq, qn)
    gh.row_norms(P, pn)
    perm = torch.randperm(C, device="cuda", generator=g)
    ident = torch.arange(C, device="cuda", dtype=torch.int32)
    Pp, pnp = torch.empty_like(P), torch.empty_like(pn)
    Pp[perm] = P                                            # column j lives in slot perm[j]
    pnp.view(C, T)[perm] = pn.view(C, T)
    permc = perm.to(torch.int32).contiguous()
    lg = [torch.empty(NQ, C, device="cuda") for _ in range(3)]
    legs = {"dense": lambda: gh.otam_gallery(Xq, qn, P, pn, lg[0]),
            "identity": lambda: lh.otam_indexed(Xq, qn, P, pn, ident, lg[1]),
            "permuted": lambda: lh.otam_indexed(Xq, qn, Pp, pnp, permc, lg[2])}
    visits = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            visits[k].append(_time_ms(fn, reps))
    torch.cuda.synchronize()
    ms = {k: statistics.median(v) for k, v in visits.items()}
    return {"NQ": NQ, "C": C, "T": T, "E": E, "dense_ms": round(ms["dense"], 4), "identity_ms": round(ms["identity"], 4),
            "permuted_ms": round(ms["permuted"], 4), "identity_over_dense": round(ms["identity"] / ms["dense"], 4),
            "permuted_over_dense": round(ms["permuted"] / ms["dense"], 4),
            "dense_visit_spread": round((max(visits["dense"]) - min(visits["dense"])) / ms["dense"], 4),
            "visits_ms": {k: [round(t, 4) for t in v] for k, v in visits.items()},
            "bit_equal": bool(torch.equal(lg[0], lg[1]) and torch.equal(lg[0], lg[2]))}


def _wall_ms(fn, reps, before=None):
    """median wall time of fn() with the device drained before and after (host work is part of a mutation's cost); before(): untimed"""
    ts = []
    for _ in range(reps + 1):
        if before is not None:
            before()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts[1:])


def mutation_cost(reps, n_classes, shots=5, batch=100):
    from types import SimpleNamespace as NS
    import clip_fsar_amd.synth as synth
    from clip_fsar_amd.gallery import SupportGallery
    from clip_fsar_amd.live_gallery import LiveGallery
    from clip_fsar_amd.models.base.few_shot import CNN_OTAM_CLIPFSAR
    T = 8
    n_test = n_classes + 8
    cfg = NS(VIDEO=NS(HEAD=NS(NAME="CNN_OTAM_CLIPFSAR", BACKBONE_NAME="ViT-B/16", PRECISION="bf16"), BACKBONE=NS(META_ARCH="Identity")),
             TRAIN=NS(CLASS_NAME=["c%d" % i for i in range(64)], WAY=5), TEST=NS(CLASS_NAME=["t%d" % i for i in range(n_test)]),
             DATA=NS(NUM_INPUT_FRAMES=T), MODEL=NS(NAME="BaseVideoModel", EMA=NS(ENABLE=False)), BN=NS(FREEZE=False), NUM_GPUS=1,
             NUM_SHARDS=1, RANDOM_SEED=18)
    head = CNN_OTAM_CLIPFSAR(cfg).eval()
    res = synth.ARCHS["ViT-B/16"]["res"]
    g = torch.Generator(device="cuda").manual_seed(1)
    V = torch.randn(batch * shots, T, 3, res, res, device="cuda", generator=g)     # one batch of videos serves every batch of classes

    def register(gal):
        for c0 in range(0, n_classes, batch):
            n = min(batch, n_classes - c0)
            gal.add_classes(V[:n * shots], [c0 + i // shots for i in range(n * shots)])

    new = n_classes                                         # the id of the class that comes and goes
    with torch.no_grad():
        sup, live = SupportGallery(head, "cuda"), LiveGallery(head, "cuda", capacity=n_classes + 64)
        register(sup)
        register(live)
        torch.cuda.synchronize()
        dense_P, dense_pn, dense_text = sup._P, sup._pn, sup._text

        def sup_restore():                                  # back to n_classes classes without re-registering
            sup._ids, sup._P, sup._pn, sup._text = list(range(n_classes)), dense_P, dense_pn, dense_text

        t_sup_add = _wall_ms(lambda: sup.add_classes(V[:shots], [new] * shots), reps, before=sup_restore)
        sup_restore()
        t_live_add = _wall_ms(lambda: live.add_classes(V[:shots], [new] * shots), reps,
                              before=lambda: live.remove_classes([new]) if new in live.class_ids else None)
        t_live_remove = _wall_ms(lambda: live.remove_classes([new]), reps,
                                 before=lambda: None if new in live.class_ids else live.add_classes(V[:shots], [new] * shots))
        if new in live.class_ids:
            live.remove_classes([new])
        t_live_shot = _wall_ms(lambda: live.add_shots(V[:1], [7]), reps)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sup.clear()
        register(sup)
        torch.cuda.synchronize()
        t_rereg = (time.perf_counter() - t0) * 1e3
    return {"arch": "ViT-B/16", "precision": "bf16", "T": T, "classes": n_classes, "shots": shots,
            "support_gallery_add_one_class_ms": round(t_sup_add, 3), "live_add_one_class_ms": round(t_live_add, 3),
            "live_remove_one_class_ms": round(t_live_remove, 4), "live_add_one_shot_ms": round(t_live_shot, 3),
            "clear_and_reregister_ms_once": round(t_rereg, 1),
            "add_class_live_over_support": round(t_live_add / t_sup_add, 3),
            "reregister_over_live_remove": round(t_rereg / t_live_remove, 1),
            "reregister_over_live_add_shot": round(t_rereg / t_live_shot, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "live_gallery_time.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--classes", type=int, default=2000)
    args = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "kernel": []}
    for NQ, C, T, E in SHAPES:
        r = kernel_point(NQ, C, T, E, args.reps)
        print(json.dumps(r), flush=True)
        out["kernel"].append(r)
    out["mutation"] = mutation_cost(args.reps, args.classes)
    print(json.dumps(out["mutation"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
