"""Time what LiveGallery(ledger=) costs an adding call, what remove_shots costs against the only remedy without it, and the audit (one
fresh process; HIP events, medians after warm-up; run it under a time limit of its own: `timeout -k 10 600 python tools/ledger_time.py`).

    python tools/ledger_time.py [--out profiles/ledger_time.json] [--reps 10] [--session NAME]

ViT-B/16 head, bf16, T = 8, E = 512, 2 000 classes registered from random tower features (the tower is not the subject), once into a
gallery with ledger=ShotLedger(shots=16384) and once into one without.  Three comparisons, the legs of each alternating three times in
this one process; what a timed call needs put back (the removed shot) is put back outside the timing:

  a. remove_shots of one shot from a class of five (the oldest; a fifth is added again before every timed call) against
     remove_classes + add_classes_features of the four others on the gallery without the option;
  b. add_shots_features of one clip to one class with and without the option: the cost of planning the slot and of cfld_put;
  c. shot_fit of one class of 8 shots, and shot_fits() of all 2 000 classes, each with its one synchronisation.

Recorded: the medians, the three alternations of every leg, the spreads; a loss is recorded as a loss.  Nothing is asserted on time.
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

from class_smooth_time import summary  # noqa: E402  (tools/class_smooth_time.py: the same summary)

T, C, SHOTS = 8, 2000, 16384
_HEAD = []


def build(ledger):
    from types import SimpleNamespace as NS
    from clip_fsar_amd.live_gallery import LiveGallery
    from clip_fsar_amd.models.base.few_shot import CNN_OTAM_CLIPFSAR
    cfg = NS(VIDEO=NS(HEAD=NS(NAME="CNN_OTAM_CLIPFSAR", BACKBONE_NAME="ViT-B/16", PRECISION="bf16"), BACKBONE=NS(META_ARCH="Identity")),
             TRAIN=NS(CLASS_NAME=["c%d" % i for i in range(64)], WAY=5), TEST=NS(CLASS_NAME=["t%d" % i for i in range(C)]),
             DATA=NS(NUM_INPUT_FRAMES=T), MODEL=NS(NAME="BaseVideoModel", EMA=NS(ENABLE=False)), BN=NS(FREEZE=False), NUM_GPUS=1,
             NUM_SHARDS=1, RANDOM_SEED=18)
    if not _HEAD:                                          # both galleries over one head
        _HEAD.append(CNN_OTAM_CLIPFSAR(cfg).eval())
    head = _HEAD[0]
    live = LiveGallery(head, "cuda", capacity=C + 64, **({"ledger": ledger} if ledger is not None else {}))
    g = torch.Generator(device="cuda").manual_seed(1)
    for c0 in range(0, C, 100):
        live.add_classes_features(torch.randn(100, T, live.E, device="cuda", generator=g), list(range(c0, c0 + 100)))
    return live


def timed(prepare, fn, reps):
    """median over reps timed calls of fn() (ms between HIP events), prepare() before each of them outside the timing; one warm-up"""
    ts = []
    for i in range(reps + 1):
        prepare()
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        if i:
            ts.append(s.elapsed_time(e))
    return statistics.median(ts)


def alternate(legs, reps, rounds=3):
    """{name: (prepare, fn)} -> {name: [median ms per round]}, the legs taking turns"""
    ts = {k: [] for k in legs}
    for _ in range(rounds):
        for k, (prepare, fn) in legs.items():
            ts[k].append(timed(prepare, fn, reps))
    return ts


def main():
    from clip_fsar_amd.ledger import ShotLedger
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ledger_time.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--session", default=time.strftime("%Y-%m-%d %H:%M:%S"), help="label of the measuring session, stored in the JSON")
    args = ap.parse_args()
    nothing = lambda: None
    with torch.no_grad():
        led, plain = build(ShotLedger(shots=SHOTS)), build(None)
        E = led.E
        g = torch.Generator(device="cuda").manual_seed(2)
        f = lambda n: torch.randn(n, T, E, device="cuda", generator=g)
        out = {"device": torch.cuda.get_device_name(0), "session": args.session,
               "method": "one process; HIP events; median of %d timed calls after a warm-up call; the legs of each comparison "
                         "alternating three times; spread = max - min of a leg's three medians; what a timed call consumes is put "
                         "back outside the timing" % args.reps,
               "arch": "ViT-B/16", "precision": "bf16", "T": T, "E": E, "classes": C, "ledger_shots": SHOTS,
               "addend_store_bytes": SHOTS * T * E * 4}
        # a. one shot out of a class of five
        four, one = f(4), f(1)
        for gal in (led, plain):
            gal.add_shots_features(four[1:], [7] * 3)          # class 7: four shots; the fifth comes and goes
        legs = {"remove_shots": (lambda: led.add_shots_features(one, [7]), lambda: led.remove_shots([led.shot_list(7)[0].serial])),
                "remove_classes_add_classes_features": (nothing, lambda: (plain.remove_classes([7]), plain.add_classes_features(four, [7] * 4)))}
        r = summary(alternate(legs, args.reps))
        out["remove"] = dict(r, shots_before=5, remove_shots_over_workaround=round(
            r["remove_shots"]["median_ms"] / r["remove_classes_add_classes_features"]["median_ms"], 3),
            note="the workaround also changes the class's column and its slot's generation: sessions reset; remove_shots does neither")
        print(json.dumps(out["remove"]), flush=True)
        # b. one further shot with and without the option
        legs = {"add_shots_features_with_ledger": (nothing, lambda: led.add_shots_features(one, [11])),
                "add_shots_features_without": (nothing, lambda: plain.add_shots_features(one, [11]))}
        r = summary(alternate(legs, args.reps))
        base = r["add_shots_features_without"]
        out["add"] = dict(r, ledger_minus_plain_ms=round(r["add_shots_features_with_ledger"]["median_ms"] - base["median_ms"], 5),
                          exceeds_the_spread_of_the_leg_without=bool(
                              r["add_shots_features_with_ledger"]["median_ms"] - base["median_ms"] > base["spread_ms"]),
                          bytes_cfld_put_moves=2 * T * E * 4)
        print(json.dumps(out["add"]), flush=True)
        # c. the audit
        led.add_shots_features(f(7), [21] * 7)                 # class 21: eight shots
        n_all = sum(len(v) for v in led.shot_fits().values())
        legs = {"shot_fit_one_class_of_8": (nothing, lambda: led.shot_fit(21)), "shot_fits_all_classes": (nothing, lambda: led.shot_fits())}
        r = summary(alternate(legs, args.reps))
        from clip_fsar_amd.live_gallery import TABLE_ROWS
        out["fit"] = dict(r, shots_audited_in_all=n_all, launches_for_all=-(-C // TABLE_ROWS),
                          bytes_read_for_all=n_all * T * E * 4 * 2)
        print(json.dumps(out["fit"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f_:
        json.dump(out, f_, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
