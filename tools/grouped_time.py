"""Time grouped scoring on the GPU (run as a fresh process; HIP events around every leg).

    python tools/grouped_time.py [--out profiles/grouped_time.json] [--reps 20]

32 groups of 8 windows, each against its own 100 of 3 200 registered classes (a random 100 per group, so the lists overlap), T = 8,
E = 512.  Three ways to the same 32 x [8, 100] logits:

  grouped   one cfgr_otam_grouped launch
  indexed   32 cfsl_otam_indexed launches, one per group
  union     one cfsl_otam_indexed launch of all 256 windows against the union of the lists, then the column gather that picks every
            group's 100 columns out of its rows

The legs alternate three times (grouped, indexed, union, grouped, ...), every visit the median of `reps` runs after a warm-up run; a leg's
figure is the median of its three visits, and the spread of the grouped leg's visits says what a ratio is worth.  The column lists and the
descriptor table are uploaded once, outside the timed region.  Nothing is asserted on time; the three results are compared for equality.
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

G, NQ_G, NC_G, CAP, T, E = 32, 8, 100, 3200, 8, 512


def measure(reps, rounds=3):
    from clip_fsar_amd import gallery_hip as gh
    from clip_fsar_amd import groups_hip as grh
    from clip_fsar_amd import live_hip as lh
    g = torch.Generator(device="cuda").manual_seed(G)
    base = torch.randn(E, device="cuda", generator=g)
    Xq = (base + torch.randn(G * NQ_G, T, E, device="cuda", generator=g)).contiguous()
    P = (base + torch.randn(CAP, T, E, device="cuda", generator=g)).contiguous()
    qn, pn = torch.empty(G * NQ_G * T, device="cuda"), torch.empty(CAP * T, device="cuda")
    gh.row_norms(Xq, qn)
    gh.row_norms(P, pn)
    lists = [torch.randperm(CAP, device="cuda", generator=g)[:NC_G].to(torch.int32).contiguous() for _ in range(G)]
    cols = torch.cat(lists).contiguous()
    rows, (nq, ncols, tiles, n_out) = grh.table_rows([NQ_G] * G, [NC_G] * G, T)
    table = grh.table_uploader("cuda", G).upload(rows)
    union, inverse = torch.unique(cols, return_inverse=True)                 # sorted slots; inverse: every list entry's column in the union
    union = union.to(torch.int32).contiguous()
    pick = inverse.view(G, 1, NC_G).expand(G, NQ_G, NC_G).contiguous()       # the union's column of every (group, window, class)
    out_g = torch.empty(n_out, device="cuda")
    out_i = torch.empty(G, NQ_G, NC_G, device="cuda")
    wide = torch.empty(G * NQ_G, union.shape[0], device="cuda")
    out_u = torch.empty(G, NQ_G, NC_G, device="cuda")

    def indexed():
        for i in range(G):
            lh.otam_indexed(Xq[i * NQ_G:(i + 1) * NQ_G], qn[i * NQ_G * T:(i + 1) * NQ_G * T], P, pn, lists[i], out_i[i])

    def by_union():
        lh.otam_indexed(Xq, qn, P, pn, union, wide)
        torch.gather(wide.view(G, NQ_G, -1), 2, pick, out=out_u)

    legs = {"grouped": lambda: grh.otam_grouped(Xq, qn, P, pn, cols, out_g, table, n_out), "indexed": indexed, "union": by_union}
    visits = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            visits[k].append(_time_ms(fn, reps))
    torch.cuda.synchronize()
    ms = {k: statistics.median(v) for k, v in visits.items()}
    return {"groups": G, "windows_per_group": NQ_G, "classes_per_group": NC_G, "registered_classes": CAP, "T": T, "E": E,
            "union_classes": int(union.shape[0]), "tiles": tiles, "grouped_ms": round(ms["grouped"], 4),
            "indexed_launches_ms": round(ms["indexed"], 4), "union_and_gather_ms": round(ms["union"], 4),
            "indexed_over_grouped": round(ms["indexed"] / ms["grouped"], 3), "union_over_grouped": round(ms["union"] / ms["grouped"], 3),
            "grouped_visit_spread": round((max(visits["grouped"]) - min(visits["grouped"])) / ms["grouped"], 4),
            "visits_ms": {k: [round(t, 4) for t in v] for k, v in visits.items()},
            "bit_equal": bool(torch.equal(out_g.view(G, NQ_G, NC_G), out_i) and torch.equal(out_i, out_u))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grouped_time.json"))
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "point": measure(args.reps)}
    print(json.dumps(out["point"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
