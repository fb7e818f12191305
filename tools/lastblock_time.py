"""Time the last block's class-token attention on the GPU, folded and unfolded (run as a fresh process; HIP events around every leg).

    python tools/lastblock_time.py [--out profiles/lastblock_time.json] [--reps 20] [--frames 2880] [--arch b16|l14]

The shape bench.py runs: 2 880 frames of 197 tokens, D = 768, 12 heads (--arch l14: 257 tokens, D = 1 024, 16 heads), random data (a
zero-filled stream would flatter the softmax), statistics as the producer's partials.  Legs:

  key_fold, class_attend, value_fold   the three launches of libclipfsar_lastblock.so
  kv_gemm, attn_cls                    the two launches they replace: cfsar_gemm_lnfold_partials with N = 2 D, cfsar_vit_attention_cls
  row_stats                            cfsar_row_stats over the same rows: one read of the stream, the floor of class_attend

The legs alternate three times, every visit the median of `reps` runs after a warm-up run; a leg's figure is the median of its visits.
Nothing is asserted on time.
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

ARCHS = {"b16": (197, 12), "l14": (257, 16)}


def measure(reps, frames, arch, rounds=3):
    from clip_fsar_amd import hip
    from clip_fsar_amd import lastblock_hip as lb
    N, H = ARCHS[arch]
    D, F_ = 64 * H, frames
    M = F_ * N
    dev = torch.device("cuda")
    gen = torch.Generator(device="cuda").manual_seed(H)
    x = (torch.randn(M, D, device=dev, generator=gen) * 0.8 + 0.1).to(torch.float16)
    q = torch.randn(F_, D, device=dev, generator=gen).to(torch.bfloat16)
    wg = (torch.randn(3 * D, D, device=dev, generator=gen) / D ** 0.5).to(torch.float16)
    dvec = torch.randn(3 * D, device=dev, generator=gen) * 0.3
    cvec = wg.double().sum(1).float()
    xf = x.float().view(M, H, 64)
    part = torch.stack([xf.sum(2), (xf * xf).sum(2)], 2).contiguous()
    del xf
    rstat = torch.empty(M, 4, device=dev)
    wk_t = lb.key_weight(wg[D:2 * D], H)
    g, G = torch.empty(F_, H, D, device=dev, dtype=torch.float16), torch.empty(F_, H, device=dev)
    z, oc = torch.empty(F_, H, D, device=dev), torch.empty(F_, D, device=dev, dtype=torch.bfloat16)
    kv = torch.empty(M, 2 * D, device=dev, dtype=torch.bfloat16)
    legs = {
        "key_fold": lambda: lb.key_fold(q, wk_t, g, G),
        "class_attend": lambda: lb.class_attend(x, g, G, z, N, partial=part),
        "value_fold": lambda: lb.value_fold(z, wg[2 * D:], dvec[2 * D:], oc),
        "kv_gemm": lambda: hip.gemm_lnfold_partials(x, wg[D:], kv, cvec[D:], dvec[D:], part, H, rstat, M=M),
        "attn_cls": lambda: hip.vit_attention_cls(None, oc, F_, N, D, H, q=q, kv=kv),
        "row_stats": lambda: hip.row_stats(x, rstat, M, D),
    }
    visits = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            visits[k].append(round(_time_ms(fn, reps), 4))
    t = {k: statistics.median(v) for k, v in visits.items()}
    folded, unfolded = t["key_fold"] + t["class_attend"] + t["value_fold"], t["kv_gemm"] + t["attn_cls"]
    return {"frames": F_, "tokens": N, "D": D, "heads": H, "legs_ms": t, "folded_ms": round(folded, 4), "unfolded_ms": round(unfolded, 4),
            "saved_ms": round(unfolded - folded, 4), "class_attend_over_row_stats": round(t["class_attend"] / t["row_stats"], 3),
            "stream_bytes": M * D * 2, "visits_ms": visits}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--frames", type=int, default=2880)
    ap.add_argument("--arch", default="b16", choices=sorted(ARCHS))
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "point": measure(a.reps, a.frames, a.arch)}
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
