#!/usr/bin/env python3
"""Benchmark of the CLIP-FSAR episodic-inference hot path on MI355X.

    python bench.py --gpus N --steps K --warmup W [--episodes-per-step B] [--precision bf16|fp16|fp16_strict|fp32]
                    [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

`python bench.py --gpus N` with N > 1 and no launcher environment (WORLD_SIZE unset) spawns its own N ranks, one process per
GPU, the way the reference's launcher does (reference utils/launcher.py:29-34: torch.multiprocessing.spawn); under
torch.distributed.run the launcher's RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* are used as given.

Metric (BASELINE.json): episodes/sec, 5-way 1-shot, 8 frames, ViT-B/16 (config[1]: bf16 on MI355X, random-init CLIP
weights, synthetic frames).  One "step" = the full forward A0 -> A15 (+ top-1) over a batch of B synthetic episodes
that are already resident in HBM.  Episodes shard over ranks with no data-path collective (weak scaling: every rank
does K steps of B episodes); the only collective is ONE all-gather (RCCL) of the per-episode accuracies, inside the
timed region.  Rank 0 prints ONE JSON line: `metric`, `value` (episodes/s), `unit`, `higher_is_better`, `dtype` and
`ms_per_step` (wall time of one timed step) are the headline.  A plain run does only what that line needs: set-up, W warm-up
steps, K timed steps, the line.

--dump-outputs DIR  after the timed steps, rank 0 writes what its last timed step returned to a caller, as float32 .npy files:
                    logits.npy [B, queries, way], class_logits.npy [B, support + queries, train classes] and top1.npy [B] (the
                    per-episode top-1 accuracies).  Inputs and weights are seeded: the same arguments give the same inputs.
--full              everything else the line has carried, each measured as before:
  roofline     -- for the dominant kernel (the bf16 MFMA GEMM): algorithmic FLOPs of its launches / their measured
                  duration (HIP events on the launch stream, recorded live during the timed steps), against the dense
                  bf16 MFMA peak of MI355X (2.5 PFLOP/s, MI355X datasheet);
  parity       -- the first episode's logits against the reference-generated golden of the configuration;
  fp16_mode, strict_mode, configs -- short timed legs of the other 16-bit modes and of cfg3 / cfg4 (default bf16 cfg2 run);
  cpu_baseline -- the CPU oracle (torch fp32 restatement of the reference path, oracle/clipfsar_oracle.py) timed on the
                  host cores of this box on a bounded sample (rank 0, N = 1 only).
The --no-* switches below drop single pieces of a --full run.
"""
from __future__ import annotations

import argparse
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

import clip_fsar_amd.synth as synth  # noqa: E402

ARCH = "ViT-B/16"
WAY, SHOT, QPC, T = 5, 1, 1, 8
MERGE_BEFORE = False
N_TRAIN, N_TEST, SEED = 64, 24, 18
# algorithmic FLOPs (2 per MAC) of the ViT tower per frame (ViT-B/16: 35.127 G, ViT-L/14: 162.026 G)
GFLOP_PER_FRAME = 35.127
# --config selects another BASELINE config for reporting (the driver's default stays config[1] = cfg2)
CONFIGS = {
    "cfg2": dict(arch="ViT-B/16", shot=1, T=8, merge_before=False, gflop=35.127,
                 name="BASELINE config[1]: 5-way 1-shot, 1 query/class, 8x224^2 frames, ViT-B/16"),
    "cfg3": dict(arch="ViT-B/16", shot=5, T=8, merge_before=True, gflop=35.127,
                 name="BASELINE config[2]: 5-way 5-shot (MERGE_BEFORE), 1 query/class, 8x224^2 frames, ViT-B/16"),
    "cfg4": dict(arch="ViT-L/14", shot=1, T=16, merge_before=False, gflop=162.026,
                 name="BASELINE config[3]: 5-way 1-shot, 1 query/class, 16x224^2 frames, ViT-L/14 (extension A16)"),
    # N3: the backbone of every shipped reference config (configs/projects/CLIPFSAR/*: BACKBONE_NAME "RN50").
    # 11.997 GFLOP/frame = 2 x (5.367 GMAC convs + 0.631 GMAC attention pool), DESIGN.md (d).
    "rn50": dict(arch="RN50", shot=1, T=8, merge_before=False, gflop=11.997,
                 name="reference shipped backbone: 5-way 1-shot, 1 query/class, 8x224^2 frames, CLIP RN50"),
}
GEMM_KERNEL_NOTE = "16-bit MFMA GEMM kernels (QKV, out_proj, c_fc, c_proj: vit_gemm_kernel, csrc/gemm_vit.hip; patch embed: gemm.hip)"
PEAK_BF16_TFLOPS = 2500.0          # dense bf16 MFMA, MI355X_MICROARCH.md "Peak BF16/FP16 MFMA ~2.5 PF dense"


class GemmTimer:
    """Wraps the 16-bit MFMA GEMM entry points of clip_fsar_amd.hip (gemm, gemm_lnfold, gemm_lnfold_partials, gemm_residual_stats): brackets every
    launch with HIP events on the current stream (no host sync) and sums algorithmic FLOPs; durations are read after the
    timed region."""

    def __init__(self, hip_mod):
        self.hip = hip_mod
        self.events = []
        self.flops = 0.0
        self.launches = 0
        self.enabled = False
        self.k_div = 1               # fp16_strict: the patch-embed GEMM behind cfsar_im2col_patches_split executes 3 K passes of ONE algorithmic GEMM

    def install(self):
        def wrap(name):
            orig = getattr(self.hip, name)

            def timed(A, W, out, *a, **k):
                kd, self.k_div = self.k_div, 1
                if not (self.enabled and A.dtype in (torch.bfloat16, torch.float16)):
                    return orig(A, W, out, *a, **k)
                M = k.get("M") or A.shape[0]
                N = k.get("N") or W.shape[0]
                K = (k.get("K") or A.shape[1]) // kd             # of A: a split weight matrix is [N, 2K]; three-word patch rows count once
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                r = orig(A, W, out, *a, **k)
                e.record()
                self.events.append((s, e))
                self.flops += 2.0 * M * N * K
                self.launches += 1
                return r
            setattr(self.hip, name, timed)
        # engine.py binds `hip` as a module attribute, so patching the module functions is enough
        # _partials: + its finalize launch at batch scale; _hp / _wide: the fp16 numerics mode's forms (their tiny per-frame correction
        # GEMMs go through hip.corr_gemm and are not counted) (FLOPs stay the ALGORITHMIC
        # 2 M N K of the reference op: a split-weight launch executes twice that on the matrix cores)
        for name in ("gemm", "gemm_lnfold", "gemm_lnfold_partials", "gemm_residual_stats", "gemm_lnfold_hp", "gemm_residual_wide"):
            wrap(name)
        orig_split = self.hip.im2col_patches_split

        def split_marker(*a, **k):
            self.k_div = 3
            return orig_split(*a, **k)
        self.hip.im2col_patches_split = split_marker
        # the patch-embed GEMM that gathers its rows from the frames (cfsar_patch_embed): 2 x (frames x patches) x D x 3 P^2
        orig_pe = self.hip.patch_embed

        def timed_pe(frames, w, pos, cls, x, *a, **k):
            if not self.enabled:
                return orig_pe(frames, w, pos, cls, x, *a, **k)
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            r = orig_pe(frames, w, pos, cls, x, *a, **k)
            e.record()
            self.events.append((s, e))
            patch = k.get("patch", a[0] if a else 16)
            self.flops += 2.0 * frames.shape[0] * (pos.shape[0] - 1) * w.shape[0] * 3 * patch * patch      # algorithmic K = 3 P^2 (the 14 x 14 form walks 704 padded slots)
            self.launches += 1
            return r
        self.hip.patch_embed = timed_pe

    def result(self):
        ms = sum(s.elapsed_time(e) for s, e in self.events)
        return ms, self.flops, self.launches

    def reset(self):
        self.events, self.flops, self.launches = [], 0.0, 0


def csrc_fingerprint():
    """sha256 (16 hex digits) over the GEMM sources: a PMC profile is only quoted for the kernels it was taken on."""
    import hashlib
    h = hashlib.sha256()
    d = os.path.join(ROOT, "clip-fsar_amd", "csrc")
    for n in ("common.h", "gemm.hip", "gemm_vit.h", "gemm_vit_epi.h", "gemm_vit.hip"):
        with open(os.path.join(d, n), "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:16]


def measured_traffic(episodes_per_step):
    """(HBM bytes per 16-bit GEMM launch, provenance) from the newest committed rocprofv3 PMC profile (FETCH_SIZE and WRITE_SIZE in
    separate runs, FETCH_SIZE doubled per the gfx950 note in MI355X_MICROARCH.md; tools/collect_profiles.sh).  PMC collection cannot run
    inside the timed bench, so the value comes from profiles/ -- and is reported ONLY when the profile was taken at the same
    episodes-per-step AND on the GEMM sources of this tree (`csrc_sha16` recorded by collect_profiles.sh == csrc_fingerprint()); else
    null.  The provenance object names the file, its source fingerprint, commit and box either way."""
    src = {"file": None, "csrc_sha16_profile": None, "csrc_sha16_tree": csrc_fingerprint(), "matches_tree": False}
    try:
        names = sorted((n for n in os.listdir(os.path.join(ROOT, "profiles")) if re.fullmatch(r"r\d+_gemm_traffic\.json", n)), reverse=True)
        path = os.path.join(ROOT, "profiles", names[0])
        d = json.load(open(path))["_all_bf16_gemm"]
        src.update(file="profiles/" + names[0], csrc_sha16_profile=d.get("csrc_sha16"), commit=d.get("commit"), box=d.get("box"))
        src["matches_tree"] = d.get("csrc_sha16") == src["csrc_sha16_tree"]
        if src["matches_tree"] and re.search(r"--episodes-per-step %d\b" % episodes_per_step, d["note"]):
            return round(d["hbm_bytes_per_launch"]), src
    except Exception:
        pass
    return None, src


def _cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_baseline(sample_episodes: int = 5):
    """Oracle (kind "port") on the host cores of this box, bounded sample of the same workload (~30-40 s of CPU work).

    torch's intra-op pool does not scale on this path beyond a few tens of threads (on the 256-thread GPU-box host
    128 threads are 6x SLOWER than 16), so the thread count is calibrated first on a 4-frame ViT pass; the best candidate
    runs the timed episodes and is reported as `cores`.  The all-cores figure BASELINE.md section 4 asks for is reported
    next to it (`all_cores`), measured on one 8-frame ViT pass (the tower is 99.6 % of the reference's time)
    and scaled to the 80 frames of an episode, because whole episodes on every thread would take minutes."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import clipfsar_oracle as orc
    a = synth.ARCHS[ARCH]
    sd = {k: torch.from_numpy(v) for k, v in synth.head_state_dict(ARCH, SEED).items()}
    tt = torch.from_numpy(synth.text_features(N_TRAIN, a["embed"], "train", SEED))
    te = torch.from_numpy(synth.text_features(N_TEST, a["embed"], "test", SEED))
    ncpu = os.cpu_count() or 1
    ep0 = {k: torch.from_numpy(v) for k, v in synth.make_episode(WAY, SHOT, QPC, T, a["res"], N_TEST, 0, SEED).items()}
    frames_per_ep = (WAY * SHOT + WAY * QPC) * T
    best_t, best_dt = 1, float("inf")
    with torch.no_grad():
        for th in sorted({min(ncpu, c) for c in (8, 16, 32, 64)}):
            torch.set_num_threads(th)
            orc.vit_forward(ep0["support_set"][:2], sd, a)                      # warm the pool
            t0 = time.perf_counter()
            orc.vit_forward(ep0["support_set"][:4], sd, a)
            dt = time.perf_counter() - t0
            if dt < best_dt:
                best_t, best_dt = th, dt
        torch.set_num_threads(best_t)
        times = []
        for e in range(sample_episodes):
            ep = {k: torch.from_numpy(v) for k, v in synth.make_episode(WAY, SHOT, QPC, T, a["res"], N_TEST, e, SEED).items()}
            t0 = time.perf_counter()
            orc.head_forward(ep, sd, tt, te, a, frames=T)
            times.append(time.perf_counter() - t0)
        all_cores = None
        if ncpu != best_t:
            torch.set_num_threads(ncpu)
            orc.vit_forward(ep0["support_set"][:2], sd, a)
            t0 = time.perf_counter()
            orc.vit_forward(ep0["support_set"][:8], sd, a)
            dt = (time.perf_counter() - t0) * frames_per_ep / 8.0
            all_cores = {"cores": ncpu, "value": round(1.0 / dt, 4), "unit": "episodes/s",
                         "sample": "one 8-frame ViT-B/16 pass on all %d threads, scaled to %d frames" % (ncpu, frames_per_ep)}
        torch.set_num_threads(best_t)
    med = sorted(times)[len(times) // 2]
    return {"value": round(1.0 / med, 4), "unit": "episodes/s", "cores": best_t, "kind": "port", "cpu_model": _cpu_model(),
            "host_threads": ncpu, "all_cores": all_cores,
            "sample": "torch-fp32 CPU oracle (restatement of the reference path), %d timed cfg2 episodes (5-way 1-shot, "
                      "8x224^2 frames, ViT-B/16) after a thread-count calibration pass; %d of %d host threads used; "
                      "median %.2f s/episode (min %.2f, max %.2f)" % (sample_episodes, best_t, ncpu, med, min(times), max(times))}


GOLDEN_FILE = {"cfg2": "head_cfg2_B16_5w1s_T8.npz", "cfg3": "head_cfg3_B16_5w5s_T8_mb.npz", "cfg4": "head_cfg4_L14_5w1s_T16.npz"}


def golden_parity(logits0, precision, config="cfg2"):
    """Rank 0's first pooled episode (seed 18, episode id 0) is the configuration's golden case generated from the
    reference itself (oracle/make_golden.py): compare the logits this run produced, in the configuration it timed."""
    path = os.path.join(ROOT, "tests", "golden", GOLDEN_FILE[config])
    try:
        import numpy as np
        z = np.load(path)
        ref = torch.from_numpy(z["logits"])
    except Exception as exc:                                         # fixture missing: say so, do not guess
        return {"checked": False, "reason": "golden fixture unavailable: %s" % exc}
    got = logits0.detach().float().cpu()
    if tuple(got.shape) != tuple(ref.shape):
        return {"checked": False, "reason": "shape %s vs golden %s" % (tuple(got.shape), tuple(ref.shape))}
    d = float((got - ref).abs().max())
    from clip_fsar_amd import FP16_TAIL_MAX_SEEN, LOGITS_STATISTIC, LOGITS_TOLERANCE, NORTH_STAR_TOLERANCE
    tol = LOGITS_TOLERANCE[precision]
    return {"checked": True, "against": "tests/golden/%s (reference fp32 logits)" % GOLDEN_FILE[config],
            "max_abs_dlogits": round(d, 6), "argmax_equal": bool(torch.equal(got.argmax(1), ref.argmax(1))),
            "north_star_tolerance": NORTH_STAR_TOLERANCE, "meets_north_star": bool(d < NORTH_STAR_TOLERANCE),
            "tolerance": tol, "within_tolerance": bool(d < tol),
            "scope": "ONE golden episode (%d logits).  What the mode guarantees over many episodes: `contract`" % ref.numel(),
            "contract": {"fp32": "hard bound: every logit of every episode within 1e-3 (measured <= 7.6e-6)",
                         "fp16": "statistic, not a bound: rms <= %g and p99 <= %g of |dlogits| over 65 reference logit rows per configuration, standard "
                                 "and high-contrast episodes (measured rms 1.9-3.5e-4, p99 4.6-9.0e-4); an episode's largest deviation exceeds 1e-3 in about one "
                                 "episode of 13-60 (max seen %.3g)" % (LOGITS_STATISTIC["fp16"]["rms"], LOGITS_STATISTIC["fp16"]["p99"], FP16_TAIL_MAX_SEEN),
                         "fp16_strict": "bound on the reference's goldens: every one of the 455 logit rows of the six 13-episode ViT sets (standard / high contrast, "
                                        "5-shot, ViT-L/14, outlier channels) within 1e-3, no episode over (tests/test_gpu_e2e.py::"
                                        "test_strict_mode_every_reference_golden_row_inside_1e3); fresh episodes: profiles/r06_strict_eval.md",
                         "bf16": "throughput mode, NOT inside 1e-3: rms 2.3-3.9e-3, max 1.0e-2 over 65 rows per configuration"}[precision],
            "tolerance_note": "this mode's own regression bound on the full-size configurations (profiles/r05_parity_table.md, "
                              "tests/test_gpu_e2e.py::test_modes_against_multi_episode_reference_goldens); the north-star bound is 1e-3"}


def default_episodes_per_step(cfgname, dry=False):
    """The batch the product harness itself picks for a config without TEST.EPISODES_PER_STEP (datasets/base/builder.py::auto_episodes_per_step):
    ViT towers -> clip_fsar_amd.utils.batching (full rounds of the persistent GEMM grid within 2 880 frames and the 32-bit offset limit), RN50 -> what
    2 560 frames hold (32)."""
    if dry:
        return 16
    from clip_fsar_amd.utils.batching import FRAME_CAP, pick_episodes_per_step
    c = CONFIGS[cfgname]
    a = synth.ARCHS[c["arch"]]
    if a.get("kind") == "rn":
        return max(1, 2560 // ((WAY * c["shot"] + WAY * QPC) * c["T"]))     # datasets/base/builder.py: RN_FRAME_CAP
    ntok = (a["res"] // a["patch"]) ** 2 + 1
    fpe = (WAY * c["shot"] + WAY * QPC) * c["T"]
    return pick_episodes_per_step(fpe, ntok, a["width"], max_frames=min(FRAME_CAP, (2 ** 32 - 1) // (ntok * 4 * a["width"] * 2) - 1))


def executed_gflop_per_frame(arch, gflop, pruned):
    """the last ViT block is computed for the class-token rows only (engine.py: prune_last; few_shot.py:683 reads nothing else of it):
    (N - 1) (20 D^2 + 4 N D) FLOPs per frame fewer than the reference path's figure"""
    if not (pruned and arch.startswith("ViT")):
        return gflop
    a_ = synth.ARCHS[arch]
    n_, d_ = (a_["res"] // a_["patch"]) ** 2 + 1, a_["width"]
    return gflop - (n_ - 1) * (20.0 * d_ * d_ + 4.0 * n_ * d_) / 1e9


def timed_leg(cfgname, precision, B, steps, dev, timer, weights=None, batches=None, distinct=2, vit_options=None, kernel_events=True):
    """A short extra measurement inside the default run: `steps` timed steps of B episodes of configuration
    `cfgname` in `precision` after two warm-up steps, with the GEMM launches' HIP events (-> roofline) and the configuration's golden
    parity (its first episode is the golden case).  `batches`: resident steps to reuse (the headline's); else `distinct` episodes are
    generated and tiled to B per step.  `vit_options`: developer ablations (tools/fp16_stream_time.py), never set by this file; `kernel_events` False (--no-kernel-events): no
    HIP events around the launches, no roofline object.  Returns the leg's object."""
    from clip_fsar_amd import hip
    from clip_fsar_amd.engine import ClipFsarEngine
    c = CONFIGS[cfgname]
    a = synth.ARCHS[c["arch"]]
    fpe = (WAY * c["shot"] + WAY * QPC) * c["T"]
    if weights is None:
        weights = ({k: torch.from_numpy(v) for k, v in synth.head_state_dict(c["arch"], SEED).items()},
                   synth.text_features(N_TRAIN, a["embed"], "train", SEED), synth.text_features(N_TEST, a["embed"], "test", SEED))
    sd, tt, te = weights
    eng = ClipFsarEngine(a, sd, tt, te, precision=precision, device=dev, max_frames=max(1280, B * fpe), vit_options=vit_options)
    keys = (("sup", "support_set"), ("tgt", "target_set"), ("sl", "support_labels"), ("rl", "real_support_labels"))
    if batches is None:
        eps = [synth.make_episode(WAY, c["shot"], QPC, c["T"], a["res"], N_TEST, i, SEED) for i in range(distinct)]
        dev_eps = [{k: torch.from_numpy(e[src]).to(dev) for k, src in keys} for e in eps]
        batches = [{k: torch.stack([dev_eps[i % distinct][k] for i in range(B)]) for k, _ in keys}]
        del dev_eps
    lg0 = None
    for i in range(2 + steps):
        if i == 2:
            torch.cuda.synchronize()
            if timer is not None:
                timer.reset()
                timer.enabled = kernel_events
            t1 = time.perf_counter()
        b = batches[i % len(batches)]
        lg, _ = eng.forward(b["sup"], b["tgt"], b["sl"], b["rl"], way=WAY, T=c["T"], merge_before=c["merge_before"])
        if i == 0:
            lg0 = lg
    torch.cuda.synchronize()
    dt = time.perf_counter() - t1
    eps_per_s = steps * B / dt
    gexec = executed_gflop_per_frame(c["arch"], c["gflop"], getattr(getattr(eng, "vit", None), "prune_last", False))
    e2e = eps_per_s * gexec * fpe / 1e3
    leg = {"config": cfgname, "precision": precision, "value": round(eps_per_s, 3), "unit": "episodes/s", "steps": steps,
           "episodes_per_step": B, "ms_per_step": round(dt / steps * 1e3, 4), "frames_per_episode": fpe,
           "tflop_per_episode_executed": round(gexec * fpe / 1e3, 4)}
    if timer is not None:
        timer.enabled = False
        if timer.launches:
            ms, flops, n = timer.result()
            ach = flops / (ms * 1e-3) / 1e12
            leg["roofline"] = {"bound": "mfma", "achieved": round(ach, 2), "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s",
                               "frac": round(ach / PEAK_BF16_TFLOPS, 4), "frac_end_to_end": round(e2e / PEAK_BF16_TFLOPS, 4),
                               "launches": n, "avg_launch_us": round(ms * 1e3 / n, 2), "traffic": None,
                               "frac_scope": "dominant kernel only: the 16-bit MFMA GEMM launches of this leg (HIP events)"}
    leg["parity"] = golden_parity(lg0[0], precision, cfgname) if cfgname in GOLDEN_FILE else {"checked": False, "reason": "config has no in-bench golden"}
    del eng
    torch.cuda.empty_cache()
    return leg


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--episodes-per-step", type=int, default=0,
                    help="episodes per step and GPU; 0 (default) = the product harness's own choice (clip_fsar_amd.utils.batching: the batch that fills the "
                         "rounds of the persistent GEMM grid, 36 for cfg2, 12 for cfg3, 11 for cfg4; RN50: 32)")
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp16", "fp16_strict", "fp32"])
    ap.add_argument("--pool", type=int, default=0, help="distinct synthetic episodes resident in HBM per rank (0 = one per slot of a step: "
                                                        "every step holds episodes-per-step DISTINCT episodes)")
    ap.add_argument("--inputs", default="resident", choices=["resident", "host"],
                    help="host: additionally time the same steps with the episodes in pinned HOST memory -- uploaded on the compute stream "
                         "before every step (serial) and by the product harness's double-buffered copy stream (overlapped); `value` stays the "
                         "resident figure")
    ap.add_argument("--config", default="cfg2", choices=sorted(CONFIGS))
    ap.add_argument("--full", action="store_true",
                    help="also measure and check what the headline does not need: roofline (per-launch HIP events), golden parity, the fp16 / "
                         "fp16_strict legs, the cfg3 / cfg4 legs and the CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's outputs (logits, class_logits, per-episode top-1) as float32 DIR/<name>.npy")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: skip the CPU baseline")
    ap.add_argument("--no-kernel-events", action="store_true", help="--full: no HIP events around the GEMM launches, no roofline object")
    ap.add_argument("--no-fp16-leg", action="store_true", help="--full: skip the extra fp16-mode and fp16_strict-mode measurements of the bf16 run")
    ap.add_argument("--no-config-legs", action="store_true", help="--full: skip the short cfg3 / cfg4 legs (bf16 and fp16)")
    ap.add_argument("--dev-gemm-variant", default=None,
                    help="developer A/B only (needs CFSAR_DEV_LIB=1): 'variant[:dbg]' forced on every 16-bit GEMM, e.g. 13 = p12")
    ap.add_argument("--rendezvous-timeout", type=int, default=300,
                    help="seconds a rank waits for the others at the process-group rendezvous and at the pre-timing check-in before it "
                         "names the missing ranks and exits (a dead rank must not hang an 8-GPU run)")
    ap.add_argument("--job-timeout", type=int, default=3600, help="self-spawn only: seconds before the parent kills ranks that never finished")
    ap.add_argument("--dry-run", action="store_true",
                    help="CPU / gloo rehearsal of the launch + collective + timing protocol with a no-op step "
                         "(tests/test_distributed_gloo.py); prints a line marked dry_run, never a benchmark result")
    args = ap.parse_args(argv)
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    return args


def _spawn_entry(local_rank, world, port, argv):
    os.environ.update(RANK=str(local_rank), LOCAL_RANK=str(local_rank), WORLD_SIZE=str(world),
                      MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")         # dmabuf IPC: RCCL needs it on this driver
    run(parse_args(argv))


def _free_port():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def main(argv=None):
    args = parse_args(argv)
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # no launcher: one process per GPU, spawned here (reference utils/launcher.py:29-34)
        import torch.multiprocessing as mp
        ctx = mp.spawn(_spawn_entry, args=(args.gpus, _free_port(), sys.argv[1:] if argv is None else list(argv)),
                       nprocs=args.gpus, join=False)
        deadline = time.time() + args.job_timeout
        while not ctx.join(timeout=5):                   # raises as soon as one rank failed (and terminates the others)
            if time.time() > deadline:
                alive = [i for i, p in enumerate(ctx.processes) if p.is_alive()]
                for p in ctx.processes:
                    if p.is_alive():
                        p.terminate()
                raise SystemExit("bench.py: rank(s) %s still running after %d s -- killed" % (alive, args.job_timeout))
        return
    run(args)


def _checkin(tag, rank, world, timeout_s):
    """Every rank posts `tag` in the rendezvous store and waits for every other rank's post: a rank that died (or never got its GPU)
    is NAMED after `timeout_s` seconds instead of hanging the collective that follows."""
    import datetime
    store = dist.distributed_c10d._get_default_store()
    store.set("%s/%d" % (tag, rank), "1")
    missing = []
    for r in range(world):
        try:
            store.wait(["%s/%d" % (tag, r)], datetime.timedelta(seconds=timeout_s if not missing else 1))
        except Exception:
            missing.append(r)
    if missing:
        raise SystemExit("bench.py rank %d: rank(s) %s did not reach '%s' within %d s" % (rank, missing, tag, timeout_s))


class _CollectiveWatchdog:
    """The timed region ends in the path's one collective.  A rank that died or hangs inside its steps would leave the others waiting in it
    (RCCL: until the process-group watchdog tears the job down, naming nobody).  Every rank posts `<tag>/<rank>` in the rendezvous store (a
    non-blocking set) right before it enters the collective; if the collective has not returned after `timeout_s` seconds this timer thread
    reads which ranks never posted, names them on stderr and ends the process with a non-zero code."""

    def __init__(self, tag, rank, world, timeout_s):
        import threading
        self.tag, self.rank, self.world, self.timeout_s = tag, rank, world, timeout_s
        self.store = dist.distributed_c10d._get_default_store()
        self.store.set("%s/%d" % (tag, rank), "1")
        self.timer = threading.Timer(timeout_s, self._fire)
        self.timer.daemon = True
        self.timer.start()

    def missing(self):
        out = []
        for r in range(self.world):
            try:
                if not self.store.check(["%s/%d" % (self.tag, r)]):
                    out.append(r)
            except Exception:
                return "unknown (the rendezvous store on rank 0 is unreachable: rank 0 is gone)"
        return out

    def _fire(self):
        sys.stderr.write("bench.py rank %d: the timed collective did not complete within %d s -- rank(s) %s never reached it\n" % (
            self.rank, self.timeout_s, self.missing()))
        sys.stderr.flush()
        os._exit(3)

    def cancel(self):
        self.timer.cancel()


def run(args):
    global ARCH, SHOT, T, MERGE_BEFORE, GFLOP_PER_FRAME
    cfgsel = CONFIGS[args.config]
    ARCH, SHOT, T, MERGE_BEFORE, GFLOP_PER_FRAME = cfgsel["arch"], cfgsel["shot"], cfgsel["T"], cfgsel["merge_before"], cfgsel["gflop"]
    if args.config != "cfg2":
        args.no_cpu_baseline = True            # the CPU leg is defined on the headline config only
    full = args.full

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus > 1 and world != args.gpus:
        raise SystemExit("--gpus %d but the launcher exported WORLD_SIZE=%d" % (args.gpus, world))
    dry = args.dry_run
    if not dry and not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the hot path has no CPU fallback")
    if dry:
        dev = torch.device("cpu")
    else:
        if local_rank >= torch.cuda.device_count():
            raise SystemExit("rank %d: LOCAL_RANK %d but only %d GPU(s) visible" % (rank, local_rank, torch.cuda.device_count()))
        torch.cuda.set_device(local_rank)
        dev = torch.device("cuda", local_rank)
    sync = (lambda: None) if dry else torch.cuda.synchronize
    use_dist = world > 1 or os.environ.get("CFSAR_BENCH_FORCE_DIST") == "1"    # the flag exercises the RCCL path at N=1
    if use_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        os.environ.setdefault("RANK", str(rank))
        os.environ.setdefault("WORLD_SIZE", str(world))
        import datetime
        pg_timeout = datetime.timedelta(seconds=max(args.rendezvous_timeout, 30))
        try:
            if dry:
                dist.init_process_group(backend="gloo", timeout=pg_timeout)
            else:
                dist.init_process_group(backend="nccl", device_id=dev, timeout=pg_timeout)   # "nccl" on ROCm == RCCL over xGMI
        except Exception as exc:
            raise SystemExit("bench.py rank %d of %d: process-group rendezvous at %s:%s failed within %d s: %s" % (
                rank, world, os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"], args.rendezvous_timeout, exc))

    frames_per_ep = (WAY * SHOT + WAY * QPC) * T
    B = args.episodes_per_step or default_episodes_per_step(args.config, dry)
    timer = None
    first_logits = {}
    last = {}                                                        # what the last step returned (--dump-outputs)
    if dry:
        def step(i, acc_out):                                        # no-op stand-in: protocol rehearsal only
            acc_out[i * B:(i + 1) * B] = float(rank)
            last["top1"] = acc_out[i * B:(i + 1) * B]
    else:
        from clip_fsar_amd import hip
        from clip_fsar_amd.engine import ClipFsarEngine
        hip.lib()
        if args.dev_gemm_variant:
            v = [int(x) for x in (args.dev_gemm_variant.split(":") + ["0"])[:2]]
            hip.lib().cfsar_debug_set_gemm_variant(v[0], v[1])
        a = synth.ARCHS[ARCH]
        # identical weights on every rank, built locally (no broadcast needed), and the synthetic episodes of this rank (episode ids e
        # with e % world == rank).  Both are pure functions of their seeds; numpy releases the GIL in the generators, so a few threads
        # build the same arrays several times faster than one.
        npool = args.pool if args.pool > 0 else B
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(8) as ex:
            sd_job = ex.submit(synth.head_state_dict, ARCH, SEED)
            pool = list(ex.map(lambda i: synth.make_episode(WAY, SHOT, QPC, T, a["res"], N_TEST, rank + world * i, SEED), range(npool)))
            sd = {k: torch.from_numpy(v) for k, v in sd_job.result().items()}
        tt = synth.text_features(N_TRAIN, a["embed"], "train", SEED)
        te = synth.text_features(N_TEST, a["embed"], "test", SEED)
        eng = ClipFsarEngine(a, sd, tt, te, precision=args.precision, device=dev, max_frames=max(1280, B * frames_per_ep))
        # resident in HBM before timing: every step holds B DISTINCT episodes (each uploaded once; the steps cycle through a few
        # rotations of the pool)
        keys = (("sup", "support_set"), ("tgt", "target_set"), ("sl", "support_labels"), ("rl", "real_support_labels"), ("tl", "target_labels"))
        dev_eps = [{k: torch.from_numpy(e[src]).to(dev) for k, src in keys} for e in pool]
        batches = []
        for j in range(min(npool, 4)):
            eps = [dev_eps[(j + i) % npool] for i in range(B)]
            batches.append({k: torch.stack([e[k] for e in eps]) for k, _ in keys})
        del dev_eps

        if rank == 0 and full:                                       # per-launch events and the CPU leg: rank 0 only
            timer = GemmTimer(hip)
            timer.install()

        def step(i, acc_out):
            b = batches[i % len(batches)]
            logits, class_logits = eng.forward(b["sup"], b["tgt"], b["sl"], b["rl"], way=WAY, T=T, merge_before=MERGE_BEFORE)
            # A17: per-episode top-1 accuracy (metrics.topks_correct semantics, reference utils/metrics.py:100-138)
            hip.episode_top1(logits, b["tl"], acc_out[i * B:(i + 1) * B])
            if i % len(batches) == 0:
                first_logits["v"] = logits                           # batch 0, kept for the post-run parity check
            last.update(logits=logits, class_logits=class_logits, top1=acc_out[i * B:(i + 1) * B])

    acc = torch.zeros(max(args.steps, args.warmup, 1) * B, device=dev)
    for i in range(args.warmup):
        step(i, acc)
    sync()
    if use_dist:
        _checkin("warm", rank, world, args.rendezvous_timeout)      # engines built, warm-up done on EVERY rank -- or say which is missing
        dist.barrier()
    sync()
    # --full: HIP events around every GEMM launch of the timed region (the roofline object).  Small batches run the tower as two concurrent
    # chains on two streams, where ~200 timing events per episode serialise the chains (measured: 3.97 -> 5.64 ms per episode):
    # there the events bracket the launches of every 5th step only; the value is still the time of ALL timed steps.
    event_every = 1 if (dry or B * frames_per_ep > 160) else 5
    t0 = time.perf_counter()
    for i in range(args.steps):
        if timer is not None:
            timer.enabled = (not args.no_kernel_events) and i % event_every == 0
        step(i, acc)
    gathered = acc[:args.steps * B]
    if dry and os.environ.get("CFSAR_BENCH_TEST_HANG_RANK") == str(rank):      # dry runs only (tests/test_bench_contract.py): a rank that
        time.sleep(3600)                                                        # never leaves its timed steps
    if use_dist:                                                     # the path's single collective
        wd = _CollectiveWatchdog("timed", rank, world, args.rendezvous_timeout)
        try:
            allacc = torch.empty(world * args.steps * B, device=dev)
            dist.all_gather_into_tensor(allacc, gathered.contiguous())
            gathered = allacc
            sync()
            dist.barrier()
        except Exception as exc:                                     # gloo reports a dead peer at once: say WHICH rank is missing
            raise SystemExit("bench.py rank %d: the timed collective failed (%s) -- rank(s) %s never reached it" % (rank, exc, wd.missing()))
        finally:
            wd.cancel()
    sync()
    elapsed = time.perf_counter() - t0
    main_gemm = None
    if timer is not None:
        timer.enabled = False
        if timer.launches:
            main_gemm = timer.result()              # read NOW: the extra legs below reuse (and reset) the timer
    rank_elapsed = [elapsed]
    collective = None
    if use_dist:
        tall = torch.zeros(world, device=dev, dtype=torch.float64)
        dist.all_gather_into_tensor(tall, torch.tensor([elapsed], device=dev, dtype=torch.float64))      # outside the timed region
        rank_elapsed = [float(v) for v in tall.tolist()]
        elapsed = max(rank_elapsed)                                  # MAX over ranks
        # what the timed all-gather really spanned: the gathered tensor holds world x steps x B accuracies
        collective = {"backend": dist.get_backend(), "rccl_world_size": int(gathered.numel() // max(1, args.steps * B)),
                      "gathered_elements": int(gathered.numel())}

    if args.dump_outputs and rank == 0:                              # the last timed step's results, before anything else runs
        import numpy as np
        os.makedirs(args.dump_outputs, exist_ok=True)
        for name, v in last.items():
            if v is not None:
                np.save(os.path.join(args.dump_outputs, name + ".npy"), v.detach().float().cpu().numpy())

    host_inputs = None
    if args.inputs == "host" and not dry:
        # The same steps with the episodes in pinned HOST memory (the C ABI takes device pointers; `value` above is the resident
        # figure).  serial: uploaded on the compute stream in front of every step; overlapped: the product harness's copy-stream
        # double buffer (clip_fsar_amd.utils.prefetch.DevicePrefetcher, used by runs/test_net_few_shot.py::test_epoch).
        from clip_fsar_amd.utils.prefetch import DevicePrefetcher
        hb = [{k: v.cpu().pin_memory() for k, v in b.items()} for b in batches]
        nbytes = sum(v.numel() * v.element_size() for v in hb[0].values())

        def run_host(overlapped):
            it = (hb[i % len(hb)] for i in range(args.steps))
            sync()
            t1 = time.perf_counter()
            if overlapped:
                for i, b in enumerate(DevicePrefetcher(it, dev)):
                    eng.forward(b["sup"], b["tgt"], b["sl"], b["rl"], way=WAY, T=T, merge_before=MERGE_BEFORE)
            else:
                for b in it:
                    d = {k: v.to(dev, non_blocking=True) for k, v in b.items()}
                    eng.forward(d["sup"], d["tgt"], d["sl"], d["rl"], way=WAY, T=T, merge_before=MERGE_BEFORE)
            sync()
            return time.perf_counter() - t1
        run_host(True)                                               # warm both paths (buffer allocation)
        t_ser, t_ovl = run_host(False), run_host(True)
        host_inputs = {"bytes_per_step": nbytes, "pinned": True,
                       "serial_episodes_per_s": round(args.steps * B / t_ser, 3), "overlapped_episodes_per_s": round(args.steps * B / t_ovl, 3),
                       "note": "per rank; serial = upload on the compute stream before each step, overlapped = copy-stream double buffer "
                               "(utils/prefetch.py, the product harness's path)"}

    fp16_mode = None
    strict_mode = None
    config_legs = None
    if (full and not dry and rank == 0 and world == 1 and args.precision == "bf16" and not args.no_fp16_leg
            and B * frames_per_ep > 160):              # (small steps: a handful of them does not time anything)
        # The 16-bit mode that meets the north-star tolerance on the goldens (precision "fp16": IEEE-half operands everywhere, same kernels), timed
        # in the same process on the same resident steps: `value` stays BASELINE's bf16 configuration, this object says what the
        # conforming mode costs and where its GEMMs sit on the roofline.  `python bench.py --precision fp16` makes it the headline instead.
        fp16_mode = timed_leg(args.config, "fp16", B, max(4, min(args.steps, 10)), dev, timer, weights=(sd, tt, te), batches=batches,
                              kernel_events=not args.no_kernel_events)
        # ... and the 16-bit mode whose contract is a BOUND on the reference's goldens (precision "fp16_strict", round 6), same steps
        if ARCH.startswith("ViT"):
            strict_mode = timed_leg(args.config, "fp16_strict", B, max(4, min(args.steps, 10)), dev, timer, weights=(sd, tt, te), batches=batches,
                                    kernel_events=not args.no_kernel_events)
    if (full and not dry and rank == 0 and world == 1 and args.precision == "bf16" and args.config == "cfg2" and not args.no_config_legs
            and B * frames_per_ep > 160):
        # BASELINE configs[2..3] in front of the driver: 3 timed steps of the harness's batch (12 / 11 episodes), bf16, fp16 and fp16_strict, with golden parity
        config_legs = {}
        for cname in ("cfg3", "cfg4"):
            cc = CONFIGS[cname]
            w = (sd, tt, te) if cc["arch"] == ARCH else None
            if w is None:
                aa = synth.ARCHS[cc["arch"]]
                w = ({k: torch.from_numpy(v) for k, v in synth.head_state_dict(cc["arch"], SEED).items()},
                     synth.text_features(N_TRAIN, aa["embed"], "train", SEED), synth.text_features(N_TEST, aa["embed"], "test", SEED))
            for prec in ("bf16", "fp16", "fp16_strict"):
                config_legs["%s_%s" % (cname, prec)] = timed_leg(cname, prec, default_episodes_per_step(cname), 3, dev, timer, weights=w,
                                                                 kernel_events=not args.no_kernel_events)
            del w

    if rank == 0:
        episodes = world * args.steps * B
        eps_per_s = episodes / elapsed
        tflop_per_ep = GFLOP_PER_FRAME * frames_per_ep / 1e3            # the reference path's algorithmic work
        # executed work: the last ViT block is computed for the class-token rows only (engine.py: prune_last; few_shot.py:683 reads
        # nothing else of it; q, attention, out_proj and the MLP of the other N - 1 rows) -- (N - 1) (20 D^2 + 4 N D) FLOPs per frame fewer; every
        # end-to-end fraction below is priced on THIS figure
        pruned = bool(not dry and ARCH.startswith("ViT") and getattr(eng.vit, "prune_last", False))
        gflop_exec = executed_gflop_per_frame(ARCH, GFLOP_PER_FRAME, pruned)
        tflop_exec = gflop_exec * frames_per_ep / 1e3
        out = {
            "metric": "episodes/sec (5-way %d-shot, %d frames, %s)" % (SHOT, T, ARCH), "value": round(eps_per_s, 3),
            "unit": "episodes/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1e3, 4), "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": {"bf16": "bf16", "fp16": "f16", "fp16_strict": "f16", "fp32": "f32"}[args.precision], "data": "synthetic",
            "config": {"workload": cfgsel["name"] + ", random-init CLIP weights, synthetic structured frames",
                       "episodes_per_step_per_gpu": B, "frames_per_episode": frames_per_ep,
                       "tflop_per_episode": round(tflop_per_ep, 4), "tflop_per_episode_executed": round(tflop_exec, 4),
                       "last_block": ("class-token rows only behind the attention (the path reads x[:, 0] after the last block: "
                                      "few_shot.py:683); CFSAR_FULL_LAST_BLOCK=1 computes it whole") if pruned else "whole",
                       "precision": args.precision,
                       "numerics": ("%s MFMA operands, fp32 accumulation / LayerNorm + softmax statistics / final projection / "
                                    "temporal head" % args.precision + (", fp16 residual stream" if ARCH.startswith("ViT") else " (RN50: %s NHWC activations, BatchNorm folded)" % args.precision)
                                    if args.precision != "fp32" else "fp32 throughout"),
                       "parallelism": "episodes sharded over %d rank(s); one all-gather of accuracies" % world,
                       "launcher": "torch.distributed.run" if "TORCHELASTIC_RUN_ID" in os.environ else
                                   ("bench.py self-spawn" if world > 1 else "single process")},
            "episodes_per_step": B,
            "top1_acc_mean": round(float(gathered.mean().item()), 4),
            # per-rank rates of the timed region (value = all ranks' episodes / the slowest rank's time) and the collective's span
            "per_rank_episodes_per_s": {"min": round(args.steps * B / max(rank_elapsed), 3), "max": round(args.steps * B / min(rank_elapsed), 3),
                                        "ranks": len(rank_elapsed)},
            "collective": collective,
            "full": full,
        }
        if dry:
            out["dry_run"] = True
            out["value"] = 0.0
            out["config"]["workload"] = "DRY RUN (no-op step on CPU, gloo): launch / collective / timing protocol only"
            out["gathered_rank_ids"] = sorted({int(v) for v in gathered.tolist()})
        else:
            e2e_tflops = eps_per_s / world * tflop_exec                      # executed FLOPs, not the reference path's
            out["end_to_end_vit_tflops_per_gpu"] = round(e2e_tflops, 2)
            if full:
                if main_gemm is not None:
                    ms, flops, n = main_gemm
                    achieved = flops / (ms * 1e-3) / 1e12
                    traffic, traffic_src = measured_traffic(B) if (args.config == "cfg2" and args.precision == "bf16") else (None, None)
                    out["roofline"] = {"bound": "mfma", "achieved": round(achieved, 2), "peak": PEAK_BF16_TFLOPS,
                                       "unit": "TFLOP/s", "frac": round(achieved / PEAK_BF16_TFLOPS, 4),
                                       "frac_scope": "dominant kernel only: the bf16 MFMA GEMM launches of rank 0 (HIP events)",
                                       # episodes/s x TFLOP/episode / peak -- every kernel, launch gaps and the tail included
                                       "frac_end_to_end": round(e2e_tflops / PEAK_BF16_TFLOPS, 4),
                                       "traffic": traffic, "traffic_source": traffic_src,                 # the PMC passes were made on cfg2, bf16
                                       "kernel": GEMM_KERNEL_NOTE,
                                       "launches": n, "avg_launch_us": round(ms * 1e3 / n, 2),
                                       "algorithmic_gflop_per_launch": round(flops / n / 1e9, 3),
                                       "event_sampling": "every step" if event_every == 1 else "every %d-th timed step" % event_every, "gemm_share_of_step": round(ms / (elapsed * 1e3 * len(range(0, args.steps, event_every)) / max(args.steps, 1)), 4)}
                else:
                    out["roofline"] = None
                out["parity"] = (golden_parity(first_logits["v"][0], args.precision)
                                 if args.config == "cfg2" and "v" in first_logits else {"checked": False, "reason": "config has no in-bench golden"})
            if fp16_mode is not None:
                fp16_mode["relative_to_value"] = round(fp16_mode["value"] / eps_per_s, 4)
                out["fp16_mode"] = fp16_mode
            if strict_mode is not None:
                strict_mode["relative_to_value"] = round(strict_mode["value"] / eps_per_s, 4)
                out["strict_mode"] = strict_mode
            if config_legs is not None:
                out["configs"] = config_legs
            if host_inputs is not None:
                host_inputs["resident_episodes_per_s"] = round(eps_per_s / world, 3)
                out["inputs_host"] = host_inputs
            if full:
                out["cpu_baseline"] = None if (args.no_cpu_baseline or world > 1) else cpu_baseline()
    if use_dist:
        dist.destroy_process_group()
    if rank == 0:
        print(json.dumps(out), flush=True)          # the ONE JSON line, after every library's own teardown chatter


if __name__ == "__main__":
    main()
