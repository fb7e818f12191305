"""GPU: frame ingest (clip_fsar_amd.ingest.FrameIngest on libclipfsar_ingest.so) -- the mixed-geometry kernel bit for bit against
preprocess_video run clip by clip and against the reference golden, beyond the launch cap and on the 4-byte store path; the same result
from device, pinned and pageable clips; staging buffers reused and grown under copies and kernels in flight; StreamPool.push_u8 /
push_u8_packed and WindowStream.push_u8 bit for bit against push fed preprocess_video of the same clips over the pool's contract schedule."""
import collections

import pytest
import torch

import clip_fsar_amd.synth as synth
from test_gpu_pool import _ticks
from test_gpu_stream import DEV, _filled, _head
from test_preprocess_n2 import _cases

pytestmark = pytest.mark.gpu

MEAN, STD = synth.CLIP_MEAN, synth.CLIP_STD
GOLD_BOUND = 2e-5         # tests/test_preprocess_n2.py::test_hip_preprocess_matches_reference


def _clip(n, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (n, H, W, 3), dtype=torch.uint8, generator=g)


def _reference(clips, test_scale, crop, nsc=1, idx=1):
    """preprocess_video clip by clip: one upload and one launch per clip"""
    from clip_fsar_amd.preprocess import preprocess_video
    idxs = idx if isinstance(idx, list) else [idx] * len(clips)
    return torch.cat([preprocess_video(c.to(DEV), test_scale, crop, MEAN, STD, nsc, ix) for c, ix in zip(clips, idxs)])


def _ingest(test_scale, crop, **kw):
    from clip_fsar_amd.ingest import FrameIngest
    return FrameIngest(DEV, test_scale, crop, MEAN, STD, **kw)


# ------------------------------------------------------------------ 1: the kernel
@pytest.mark.parametrize("test_scale,crop", [(256, 224), ([72, 96], 64)])
def test_one_launch_equals_preprocess_video_clip_by_clip(test_scale, crop):
    """seven groups in one call: the listed geometries, an odd one, an upscaled one, one whose source equals the scale; n from 1 to 17"""
    sh, sw = (test_scale, test_scale) if isinstance(test_scale, int) else test_scale
    shapes = [(1, 240, 320), (17, 256, 340), (3, 360, 640), (5, 97, 131), (2, sh, sw), (9, 48, 40), (4, 2, 2)]
    clips = [_clip(n, H, W, seed=10 * crop + i) for i, (n, H, W) in enumerate(shapes)]
    fi = _ingest(test_scale, crop)
    got = fi.transform([c.to(DEV) for c in clips])
    want = _reference(clips, test_scale, crop)
    assert got.shape == (41, 3, crop, crop) and got.dtype == torch.float32
    assert torch.equal(got, want)
    one = fi.transform([clips[3].to(DEV)])                                    # a single device clip: read where it lies
    assert torch.equal(one, want[21:26]) and all(s.done is None for s in fi._slots[1:])


def test_against_the_reference_golden():
    groups = collections.defaultdict(list)
    for name, c, vid, scale, ref in _cases():
        groups[(c["crop"], tuple(scale), c["nsc"])].append((name, c, vid, ref))
    for (crop, scale, nsc), cases in groups.items():
        fi = _ingest(list(scale), crop, num_spatial_crops=nsc, idx=[c["idx"] for _, c, _, _ in cases])
        got = fi.transform([vid for _, _, vid, _ in cases]).cpu()
        want = torch.cat([ref for _, _, _, ref in cases])
        err = float((got - want).abs().max())
        print("ingest of %s vs the reference golden: %.2e" % ([n for n, _, _, _ in cases], err))
        assert got.shape == want.shape and err < GOLD_BOUND, err


def test_beyond_the_launch_cap():
    """604 frames at crop 224 are 4 228 workgroup units, more than the 4 096 workgroups of one grid: the grid-stride loop"""
    shapes = [(150, 32, 48), (151, 40, 30), (152, 24, 56), (151, 36, 36)]
    clips = [_clip(n, H, W, seed=70 + i).to(DEV) for i, (n, H, W) in enumerate(shapes)]
    got = _ingest(256, 224).transform(clips)
    assert got.shape[0] == 604 and torch.equal(got, _reference(clips, 256, 224))


@pytest.mark.parametrize("test_scale,crop", [([33, 45], 30), (23, 21), (9, 1)])
def test_crops_that_are_no_multiple_of_4(test_scale, crop):
    shapes = [(3, 50, 70), (1, 17, 19), (6, 33, 45), (2, 5, 4)]
    clips = [_clip(n, H, W, seed=crop + i) for i, (n, H, W) in enumerate(shapes)]
    got = _ingest(test_scale, crop).transform(clips)
    assert torch.equal(got, _reference(clips, test_scale, crop))


def test_an_out_that_is_not_16_byte_aligned_takes_the_4_byte_stores():
    """the binding on an `out` four bytes off a 16-byte boundary at crop 224 (FrameIngest's own torch.empty is always aligned): the
    single-pixel kernel, the same frames, nothing written in front of them"""
    from clip_fsar_amd import ingest_hip as ihp
    from clip_fsar_amd.ingest import plan_ingest
    shapes = [(2, 97, 131), (3, 120, 160), (1, 256, 256)]
    clips = [_clip(n, H, W, seed=50 + i).to(DEV) for i, (n, H, W) in enumerate(shapes)]
    plan = plan_ingest(shapes, 256, 224)
    staged = torch.zeros(plan.total_bytes, dtype=torch.uint8, device=DEV)
    for off, c in zip(plan.offsets, clips):
        staged[off:off + c.numel()].copy_(c.reshape(-1))
    table = ihp.table_uploader(DEV, 8).upload(plan.rows)
    flat = torch.full((1 + 6 * 3 * 224 * 224,), 7.0, device=DEV)
    out = flat[1:].view(6, 3, 224, 224)
    assert out.data_ptr() % 16 == 4 and out.is_contiguous()
    ihp.transform_frames(staged, out, table, 224, MEAN, STD)
    assert torch.equal(out, _reference(clips, 256, 224)) and float(flat[0]) == 7.0


def test_preprocess_frames_writes_the_bits_it_wrote_before_the_shared_header():
    """tests/golden/preprocess_bits.npz (tools/preprocess_bits.py): what cfsar_preprocess_frames wrote on an MI355X BEFORE its per-pixel
    arithmetic moved into csrc/frame_transform.h.  The golden bound of 2e-5 lets a differently contracted fma through (one unit in the
    last place, 4.8e-7); this does not: preprocess_kernel and, through one call, the ingest kernel must reproduce those bits."""
    import json
    import os

    import numpy as np
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "preprocess_bits.npz"))
    meta = json.loads(str(z["meta"]))
    from clip_fsar_amd.preprocess import preprocess_video
    assert len(meta["cases"]) >= 8
    for name, c in meta["cases"].items():
        v = synth.pseudo_normal(c["T"] * c["H"] * c["W"] * 3, "u8video/" + name, meta["seed"])
        vid = torch.from_numpy(np.clip(v * 60.0 + 128.0, 0, 255).astype(np.uint8).reshape(c["T"], c["H"], c["W"], 3))
        want = torch.from_numpy(z[name])
        got = preprocess_video(vid.to(DEV), c["scale"], c["crop"], meta["mean"], meta["std"], c["nsc"], c["idx"]).cpu()
        assert got.shape == want.shape and torch.equal(got, want), (name, float((got - want).abs().max()))
        fi = FrameIngest_for(c, meta)
        assert torch.equal(fi.transform([vid]).cpu(), want), name


def FrameIngest_for(c, meta):
    from clip_fsar_amd.ingest import FrameIngest
    return FrameIngest(DEV, c["scale"], c["crop"], meta["mean"], meta["std"], num_spatial_crops=c["nsc"], idx=c["idx"])


# ------------------------------------------------------------------ 2: residency
def test_device_pinned_pageable_and_mixed_clips_give_the_same_frames():
    shapes = [(4, 240, 320), (1, 97, 131), (7, 120, 160), (2, 256, 256), (3, 64, 48)]
    clips = [_clip(n, H, W, seed=30 + i) for i, (n, H, W) in enumerate(shapes)]
    assert not any(c.is_pinned() for c in clips)
    forms = {"device": [c.to(DEV) for c in clips], "pinned": [c.pin_memory() for c in clips], "pageable": clips,
             "mixed": [clips[0].to(DEV), clips[1].pin_memory(), clips[2], clips[3], clips[4].to(DEV)]}
    fi = _ingest(256, 224)
    got = {k: fi.transform(v) for k, v in forms.items()}                      # one object, four calls, no synchronisation between them
    assert fi.uploaded is not None and fi._copy_stream is not None
    want = _reference(clips, 256, 224)
    for k, v in got.items():
        assert torch.equal(v, want), k
    non_contiguous = [c.pin_memory().flip(0) for c in clips]                  # host copies are made; the result is the flipped clips'
    assert torch.equal(fi.transform(non_contiguous), _reference([c.flip(0) for c in clips], 256, 224))


# ------------------------------------------------------------------ 3: staging reuse
def test_staging_buffers_are_reused_and_grown_under_work_in_flight():
    """depth 2, six calls back to back with different contents and sizes, no host synchronisation; the fourth call outgrows its buffer.
    Between the calls the compute stream is kept busy, so uploads run ahead of the kernels that read the buffer before them: a buffer
    rewritten under a copy or a kernel in flight would show as wrong pixels."""
    sizes = [[(3, 120, 160), (2, 97, 131)], [(5, 100, 100), (1, 240, 320)], [(2, 90, 150), (4, 64, 64), (1, 50, 60)],
             [(9, 240, 320), (6, 256, 340), (2, 97, 131)], [(1, 31, 17), (3, 120, 160)], [(8, 240, 320), (5, 200, 300)]]
    calls = [[_clip(n, H, W, seed=100 * k + i) for i, (n, H, W) in enumerate(call)] for k, call in enumerate(sizes)]
    calls = [[c.pin_memory() if (k + i) % 2 else c for i, c in enumerate(call)] for k, call in enumerate(calls)]      # pinned and pageable
    fi = _ingest(256, 224, depth=2)
    busy = torch.randn(4096, 4096, device=DEV)
    outs, consumed, capacity = [], [], []
    torch.cuda.synchronize()
    for call in calls:
        out = fi.transform(call)
        consumed.append(out.double().sum(dim=(1, 2, 3)))                       # a later kernel on the compute stream reads the result
        for _ in range(6):
            busy = torch.tanh(busy @ busy * 1e-2)                              # ... and keeps the stream busy under the next upload
        outs.append(out)
        capacity.append([None if s.dev is None else s.dev.numel() for s in fi._slots])
    torch.cuda.synchronize()
    assert capacity[2] == capacity[1] and capacity[3][1] > capacity[2][1] and capacity[5] == capacity[3], capacity     # grown once
    assert len(fi._retired) <= 1                                                # the outgrown buffer, unless its last reader was seen finished
    fi.transform(calls[0])
    assert fi._retired == []                                                   # every call drops what nothing reads any more
    for k, (call, out, s) in enumerate(zip(calls, outs, consumed)):
        want = _reference(call, 256, 224)
        assert torch.equal(out, want), k
        assert torch.equal(s, want.double().sum(dim=(1, 2, 3))), k


# ------------------------------------------------------------------ 4: the contract
SIZES = {"a": (80, 112), "b": (64, 64), "c": (97, 131), "d": (72, 96)}       # every session its own source resolution; d's is the scale
SCALE, CROP = [72, 96], 64                                                    # ViT-test/16 takes 64 x 64 frames


def _schedule(pool, ticks, clips, call):
    """test_gpu_pool._run_schedule with the push left to `call(pool, {handle: uint8 clip})` -> ([(handles, result)], handles)"""
    h, used, results = {"a": pool.open(), "b": pool.open()}, collections.defaultdict(int), []
    for op, tick in ticks:
        if op == "open c":
            h["c"] = pool.open()
        elif op == "close b, open d":
            slot = pool._session(h["b"]).slot
            pool.close(h.pop("b"))
            h["d"] = pool.open()
            assert pool._session(h["d"]).slot == slot
        elif op == "reset a":
            pool.reset(h["a"])
        arg = {h[name]: clips[name][used[name]:used[name] + n] for name, n in tick.items()}
        for name, n in tick.items():
            used[name] += n
        results.append(call(pool, arg))
    return results, h


def _same_packed(a, b):
    assert a.sessions == b.sessions and a.first_window == b.first_window and a.offsets == b.offsets
    assert torch.equal(a.logits, b.logits) and torch.equal(a.smoothed, b.smoothed)


@pytest.mark.parametrize("precision,kind", [("fp32", "support"), ("bf16", "support"), ("fp32", "combine")])
def test_push_u8_equals_push_of_preprocess_video(precision, kind):
    """the four-session schedule of tests/test_gpu_pool.py's contract test (joins, a close with slot reuse, a reset, skipped ticks, pushes
    of 1 to 17 frames at max_push = 6), host clips: both sides hand the same fp32 frames to the same launches, so everything is equal"""
    from clip_fsar_amd.pool import StreamPool
    from clip_fsar_amd.preprocess import preprocess_video
    arch, T, stride, rate = "ViT-test/16", 8, 2, 2
    span = (T - 1) * rate + 1
    ticks = _ticks(span, stride)
    assert max(n for _, t in ticks for n in t.values()) == 17 and min(n for _, t in ticks for n in t.values()) == 1
    need = collections.defaultdict(int)
    for _, tick in ticks:
        for name, n in tick.items():
            need[name] += n
    clips = {name: _clip(n, *SIZES[name], seed=ord(name)) for name, n in need.items()}
    clips["a"], clips["c"] = clips["a"].pin_memory(), clips["c"].pin_memory()             # b and d stay pageable
    head = _head(arch, precision, T)
    data = head.args.DATA
    data.TEST_SCALE, data.TEST_CROP_SIZE, data.MEAN, data.STD = SCALE, CROP, list(MEAN), list(STD)

    def fp32(arg):
        return {hh: preprocess_video(c.to(DEV), SCALE, CROP, MEAN, STD) for hh, c in arg.items()}

    def ref_packed(pool, arg):
        f = fp32(arg)
        return pool.push_packed(torch.cat(list(f.values())), list(f), [v.shape[0] for v in f.values()])

    legs = {"push": lambda pool, arg: pool.push(fp32(arg)), "push_u8": lambda pool, arg: pool.push_u8(arg), "push_packed": ref_packed,
            "push_u8_packed": lambda pool, arg: pool.push_u8_packed(list(arg.values()), list(arg))}
    with torch.no_grad():
        gal = _filled(head, arch, T, kind)
        got, stats = {}, {}
        for leg, call in legs.items():
            explicit = _ingest(SCALE, CROP) if leg == "push_u8_packed" else None          # push_u8 builds its own from the head's config
            pool = StreamPool(gal, max_streams=3, stride=stride, rate=rate, max_push=6, smooth=0.5, ingest=explicit)
            got[leg], h = _schedule(pool, ticks, clips, call)
            stats[leg] = [pool.stats(hh) for hh in sorted(h.values())] + [pool.stats()]
            if leg == "push_u8":
                assert pool._ingest is not None and pool._ingest.scale_hw == (72, 96) and pool._ingest.crop == 64
    torch.cuda.synchronize()
    windows = 0
    for a, b in zip(got["push"], got["push_u8"]):
        assert list(a) == list(b)
        for hh in a:
            assert a[hh].first_window == b[hh].first_window
            assert torch.equal(a[hh].logits, b[hh].logits) and torch.equal(a[hh].smoothed, b[hh].smoothed)
            windows += a[hh].logits.shape[0]
    for a, b in zip(got["push_packed"], got["push_u8_packed"]):
        _same_packed(a, b)
    assert windows > 20 and stats["push"] == stats["push_u8"] == stats["push_packed"] == stats["push_u8_packed"]
    assert stats["push"][-1]["frames"] == stats["push"][-1]["tower_frames"] == sum(need.values())


def test_window_stream_push_u8_equals_push():
    from clip_fsar_amd.preprocess import preprocess_video
    from clip_fsar_amd.stream import WindowStream
    arch, T, B = "ViT-test/16", 8, 2
    head = _head(arch, "fp32", T)
    frames = _clip(B * 17, 80, 112, seed=5).view(B, 17, 80, 112, 3).pin_memory()
    with torch.no_grad():
        gal = _filled(head, arch, T)
        a = WindowStream(gal, n_streams=B, stride=2, max_push=6, smooth=0.5)
        b = WindowStream(gal, n_streams=B, stride=2, max_push=6, smooth=0.5, ingest=_ingest(SCALE, CROP))
        t = 0
        for n in (5, 9, 3):
            piece = frames[:, t:t + n]
            x = preprocess_video(piece.reshape(B * n, 80, 112, 3).to(DEV), SCALE, CROP, MEAN, STD).view(B, n, 3, CROP, CROP)
            ra, rb = a.push(x), b.push_u8(piece if n != 9 else piece.to(DEV))
            assert ra.first_window == rb.first_window
            assert torch.equal(ra.logits, rb.logits) and torch.equal(ra.smoothed, rb.smoothed)
            t += n
    assert a.stats == b.stats == {"frames": 17, "tower_frames": B * 17, "windows": 5}


# ------------------------------------------------------------------ 5: errors
def test_errors_are_raised_before_any_launch_and_leave_the_counters():
    from clip_fsar_amd.pool import StreamPool
    arch, T = "ViT-test/16", 8
    head = _head(arch, "fp32", T)
    with torch.no_grad():
        gal = _filled(head, arch, T)
        fi = _ingest(SCALE, CROP)
        pool = StreamPool(gal, max_streams=3, stride=2, max_push=6, ingest=fi)
        a, b, c = pool.open(), pool.open(), pool.open()
        u8 = _clip(9, 80, 112, seed=1)
        ok = pool.push_u8({a: u8, c: u8[:3].to(DEV)})
        assert ok[a].logits.shape[0] == 1 and ok[c].logits.shape[0] == 0
        pool.close(b)
        before = [pool.stats(a), pool.stats(c), pool.stats()]
        launched = (fi._next, [s.done for s in fi._slots])
        for exc, match, call in ((ValueError, "not open", lambda: pool.push_u8({a: u8, b: u8})),
                                 (ValueError, "appears twice", lambda: pool.push_u8_packed([u8, u8], [a, a])),
                                 (TypeError, "uint8", lambda: pool.push_u8({a: u8, c: u8.to(torch.int32)})),
                                 (TypeError, "uint8", lambda: pool.push_u8({a: u8.float()})),
                                 (TypeError, "uint8", lambda: pool.push_u8({a: u8.to(DEV).float()})),
                                 (ValueError, r"\[n, H, W, 3\]", lambda: pool.push_u8({a: u8.to(DEV)[0]})),
                                 (ValueError, "2 clips for 1 sessions", lambda: pool.push_u8_packed([u8, u8], [a]))):
            with pytest.raises(exc, match=match):
                call()
        assert [pool.stats(a), pool.stats(c), pool.stats()] == before
        assert (fi._next, [s.done for s in fi._slots]) == launched              # no staging slot was taken, no kernel recorded
        again = pool.push_u8({a: u8[:2]})
        assert again[a].first_window == 1 and pool.stats(a)["frames"] == 11
