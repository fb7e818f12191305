"""GPU: the stream pool (clip_fsar_amd.pool.StreamPool on libclipfsar_pool.so) -- the table-driven ring, gather and smoothing kernels
exactly against torch index arithmetic and against the lockstep library, a lockstep pool bit for bit against WindowStream, pool logits
against gallery.classify on every session's materialised windows over a schedule of sessions that open at different times, push unevenly,
skip pushes, close, reuse a slot and reset, in every mode; slot reuse against a fresh WindowStream; the tower-frame count; growing
galleries; top-k."""
import random

import pytest
import torch

from _cases import maxdiff
from test_gpu_stream import BOUND, CONTRACT, DEV, _filled, _frames, _gallery, _head, _materialised, _n_windows

import clip_fsar_amd.synth as synth

pytestmark = pytest.mark.gpu


def _uploader(max_streams):
    from clip_fsar_amd import pool_hip as ph
    return ph.TableUploader(DEV, max_streams)


# ------------------------------------------------------------------ 1: the kernels, exactly
@pytest.mark.parametrize("E", [64, 512, 768, 1024])
def test_ring_put_and_window_sequences_are_exact_copies(E):
    """uneven counts, sessions with 0 windows, wrapping rings, rates 1 and 3, window ranges that start and end inside sessions"""
    from clip_fsar_amd import pool_hip as ph
    from clip_fsar_amd.pool import plan_push
    g = torch.Generator().manual_seed(E)
    rng = random.Random(E)
    T, M = 5, 6
    for stride, rate, max_push in ((2, 1, 7), (1, 3, 6), (8, 1, 8)):
        cap = (T - 1) * rate + max_push
        up = _uploader(M)
        slots = {"a": 4, "b": 0, "c": 5, "d": 2}
        hist = {h: torch.empty(0, E, device=DEV) for h in slots}             # every frame a session ever pushed
        ring = torch.full((M, cap, E), -7.0, device=DEV)
        model = ring.clone()
        zero_window_rows = ranges_inside = 0
        for step in range(20):
            members = rng.sample(sorted(slots), rng.randint(1, 4))
            counts = [rng.randint(1, max_push) for _ in members]
            plan = plan_push([(slots[h], hist[h].shape[0]) for h in members], counts, T, stride, rate, max_push)
            assert len(plan.rounds) == 1 and plan.order is None
            rows = plan.rounds[0].rows
            feats = torch.randn(sum(counts), E, generator=g).to(DEV)
            table = up.upload(rows)
            ph.ring_put(feats, ring, table)
            f0 = 0
            for h, n in zip(members, counts):
                t = hist[h].shape[0]
                model[slots[h], (torch.arange(t, t + n, device=DEV) % cap)] = feats[f0:f0 + n]
                hist[h] = torch.cat([hist[h], feats[f0:f0 + n]])
                f0 += n
            assert torch.equal(ring, model), (stride, rate, step)            # the members' rows written, every other row untouched
            NW = sum(plan.n_windows)
            offsets = [sum(plan.n_windows[:i]) for i in range(len(members) + 1)]
            zero_window_rows += sum(1 for r in rows if r[ph.NW] == 0)
            if NW == 0:
                continue
            want = torch.cat([hist[h][torch.tensor([[k * stride + j * rate for j in range(T)] for k in range(first, first + nW)],
                                                   dtype=torch.long, device=DEV).reshape(nW, T)]
                              for h, first, nW in zip(members, plan.first_window, plan.n_windows)])
            X = torch.full((NW, T, E), -7.0, device=DEV)
            ph.window_sequences(ring, X, table, NW, 0, NW, T, stride, rate)
            assert torch.equal(X, want), (stride, rate, step)
            for w0, w1 in ((0, 1), (1, NW - 1), (NW // 2, NW)):
                if w0 < w1:
                    X1 = torch.full((w1 - w0 + 1, T, E), -7.0, device=DEV)  # a larger X: its first rows are written
                    ph.window_sequences(ring, X1, table, NW, w0, w1, T, stride, rate)
                    assert torch.equal(X1[:w1 - w0], want[w0:w1]) and bool((X1[w1 - w0:] == -7.0).all())
                    ranges_inside += w0 not in offsets and w1 not in offsets     # starts and ends inside sessions
        assert min(h.shape[0] for h in hist.values()) > cap                  # every session's ring wrapped
        assert zero_window_rows >= 2 and (ranges_inside >= 2 or stride == 8), (zero_window_rows, ranges_inside)


def test_copy_kernels_4_byte_path_and_large_counts():
    """E % 4 != 0 and a misaligned base take the 4-byte form; a gather of more rows than one grid has waves takes the grid-stride loop"""
    from clip_fsar_amd import pool_hip as ph
    g = torch.Generator().manual_seed(1)
    for E, off in ((66, 0), (64, 1)):
        M, cap, T = 3, 11, 4
        buf = torch.empty(M * cap * E + 4, device=DEV)
        ring = buf[off:off + M * cap * E].view(M, cap, E)
        feats = torch.randn(9 + 5, E, generator=g).to(DEV)
        # slot 2: frames 7 .. 15 in positions 7 .. 10, 0 .. 4, windows 4 .. 6 at stride 2; slot 0: frames 0 .. 4, window 0
        table = _uploader(M).upload([[2, 7, 9, 0, 8, 3, 0, 0], [0, 0, 5, 9, 0, 1, 3, 0]])
        ph.ring_put(feats, ring, table)
        live = torch.arange(7, 16, device=DEV)
        assert torch.equal(ring[2, live % cap], feats[:9]) and torch.equal(ring[0, :5], feats[9:])
        X = torch.empty(4, T, E, device=DEV)
        ph.window_sequences(ring, X, table, 4, 0, 4, T, 2, 1)
        idx = torch.tensor([[k * 2 + j for j in range(T)] for k in (4, 5, 6)], device=DEV) - 7
        assert torch.equal(X[:3], feats[:9][idx]) and torch.equal(X[3], feats[9:13])
    M, cap, T, E, nW = 3, 700, 32, 512, 600                                  # 3 * 600 * 32 rows > 4096 workgroups * 4 waves
    feats = torch.randn(M * cap, E, generator=g).to(DEV)
    ring = torch.empty(M, cap, E, device=DEV)
    rows = [[slot, 0, cap, i * cap, 0, nW, i * nW, 0] for i, slot in enumerate((1, 2, 0))]
    table = _uploader(M).upload(rows)
    ph.ring_put(feats, ring, table)
    assert torch.equal(ring[[1, 2, 0]].reshape(M * cap, E), feats)
    X = torch.empty(M * nW, T, E, device=DEV)
    ph.window_sequences(ring, X, table, M * nW, 0, M * nW, T, 1, 3)
    idx = torch.tensor([[k + 3 * j for j in range(T)] for k in range(nW)], device=DEV)
    assert torch.equal(X, feats.view(M, cap, E)[:, idx].reshape(M * nW, T, E))


@pytest.mark.parametrize("alpha", [0.5, 0.9])
def test_ragged_smoothing_has_the_bits_of_the_lockstep_library(alpha):
    """per session the recurrence of cfss_smooth_logits, bit for bit, with the windows split unevenly over several calls and some sessions
    absent from a call or present with 0 windows"""
    from clip_fsar_amd import pool_hip as ph
    from clip_fsar_amd import stream_hip as sh
    g = torch.Generator().manual_seed(int(alpha * 10))
    M, C = 5, 301
    slots = [3, 0, 4, 1]
    calls = [[2, 0, 5, 1], [0, 3, 1, None], [7, 1, 0, 4], [None, 2, 40, 1], [1, 1, 1, 1]]      # nW per session; None: not in the call
    total = [sum(c[i] or 0 for c in calls) for i in range(4)]
    x = [(torch.randn(n, C, generator=g) * 6.0 - 9.0).to(DEV) for n in total]
    state = torch.full((M, C), float("nan"), device=DEV)                      # never read before a session's first window
    up = _uploader(M)
    seen, got = [0] * 4, [[] for _ in range(4)]
    for call in calls:
        rows, off = [], 0
        for i, nW in enumerate(call):
            if nW is not None:
                rows.append([slots[i], 0, 0, 0, 0, nW, off, int(seen[i] > 0)])
                off += nW
        logits = torch.cat([x[i][seen[i]:seen[i] + nW] for i, nW in enumerate(call) if nW is not None])
        out = torch.empty_like(logits)
        ph.smooth_logits(logits, state, out, up.upload(rows), alpha)
        off = 0
        for i, nW in enumerate(call):
            if nW is not None:
                got[i].append(out[off:off + nW])
                off, seen[i] = off + nW, seen[i] + nW
    for i in range(4):
        want, st = torch.empty(1, total[i], C, device=DEV), torch.empty(1, C, device=DEV)
        sh.smooth_logits(x[i][None].contiguous(), st, want, alpha, 0)
        assert torch.equal(torch.cat(got[i]), want[0]), i
        assert torch.equal(state[slots[i]], st[0]), i
    assert bool(torch.isnan(state[2]).all())                                  # a slot outside every table


# ------------------------------------------------------------------ 2: a lockstep pool is WindowStream, bit for bit
@pytest.mark.parametrize("precision,kind", [("fp32", "support"), ("bf16", "combine")])
def test_lockstep_pool_equals_window_stream(precision, kind):
    """all sessions opened together and pushed equal counts, every push's windows within one classify_features chunk: the same rows go
    through the same launches as in WindowStream(n_streams=S), so the logits and the smoothed scores are equal bit for bit"""
    from clip_fsar_amd.pool import StreamPool
    from clip_fsar_amd.stream import WindowStream
    arch, T, S, stride, n = "ViT-test/16", 8, 3, 2, 27
    head = _head(arch, precision, T)
    with torch.no_grad():
        gal = _filled(head, arch, T, kind)
        frames = _frames(arch, S, n, seed=11)
        ws = WindowStream(gal, n_streams=S, stride=stride, max_push=6, smooth=0.5)
        pool = StreamPool(gal, max_streams=5, stride=stride, max_push=6, smooth=0.5)
        pool.close(pool.open())                                               # handles 1 .. 3 in slots 0 .. 2
        hs = [pool.open() for _ in range(S)]
        t = 0
        for m in (5, 1, 6, 4, 2, 6, 3):
            a = ws.push(frames[:, t:t + m])
            b = pool.push_packed(frames[:, t:t + m].reshape(S * m, *frames.shape[2:]), hs, [m] * S)
            nW = a.logits.shape[1]
            assert S * nW <= max(1, gal._fresh_engine().max_frames // T)      # one chunk on both sides
            assert b.first_window == [a.first_window] * S and b.offsets == [i * nW for i in range(S + 1)]
            assert torch.equal(b.logits.view(S, nW, len(gal)), a.logits), (t, m)
            assert torch.equal(b.smoothed.view(S, nW, len(gal)), a.smoothed), (t, m)
            t += m
        assert t == n and pool.stats(hs[0])["windows"] == ws.stats["windows"] and pool.stats(hs[0])["frames"] == n


# ------------------------------------------------------------------ 3: the contract
def _ticks(span, stride):
    """(operation, {session name: frames}) per tick.  a's first push and b's second exceed max_push = 6 (two or more rounds); b skips tick
    2, a skips tick 3; tick 3 lists c, whose window arrives in round 2, before b, whose windows arrive in round 1 (the result is re-ordered);
    b closes after tick 3 and d takes its slot; d's first push stops one frame short of its first window; a resets before tick 6."""
    return [(None, {"a": span + 2, "b": 3}),
            (None, {"a": 1, "b": span + 1}),
            ("open c", {"c": 1, "a": 4}),
            (None, {"c": max(span - 1, 7), "b": 5}),
            ("close b, open d", {"d": span - 1, "a": 2}),
            (None, {"d": 1 + stride, "c": 3}),
            ("reset a", {"a": span + stride, "d": 2}),
            (None, {"a": 2, "c": 1, "d": 5})]


def _run_schedule(pool, ticks, content, feats=None):
    """-> {(name, epoch): (frames pushed, [StreamOutput, ...])}; content: name -> [n, 3, H, W] frames (feats: name -> [n, E])"""
    h, used, epoch, outs = {}, {}, {}, {}
    for name in ("a", "b"):
        h[name], used[name], epoch[name] = pool.open(), 0, 0
    pushed = 0
    for op, tick in ticks:
        if op == "open c":
            h["c"], used["c"], epoch["c"] = pool.open(), 0, 0
        elif op == "close b, open d":
            slot = pool._session(h["b"]).slot
            pool.close(h.pop("b"))
            h["d"], used["d"], epoch["d"] = pool.open(), 0, 0
            assert pool._session(h["d"]).slot == slot                         # the freed slot, with the previous owner's frames in it
        elif op == "reset a":
            pool.reset(h["a"])
            epoch["a"] += 1
        src = feats if feats is not None else content
        arg = {h[name]: src[name][used[name]:used[name] + n] for name, n in tick.items()}
        got = (pool.push_features if feats is not None else pool.push)(arg)
        assert list(got) == [h[name] for name in tick]
        for name, n in tick.items():
            used[name] += n
            pushed += n
            outs.setdefault((name, epoch[name]), [0, []])
            outs[(name, epoch[name])][0] += n
            outs[(name, epoch[name])][1].append(got[h[name]])
    return outs, h, pushed


@pytest.mark.parametrize("arch,precision,kind,opts,stride,rate", CONTRACT)
def test_pool_equals_classify_on_materialised_windows(arch, precision, kind, opts, stride, rate):
    """Every session's logits against gallery.classify on its materialised windows, through push and through push_features; bound 2e-5,
    the project's figure for the same clip in a different batch.  Argmax equal on every row whose top-2 margin in the classify result
    exceeds twice the bound; at most 1 % of the rows may be exempt on that ground."""
    from clip_fsar_amd.pool import StreamPool
    T = 8
    big = arch != "ViT-test/16"
    span = (T - 1) * rate + 1
    head = _head(arch, precision, T)
    ticks = _ticks(span, stride)
    need = {}
    for _, tick in ticks:
        for name, n in tick.items():
            need[name] = need.get(name, 0) + n
    with torch.no_grad():
        gal = _filled(head, arch, T, kind, n_classes=5 if big else 6, shots=1 if big else 2, **opts)
        content = {name: _frames(arch, 1, n, seed=100 * stride + 10 * rate + i)[0] for i, (name, n) in enumerate(sorted(need.items()))}
        eng = gal._fresh_engine()
        feats = {}
        for name, fr in content.items():
            feats[name] = torch.empty(fr.shape[0], gal.E, device=DEV)
            for f0 in range(0, fr.shape[0], eng.max_frames):
                eng.vit.forward(fr[f0:f0 + eng.max_frames].contiguous(), feats[name][f0:f0 + eng.max_frames])
        worst, undecided, rows, windows = 0.0, 0, 0, 0
        for through_features in (False, True):
            pool = StreamPool(gal, max_streams=3, stride=stride, rate=rate, max_push=6)
            outs, h, pushed = _run_schedule(pool, ticks, content, feats if through_features else None)
            start = {}
            for (name, ep), (n, pieces) in sorted(outs.items()):
                k = 0
                for o in pieces:                                              # every window once, in order
                    assert o.first_window == k and o.smoothed is None
                    k += o.logits.shape[0]
                nW = _n_windows(n, T, stride, rate)
                assert k == nW, (name, ep, n, k, nW)
                f0 = start.get(name, 0)                                       # a reset starts a new epoch at the session's next frame
                start[name] = f0 + n
                if nW == 0:
                    continue
                got = torch.cat([o.logits for o in pieces])
                ref = gal.classify(_materialised(content[name][None, f0:f0 + n], T, stride, rate, nW))
                worst = max(worst, maxdiff(got.cpu(), ref.cpu()))
                top2 = ref.topk(2, dim=-1).values
                decided = (top2[:, 0] - top2[:, 1]) > 2 * BOUND
                assert torch.equal(got.argmax(-1)[decided], ref.argmax(-1)[decided]), (name, ep)
                undecided += int((~decided).sum())
                rows += nW
            windows = rows
            # d pushed span - 1 frames first: no window before its own (T-1) * rate + 1 frames
            assert outs[("d", 0)][1][0].logits.shape[0] == 0 and outs[("d", 0)][1][1].logits.shape[0] >= 1
            # the tower-frame count is exact, per session (since its reset) and pool-wide
            for name, hh in h.items():
                last_epoch = max(ep for (nm, ep) in outs if nm == name)
                n = outs[(name, last_epoch)][0]
                assert pool.stats(hh) == {"frames": n, "tower_frames": 0 if through_features else n,
                                          "windows": _n_windows(n, T, stride, rate)}
            assert pool.stats() == {"frames": pushed, "tower_frames": 0 if through_features else pushed,
                                    "windows": sum(sum(o.logits.shape[0] for o in p) for _, p in outs.values()), "open": 3}
    torch.cuda.synchronize()
    print("%s %s %s %s stride %d rate %d: |pool - classify| = %.2e over %d windows (push and push_features), %d rows without a decided "
          "argmax" % (arch, precision, kind, opts, stride, rate, worst, windows, undecided))
    assert worst <= BOUND, worst
    assert undecided <= 0.01 * windows, (undecided, windows)


# ------------------------------------------------------------------ 4: a reused slot is a fresh session
def test_reused_slot_behaves_as_a_fresh_session():
    from clip_fsar_amd.pool import StreamPool
    from clip_fsar_amd.stream import WindowStream
    arch, T, stride, rate = "ViT-test/16", 8, 2, 2
    span = (T - 1) * rate + 1
    head = _head(arch, "fp32", T)
    with torch.no_grad():
        gal = _filled(head, arch, T)
        old, new = _frames(arch, 1, 40, seed=31)[0], _frames(arch, 1, span + 9, seed=32)[0]
        pool = StreamPool(gal, max_streams=2, stride=stride, rate=rate, max_push=8, smooth=0.75)
        a, other = pool.open(), pool.open()
        first = pool.push({a: old, other: old[:5]})                           # fills a's ring and its smoothing state
        assert first[a].logits.shape[0] == _n_windows(40, T, stride, rate) and first[other].logits.shape[0] == 0
        slot = pool._session(a).slot
        pool.close(a)
        b = pool.open()
        assert b not in (a, other) and pool._session(b).slot == slot
        pieces = [pool.push({b: new[:span - 1]}), pool.push({b: new[span - 1:span], other: old[5:7]}), pool.push({b: new[span:]})]
        assert pieces[0][b].logits.shape[0] == 0 and pieces[0][b].first_window == 0          # span - 1 frames: no window yet
        assert pieces[1][b].logits.shape[0] == 1 and pieces[1][b].first_window == 0          # its own frame span completes window 0
        got = torch.cat([p[b].logits for p in pieces])
        got_s = torch.cat([p[b].smoothed for p in pieces])
        ws = WindowStream(gal, n_streams=1, stride=stride, rate=rate, max_push=8, smooth=0.75)
        ref = ws.push(new[None])
    torch.cuda.synchronize()
    d, ds = maxdiff(got.cpu(), ref.logits[0].cpu()), maxdiff(got_s.cpu(), ref.smoothed[0].cpu())
    print("reused slot vs a fresh WindowStream: logits %.2e, smoothed %.2e over %d windows" % (d, ds, got.shape[0]))
    assert got.shape == ref.logits[0].shape and got.shape[0] == _n_windows(span + 9, T, stride, rate)
    assert d <= BOUND and ds <= BOUND, (d, ds)
    assert torch.equal(got_s[0], got[0])                                      # y_0 = x_0: nothing of the previous owner's state


# ------------------------------------------------------------------ 5: the tower runs once per pushed frame, in one call sequence
def test_tower_frame_count_is_exact(monkeypatch):
    from clip_fsar_amd.pool import StreamPool
    arch, T = "ViT-test/16", 8
    head = _head(arch, "fp32", T)
    with torch.no_grad():
        gal = _filled(head, arch, T)
        eng = gal._fresh_engine()
        seen = []
        real = eng.vit.forward
        monkeypatch.setattr(eng.vit, "forward", lambda x, out, *a, **k: (seen.append(x.shape[0]), real(x, out, *a, **k))[1])
        monkeypatch.setattr(eng, "max_frames", 16)
        frames = _frames(arch, 3, 30, seed=4)
        pool = StreamPool(gal, max_streams=4, stride=1, max_push=8)
        a, b, c = pool.open(), pool.open(), pool.open()
        pool.push({a: frames[0, :21], b: frames[1, :2], c: frames[2, :14]})   # 37 frames: tower calls of 16, 16, 5
        assert seen == [16, 16, 5]
        pool.push({c: frames[2, 14:15]})
        pool.push({b: frames[1, 2:30], a: frames[0, 21:23]})
        assert seen == [16, 16, 5, 1, 16, 14]
    assert pool.stats(a) == {"frames": 23, "tower_frames": 23, "windows": 16}
    assert pool.stats(b) == {"frames": 30, "tower_frames": 30, "windows": 23}
    assert pool.stats(c) == {"frames": 15, "tower_frames": 15, "windows": 8}
    assert sum(seen) == 68 and pool.stats() == {"frames": 68, "tower_frames": 68, "windows": 47, "open": 3}


# ------------------------------------------------------------------ 6: growing galleries, smoothing state, top-k, packed order, errors on the device
def test_growth_smoothing_topk_and_errors():
    from clip_fsar_amd import stream_hip as sh
    from clip_fsar_amd.pool import StreamPool
    arch, T, n = "ViT-test/16", 8, 20
    head = _head(arch, "fp32", T, seed=23)
    res = synth.ARCHS[arch]["res"]
    with torch.no_grad():
        gal = _filled(head, arch, T, n_classes=7)
        frames = _frames(arch, 3, n, seed=6)
        plain = StreamPool(gal, max_streams=4, stride=3, max_push=32)
        smooth = StreamPool(gal, max_streams=4, stride=3, max_push=32, smooth=0.75)
        a, b = plain.open(), plain.open()
        sa, sb, sc = smooth.open(), smooth.open(), smooth.open()
        before = plain.push({a: frames[0, :11], b: frames[1, :4]})
        sbefore = smooth.push({sa: frames[0, :11], sb: frames[1, :4]})        # sa carries state now, sb and sc do not
        assert before[a].logits.shape == (2, 7) and before[b].logits.shape == (0, 7) and before[a].smoothed is None
        assert torch.equal(sbefore[sa].logits, before[a].logits)
        g = torch.Generator().manual_seed(77)
        gal.add_classes((torch.randn(2, T, 3, res, res, generator=g) * 0.5).to(DEV), [20, 21])
        # classes added between pushes appear as new columns
        after = plain.push({b: frames[1, 4:], a: frames[0, 11:]})
        nW = _n_windows(n, T, 3, 1)
        assert list(after) == [b, a] and after[a].logits.shape == (nW - 2, 9) and after[a].first_window == 2
        assert after[b].logits.shape == (nW, 9) and after[b].first_window == 0
        ref = gal.classify(_materialised(frames[:2], T, 3, 1, nW)).view(2, nW, 9)
        assert maxdiff(after[a].logits.cpu(), ref[0, 2:].cpu()) <= BOUND and maxdiff(after[b].logits.cpu(), ref[1].cpu()) <= BOUND
        assert maxdiff(before[a].logits.cpu(), ref[0, :2, :7].cpu()) <= BOUND
        # with smoothing on, a session that carries state raises until reset; the others, and sessions opened afterwards, are fine
        with pytest.raises(RuntimeError, match="reset"):
            smooth.push({sa: frames[0, 11:]})
        with pytest.raises(RuntimeError, match="reset"):
            smooth.push({sb: frames[1, 4:], sa: frames[0, 11:]})
        assert smooth.stats(sb)["frames"] == 4                                # the refused push advanced nothing
        ok = smooth.push({sb: frames[1, 4:], sc: frames[2]})
        assert ok[sb].smoothed.shape == (nW, 9) and ok[sc].smoothed.shape == (nW, 9)
        with pytest.raises(RuntimeError, match="reset"):
            smooth.push({sa: frames[0, 11:]})                                 # still: its state is of the old width
        smooth.reset(sa)
        again = smooth.push({sa: frames[0]})
        assert again[sa].first_window == 0 and again[sa].smoothed.shape == (nW, 9)
        want = torch.empty(1, nW, 9, device=DEV)
        sh.smooth_logits(again[sa].logits[None].contiguous(), torch.empty(1, 9, device=DEV), want, 0.75, 0)
        assert torch.equal(again[sa].smoothed, want[0])
        late = smooth.open()
        assert smooth.push({late: frames[2]})[late].smoothed.shape == (nW, 9)
        # packed form: session-major in the order given; top-k per window against a stable sort
        po = smooth.push_packed(torch.cat([frames[1, :9], frames[0, :12]]), [late, sa], [9, 12])
        assert po.sessions == [late, sa] and po.first_window == [nW, nW] and po.offsets == [0, 3, 7]
        for smoothed, src in ((False, po.logits), (True, po.smoothed)):
            vals, idx = smooth.topk(po, k=3, smoothed=smoothed)
            sv, si = torch.sort(src, dim=-1, descending=True, stable=True)
            assert vals.shape == (7, 3) and torch.equal(vals, sv[:, :3]) and torch.equal(idx.long(), si[:, :3])
        assert plain.topk(before[b], k=2)[0].shape == (0, 2)
        with pytest.raises(ValueError, match="no smoothed"):
            plain.topk(after[a], smoothed=True)
        with pytest.raises(ValueError, match="k must be"):
            smooth.topk(po, k=10)
        # wrong shapes, counts, CPU tensors, stale engines
        with pytest.raises(ValueError, match="frames must be"):
            plain.push({a: frames[0, :, :2]})
        with pytest.raises(ValueError, match="feats must be"):
            plain.push_features({a: torch.zeros(2, gal.E + 1, device=DEV)})
        with pytest.raises(ValueError, match="counts sum to 5"):
            plain.push_packed(frames[0, :4], [a, b], [2, 3])
        with pytest.raises(RuntimeError, match="HIP device tensor"):
            plain.push({a: frames[0, :2].cpu()})
        with pytest.raises(RuntimeError, match="no classes registered"):
            StreamPool(_gallery(head), max_streams=2).push({0: frames[0]})
        head.load_state_dict(head.state_dict())
        with pytest.raises(RuntimeError, match="changed"):
            plain.push({a: frames[0, :2]})
