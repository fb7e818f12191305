"""GPU: tempo windows (libclipfsar_tempo.so, clip_fsar_amd.tempo_hip, StreamPool(rates=...)) -- the gather and the reduction exactly
against torch index arithmetic and reference_reduce; a pool with one rate bit for bit against the pool with that `rate`; a pool with
three rates against three pools of one rate each, fed the same streams with their first frames dropped; a slowed action found at its own
tempo where a rate = 1 pool scores it lower; enrolment and explain at a tempo on a wrapped ring."""
import random

import pytest
import torch

from _cases import maxdiff
from test_gpu_enroll import _assert_same_classes
from test_gpu_live import ARCH, T, _pair, _videos
from test_gpu_pool import _run_schedule, _ticks, _uploader
from test_gpu_stream import BOUND, DEV, _filled, _frames, _head, _n_windows

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.contiguous().view(torch.int32)        # NaN-proof equality


def _same(u, v):
    return (u is None and v is None) or (u.dtype == v.dtype and u.shape == v.shape and torch.equal(_bits(u), _bits(v)))


def _tempo_rows(first, nW, stride, Tk, rates):
    """frame numbers [nW, R, Tk] of every tempo of the session's windows first .. first + nW - 1: e - (Tk - 1 - j) * rate, e the window's
    last frame in its rmax form"""
    rmax = rates[-1]
    return torch.tensor([[[k * stride + (Tk - 1) * rmax - (Tk - 1 - j) * r for j in range(Tk)] for r in rates]
                         for k in range(first, first + nW)], dtype=torch.long, device=DEV).reshape(nW, len(rates), Tk)


# ------------------------------------------------------------------ 1: the gather, exactly
@pytest.mark.parametrize("E,off", [(64, 0), (66, 0), (512, 0), (64, 1)])
def test_tempo_gather_is_an_exact_copy(E, off):
    """uneven counts, sessions with 0 windows, wrapped rings, window ranges that start and end inside sessions, sentinel rows behind the
    rows written, the ring untouched; E = 66 and a ring whose base is one float off 16 bytes take the 4-byte pieces"""
    from clip_fsar_amd import pool_hip as ph
    from clip_fsar_amd import tempo_hip as th
    from clip_fsar_amd.pool import plan_push
    g = torch.Generator().manual_seed(E + off)
    rng = random.Random(E + off)
    Tk, M = 5, 6
    for stride, rates, max_push in ((2, (1,), 7), (1, (1, 3), 6), (2, (1, 2, 4), 9)):
        R, rmax = len(rates), rates[-1]
        cap = (Tk - 1) * rmax + max_push
        up = _uploader(M)
        slots = {"a": 4, "b": 0, "c": 5, "d": 2}
        hist = {h: torch.empty(0, E, device=DEV) for h in slots}             # every frame a session ever pushed
        buf = torch.full((M * cap * E + 4,), -7.0, device=DEV)
        ring = buf[off:off + M * cap * E].view(M, cap, E)
        zero_window_rows = ranges_inside = 0
        for step in range(20):
            members = rng.sample(sorted(slots), rng.randint(1, 4))
            counts = [rng.randint(1, max_push) for _ in members]
            plan = plan_push([(slots[h], hist[h].shape[0]) for h in members], counts, Tk, stride, rmax, max_push)
            assert len(plan.rounds) == 1 and plan.order is None
            rows = plan.rounds[0].rows
            feats = torch.randn(sum(counts), E, generator=g).to(DEV)
            table = up.upload(rows)
            ph.ring_put(feats, ring, table)
            f0 = 0
            for h, n in zip(members, counts):
                hist[h] = torch.cat([hist[h], feats[f0:f0 + n]])
                f0 += n
            NW = sum(plan.n_windows)
            offsets = [sum(plan.n_windows[:i]) for i in range(len(members) + 1)]
            zero_window_rows += sum(1 for r in rows if r[ph.NW] == 0)
            if NW == 0:
                continue
            want = torch.cat([hist[h][_tempo_rows(first, nW, stride, Tk, rates)]
                              for h, first, nW in zip(members, plan.first_window, plan.n_windows) if nW]).reshape(NW * R, Tk, E)
            before = buf.clone()
            X = torch.full(((NW + 1) * R, Tk, E), -9.0, device=DEV)          # a window larger than needed: its rows must survive
            th.window_sequences(ring, X, table, NW, 0, NW, Tk, stride, rates)
            assert torch.equal(X[:NW * R], want) and bool((X[NW * R:] == -9.0).all()), (stride, rates, step)
            for w0, w1 in ((0, 1), (1, NW - 1), (NW // 2, NW)):
                if w0 < w1:
                    X1 = torch.full(((w1 - w0 + 1) * R, Tk, E), -9.0, device=DEV)
                    th.window_sequences(ring, X1, table, NW, w0, w1, Tk, stride, rates)
                    assert torch.equal(X1[:(w1 - w0) * R], want[w0 * R:w1 * R]) and bool((X1[(w1 - w0) * R:] == -9.0).all())
                    ranges_inside += w0 not in offsets and w1 not in offsets     # starts and ends inside sessions
            assert torch.equal(buf, before)                                   # the ring is only read
        assert min(h.shape[0] for h in hist.values()) > cap                  # every session's ring wrapped
        assert zero_window_rows >= 2 and ranges_inside >= 2, (zero_window_rows, ranges_inside)


def test_tempo_gather_beyond_one_grid():
    """3 * 600 windows of 2 tempos of 32 frames: more rows than 4096 workgroups have waves, the grid-stride loop"""
    from clip_fsar_amd import pool_hip as ph
    from clip_fsar_amd import tempo_hip as th
    g = torch.Generator().manual_seed(2)
    M, cap, Tk, E, nW, rates = 3, 700, 32, 512, 600, (1, 3)
    feats = torch.randn(M * cap, E, generator=g).to(DEV)
    ring = torch.empty(M, cap, E, device=DEV)
    rows = [[slot, 0, cap, i * cap, 0, nW, i * nW, 0] for i, slot in enumerate((1, 2, 0))]
    table = _uploader(M).upload(rows)
    ph.ring_put(feats, ring, table)
    X = torch.empty(M * nW * 2, Tk, E, device=DEV)
    th.window_sequences(ring, X, table, M * nW, 0, M * nW, Tk, 1, rates)
    idx = _tempo_rows(0, nW, 1, Tk, rates)
    assert int(idx.max()) == 599 + 93 < cap
    assert torch.equal(X, feats.view(M, cap, E)[:, idx].reshape(M * nW * 2, Tk, E))


# ------------------------------------------------------------------ 2: the reduction, exactly
def _scores(NW, R, C, seed):
    """[NW * R, C] with ties (a tempo's row copied into another), NaNs in the first, a middle and the last tempo, and rows of -inf"""
    g = torch.Generator().manual_seed(seed)
    s = torch.randn(NW, R, C, generator=g)
    for w in range(NW):
        a, b = w % R, (w * 3 + 1) % R
        if w % 3 == 0 and a != b:
            s[w, b] = s[w, a]                                                 # the whole row tied: the lower of a and b is expected
        if w % 5 == 1:
            s[w, :, w % C] = s[w, 0, w % C]                                   # a cell tied over every tempo
        if w % 4 == 2:
            s[w, (0, R // 2, R - 1)[(w // 4) % 3], (w * 7) % C] = float("nan")
        if w % 7 == 3:
            s[w, :, (w * 5) % C] = float("-inf")
        if w % 7 == 5:
            s[w, w % R, (w * 5) % C] = float("-inf")
    if NW > 8:
        s[8, 0, 0] = s[8, R - 1, 0] = float("nan")                            # two NaNs in one cell: the first one's index
    return s.reshape(NW * R, C).to(DEV)


def _reduce_into(scores, R, off=0):
    """cftp_reduce with sentinels behind both outputs; off: floats by which the three bases are moved off 16 bytes"""
    from clip_fsar_amd import tempo_hip as th
    rows, C = scores.shape
    NW = rows // R
    sbuf = torch.empty(rows * C + 4, device=DEV)
    src = sbuf[off:off + rows * C].view(rows, C)
    src.copy_(scores)
    obuf = torch.full((NW * C + 4 + 64,), -9.0, device=DEV)
    tbuf = torch.full((NW * C + 4 + 64,), -9, device=DEV, dtype=torch.int32)
    out, tempo = obuf[off:off + NW * C].view(NW, C), tbuf[off:off + NW * C].view(NW, C)
    th.reduce(src, out, tempo, R)
    assert bool((obuf[off + NW * C:] == -9.0).all()) and bool((tbuf[off + NW * C:] == -9).all()) and bool((obuf[:off] == -9.0).all())
    assert torch.equal(_bits(src), _bits(scores))                             # the scores are only read
    return out, tempo


@pytest.mark.parametrize("R", [1, 2, 3, 4, 5, 6, 7, 8])
def test_tempo_reduce_is_reference_reduce(R):
    from clip_fsar_amd.pool import reference_reduce
    nans = ties = 0
    for C in (1, 3, 64, 67):
        for NW in (1, 37):
            scores = _scores(NW, R, C, 100 * R + C + NW)
            want_out, want_tempo = reference_reduce(scores, R)
            for off in (0, 1) if C == 64 else (0,):                           # a base one float off 16 bytes: one class per thread
                out, tempo = _reduce_into(scores, R, off)
                assert torch.equal(_bits(out), _bits(want_out)) and torch.equal(tempo, want_tempo), (R, C, NW, off)
                again = _reduce_into(scores, R, off)
                assert torch.equal(_bits(again[0]), _bits(out)) and torch.equal(again[1], tempo)      # two runs, identical bytes
            nans += int(torch.isnan(want_out).sum())
            s = scores.view(NW, R, C)
            ties += int(((s == s.max(1, keepdim=True).values).sum(1) > 1).sum())
            if R == 1:
                assert not bool(tempo.any()) and torch.equal(_bits(out), _bits(scores))              # a copy and a plane of zeros
    assert nans >= 4 and (ties >= 20 or R == 1), (nans, ties)


def test_tempo_reduce_beyond_one_grid():
    from clip_fsar_amd.pool import reference_reduce
    NW, C, R = 600, 8192, 2                                                   # 600 * 2048 threads' worth of quads: past 4096 * 256
    g = torch.Generator().manual_seed(9)
    scores = torch.randn(NW * R, C, generator=g).to(DEV)
    scores[5::7, ::3] = scores[4::7, ::3][:scores[5::7, ::3].shape[0]]        # ties between neighbouring rows
    want_out, want_tempo = reference_reduce(scores, R)
    out, tempo = _reduce_into(scores, R)
    assert torch.equal(_bits(out), _bits(want_out)) and torch.equal(tempo, want_tempo)
    assert 0.3 < float(tempo.float().mean()) < 0.7


# ------------------------------------------------------------------ 3: one rate is the pool as it was
def _tower_feats(gal, arch, ticks, seed):
    need = {}
    for _, tick in ticks:
        for name, n in tick.items():
            need[name] = need.get(name, 0) + n
    eng = gal._fresh_engine()
    feats = {}
    for i, (name, n) in enumerate(sorted(need.items())):
        fr = _frames(arch, 1, n, seed=seed + i)[0]
        feats[name] = torch.empty(n, gal.E, device=DEV)
        for f0 in range(0, n, eng.max_frames):
            eng.vit.forward(fr[f0:f0 + eng.max_frames].contiguous(), feats[name][f0:f0 + eng.max_frames])
    return feats


@pytest.mark.parametrize("kind", ["support-column", "live-class"])
@pytest.mark.parametrize("r", [1, 3])
@pytest.mark.parametrize("smooth", [0.0, 0.5])
def test_one_rate_is_the_pool_with_that_rate(kind, r, smooth):
    """StreamPool(g, rates=(r,)) against StreamPool(g, rate=r) over the contract test's schedule: sessions that open at different
    times and skip pushes, pushes beyond max_push, a close with slot reuse, a reset -- every output bit for bit, tempo all 0"""
    from clip_fsar_amd.baseline import Baseline
    from clip_fsar_amd.events import EventRule
    from clip_fsar_amd.live_gallery import LiveGallery
    from clip_fsar_amd.pool import StreamPool
    arch, Tk, stride = ARCH, T, 2
    head = _head(arch, "fp32", Tk)
    head.args.TRAIN.MERGE_BEFORE = head.args.TRAIN.SINGLE_DIRECT = False
    ticks = _ticks((Tk - 1) * r + 1, stride)
    with torch.no_grad():
        if kind == "support-column":
            gal = _filled(head, arch, Tk)
            opts = dict(smooth=smooth)
        else:
            gal = LiveGallery(head, DEV, capacity=8)
            gal.add_classes(_videos(12, 5), [i // 2 for i in range(12)])
            opts = dict(smooth=smooth, smooth_by="class", events=EventRule(on=0.5, off=-0.5, min_on=1, min_off=1),
                        baseline=Baseline(rate=0.25, warm_rate=0.5, warmup=2, gate=3.0))
        feats = _tower_feats(gal, arch, ticks, 300 + 10 * r)
        old = StreamPool(gal, max_streams=3, stride=stride, rate=r, max_push=6, **opts)
        new = StreamPool(gal, max_streams=3, stride=stride, max_push=6, rates=(r,), **opts)
        assert new.rate == r and new.cap == old.cap and new.rates == (r,)
        a, ha, pushed = _run_schedule(old, ticks, None, feats)
        b, hb, _ = _run_schedule(new, ticks, None, feats)
        windows = 0
        assert sorted(a) == sorted(b) and ha == hb
        for key in a:
            assert a[key][0] == b[key][0] and len(a[key][1]) == len(b[key][1])
            for x, y in zip(a[key][1], b[key][1]):
                assert x.first_window == y.first_window and _same(x.logits, y.logits) and _same(x.smoothed, y.smoothed), key
                assert _same(getattr(x, "deviation", None), getattr(y, "deviation", None)), key
                assert tuple(y.tempo.shape) == tuple(y.logits.shape) and y.tempo.dtype == torch.int32 and not bool(y.tempo.any())
                assert y.rates == (r,) and not hasattr(x, "tempo")
                windows += y.logits.shape[0]
        assert windows == new.stats()["windows"] == old.stats()["windows"] >= 20 and old.stats() == new.stats()
        if kind == "live-class":
            events = new.take_events()
            assert repr(old.take_events()) == repr(events)
            assert [repr(old.active(h)) for h in ha.values()] == [repr(new.active(h)) for h in hb.values()]
            print("one rate %d, smooth %.1f: %d windows, %d events, equal" % (r, smooth, windows, len(events)))
        # the packed form: sessions, first windows, offsets and the planes
        names = sorted(ha)
        more = torch.cat([feats[n][-3:] for n in names])
        po, pn = (p.push_features_packed(more, [h[n] for n in names], [3] * len(names)) for p, h in ((old, ha), (new, hb)))
        assert po.sessions == pn.sessions and po.first_window == pn.first_window and po.offsets == pn.offsets and po.offsets[-1] >= 3
        assert _same(po.logits, pn.logits) and _same(po.smoothed, pn.smoothed) and tuple(pn) == (pn.sessions, pn.first_window, pn.offsets,
                                                                                                   pn.logits, pn.smoothed)
        assert _same(getattr(po, "deviation", None), getattr(pn, "deviation", None)) and not bool(pn.tempo.any())
        assert all(_same(u, v) for u, v in zip(old.topk(po, k=3), new.topk(pn, k=3)))


# ------------------------------------------------------------------ the replay world of tests 4, 5 and 6
C6 = 6
RATES = (1, 2, 3)


class _World:
    pass


@pytest.fixture(scope="module")
def world():
    """a LiveGallery of 6 classes registered from random sequences [6, T, E]: the tower never runs"""
    from clip_fsar_amd.live_gallery import LiveGallery
    w = _World()
    with torch.no_grad():
        w.head = _head(ARCH, "fp32", T)
        w.head.args.TRAIN.MERGE_BEFORE = w.head.args.TRAIN.SINGLE_DIRECT = False
        w.live = LiveGallery(w.head, DEV, capacity=16)
        g = torch.Generator().manual_seed(41)
        w.seqs = torch.randn(C6, T, w.live.E, generator=g).to(DEV)
        assert w.live.add_classes_features(w.seqs, list(range(C6))) == list(range(C6))
        torch.cuda.synchronize()
    return w


def _replay(seqs, c, r, g, noise=0.02):
    """class c's T rows each held r times, with a little noise: [T * r, E]"""
    rows = seqs[c].repeat_interleave(r, 0)
    return rows + noise * torch.randn(rows.shape, generator=g).to(DEV)


def _mixed_stream(seqs, n, seed):
    """n frames: replays of random classes at random holds between runs of noise, under a slowly drifting offset"""
    g = torch.Generator().manual_seed(seed)
    rng = random.Random(seed)
    parts, total = [], 0
    while total < n:
        part = (_replay(seqs, rng.randrange(C6), rng.randint(1, 3), g, 0.05) if rng.random() < 0.6
                else torch.randn(rng.randint(2, 9), seqs.shape[-1], generator=g).to(DEV))
        parts.append(part)
        total += part.shape[0]
    x = torch.cat(parts)[:n]
    return (x + torch.cumsum(0.02 * torch.randn(n, seqs.shape[-1], generator=g), 0).to(DEV)).contiguous()


# ------------------------------------------------------------------ 4: several rates against one pool per rate
@pytest.mark.parametrize("chunked", [False, True])
def test_three_rates_against_three_pools_of_one_rate(world, chunked, monkeypatch):
    """Each reference pool (rate = r) is fed a session's stream without its first (T - 1) * (3 - r) frames: its window k is then tempo
    i of window k.  logits within BOUND (the same clip in another batch) of the largest reference score; tempo equal to the reference
    argmax wherever the reference's best tempo beats its runner-up by more than 2 * BOUND; at most 10 % of the cells may be undecided.
    chunked: 2 windows (6 sequences) per classify_features chunk, so the rounds of several windows run several chunks."""
    from clip_fsar_amd.pool import StreamPool
    live, stride, rmax = world.live, 2, RATES[-1]
    ticks = _ticks((T - 1) * rmax + 1, stride) + [(None, {"a": 9, "c": 14, "d": 11}), (None, {"a": 13, "d": 2, "c": 5})]
    need = {}
    for _, tick in ticks:
        for name, n in tick.items():
            need[name] = need.get(name, 0) + n
    with torch.no_grad():
        if chunked:
            monkeypatch.setattr(live._fresh_engine(), "max_frames", 2 * len(RATES) * T)
        feats = {name: _mixed_stream(world.seqs, n, 50 + i) for i, (name, n) in enumerate(sorted(need.items()))}
        pool = StreamPool(live, max_streams=3, stride=stride, max_push=6, rates=RATES)
        refs = [StreamPool(live, max_streams=1, stride=stride, rate=r, max_push=6) for r in RATES]
        outs, h, pushed = _run_schedule(pool, ticks, None, feats)
        worst, cells, undecided, start, windows, wrapped = 0.0, 0, 0, {}, 0, 0
        for (name, ep), (n, pieces) in sorted(outs.items()):
            k = 0
            for o in pieces:                                                  # every window once, in order
                assert o.first_window == k and o.rates == RATES and o.tempo.shape == o.logits.shape
                k += o.logits.shape[0]
            nW = _n_windows(n, T, stride, rmax)
            assert k == nW, (name, ep, n, k, nW)
            f0 = start.get(name, 0)
            start[name] = f0 + n
            if nW == 0:
                continue
            wrapped += n > pool.cap
            got, tempo = torch.cat([o.logits for o in pieces]), torch.cat([o.tempo for o in pieces])
            per_rate = []
            for r, ref in zip(RATES, refs):
                s = ref.open()
                o = ref.push_features({s: feats[name][f0 + (T - 1) * (rmax - r):f0 + n]})[s]
                ref.close(s)
                assert o.first_window == 0 and tuple(o.logits.shape) == (nW, C6)
                per_rate.append(o.logits)
            stack = torch.stack(per_rate)                                     # [R, nW, C]
            worst = max(worst, maxdiff(got.cpu(), stack.max(0).values.cpu()))
            top2 = stack.topk(2, dim=0).values
            decided = (top2[0] - top2[1]) > 2 * BOUND
            assert torch.equal(tempo[decided].long(), stack.argmax(0)[decided]), (name, ep)
            assert int(tempo.min()) >= 0 and int(tempo.max()) < len(RATES)
            undecided += int((~decided).sum())
            cells += decided.numel()
            windows += nW
        assert pool.stats()["windows"] == windows and pool.stats()["frames"] == pushed         # windows, not windows times R
        torch.cuda.synchronize()
        share = undecided / cells
        print("rates %r (chunked %s): |pool - max over the one-rate pools| = %.2e over %d windows, %d of %d cells undecided (%.2f %%)"
              % (RATES, chunked, worst, windows, undecided, cells, 100 * share))
        assert wrapped >= 2 and windows > 30
        assert share <= 0.10, (undecided, cells)
        assert worst <= BOUND, worst


# ------------------------------------------------------------------ 5: it finds a slowed action
@pytest.mark.parametrize("r", [1, 2, 3])
def test_a_slowed_action_is_found_at_its_tempo(world, r):
    """noise, class c's T rows each held r times, noise.  At the window whose last frame is the replay's last frame, tempo `r` reads
    the last copy of every row: the rates pool's top-1 is c at that tempo, with the logit classify_features gives that sequence alone;
    a rate = 1 pool sees the last T frames -- for r > 1 only the action's second half, stretched -- and scores c lower."""
    from clip_fsar_amd.pool import StreamPool
    live, stride, c = world.live, 2, (2 * r + 1) % C6
    g = torch.Generator().manual_seed(60 + r)
    pre, post = 16, 5
    with torch.no_grad():
        x = torch.cat([torch.randn(pre, live.E, generator=g).to(DEV), _replay(world.seqs, c, r, g),
                       torch.randn(post, live.E, generator=g).to(DEV)]).contiguous()
        last = pre + T * r - 1                                                # the replay's last frame
        k = (last - (T - 1) * RATES[-1]) // stride                            # the window it completes in the rates pool ...
        k1 = (last - (T - 1)) // stride                                       # ... and in the rate = 1 pool
        assert k * stride + (T - 1) * RATES[-1] == last == k1 * stride + (T - 1) and k >= 0
        pool = StreamPool(live, max_streams=2, stride=stride, max_push=6, rates=RATES)
        plain = StreamPool(live, max_streams=2, stride=stride, rate=1, max_push=6)
        pool.close(pool.open())                                               # the session is not handle 0
        h, h1 = pool.open(), plain.open()
        logits, tempo, logits1, t = [], [], [], 0
        for n in (5, 1, 6, 3, 6, 2, 4, 6, 6, 6, 6, 6):
            n = min(n, x.shape[0] - t)
            if n == 0:
                break
            o, o1 = pool.push_features({h: x[t:t + n]})[h], plain.push_features({h1: x[t:t + n]})[h1]
            assert o.first_window == sum(p.shape[0] for p in logits) and o1.first_window == sum(p.shape[0] for p in logits1)
            logits.append(o.logits), tempo.append(o.tempo), logits1.append(o1.logits)
            if o.first_window <= k < o.first_window + o.logits.shape[0]:
                values, index = pool.topk(o, k=1)                             # topk takes the tempo outputs as it takes their bases
                assert int(index[k - o.first_window, 0]) == c
            t += n
        logits, tempo, logits1 = torch.cat(logits), torch.cat(tempo), torch.cat(logits1)
        assert int(logits[k].argmax()) == c and int(tempo[k, c]) == RATES.index(r)
        seq = x[torch.tensor([last - (T - 1 - j) * r for j in range(T)], device=DEV)]
        alone = live.classify_features(seq[None].contiguous())[0]
        gap = float(logits[k, c] - logits1[k1, c])
        print("held %d times: class %d at window %d, tempo %d; pool %.6f, alone %.6f, the rate = 1 pool %.6f (gap %.3e)"
              % (r, c, k, int(tempo[k, c]), float(logits[k, c]), float(alone[c]), float(logits1[k1, c]), gap))
        assert abs(float(logits[k, c]) - float(alone[c])) <= BOUND
        if r > 1:
            assert gap > 2 * BOUND, gap
        else:
            assert abs(gap) <= BOUND                                          # at r = 1 the rate = 1 pool sees the same clip


# ------------------------------------------------------------------ 6: enrolment and explain at a tempo
def test_enroll_and_explain_at_a_tempo_on_a_wrapped_ring():
    """enroll(h, id, window=w, tempo=i) gives the prototype bits of add_classes_features on the materialised rows; explain(..., tempo=i)
    is Aligner.align_features of them, bit for bit; tempo=None is tempo=R - 1; neither changes a later push's outputs"""
    from clip_fsar_amd.align import Aligner
    from clip_fsar_amd.pool import StreamPool
    stride, max_push = 2, 6
    g = torch.Generator().manual_seed(83)
    with torch.no_grad():
        head, live, _ = _pair(capacity=16)
        ref = _pair(capacity=16)[1]
        seqs = torch.randn(C6, T, live.E, generator=g).to(DEV)
        live.add_classes_features(seqs, list(range(C6)))
        ref.add_classes_features(seqs, list(range(C6)))
        asked = StreamPool(live, max_streams=3, stride=stride, max_push=max_push, rates=RATES)
        quiet = StreamPool(live, max_streams=3, stride=stride, max_push=max_push, rates=RATES)
        assert asked.cap == (T - 1) * 3 + max_push
        asked.close(asked.open()), quiet.close(quiet.open())
        ha, hq = asked.open(), quiet.open()
        x = _mixed_stream(seqs, 90, 84)
        t = 0
        for n in (5, 6, 3, 6, 6, 1, 6, 6, 4, 6, 6, 6, 2, 6):                  # 69 frames: the ring wrapped more than twice
            for p, h in ((asked, ha), (quiet, hq)):
                p.push_features({h: x[t:t + n]})
            t += n
        assert t > 2 * asked.cap
        ok = asked.enrolable(ha)
        assert len(ok) >= 3 and ok == quiet.enrolable(hq)
        ring, stats = asked._ring.clone(), (asked.stats(), asked.stats(ha))

        def rows(w, i):
            return x[torch.tensor([w * stride + (T - 1) * 3 - (T - 1 - j) * RATES[i] for j in range(T)], device=DEV)][None].contiguous()

        al = Aligner(live)
        text = torch.randn(live.E, generator=g)
        new_id = 10
        for w in (ok[0], ok[1], ok[-1]):
            for i in (0, 1, 2, None):
                ii = len(RATES) - 1 if i is None else i
                for cls in ([3], [0, 5]):                                     # explain first: the class list is the same on both sides
                    a = asked.explain(ha, cls, window=w, tempo=i)
                    want = al.align_features(rows(w, ii), classes=cls)
                    assert all(torch.equal(_bits(u), _bits(v)) for u, v in ((a.plan, want.plan), (a.dists, want.dists),
                                                                            (a.logits, want.logits))), (w, i)
                cid = "new" if (w, i) == (ok[0], 0) else new_id
                kw = {"text": {"new": text}} if cid == "new" else {}
                assert asked.enroll(ha, cid, window=w, tempo=i, **kw) == 1
                assert ref.add_classes_features(rows(w, ii), [cid], **kw) == [live.class_ids.index(cid)]
                new_id += 1
        _assert_same_classes(live, ref)
        assert asked.enroll(ha, 3, tempo=1) == 2 and ref.add_shots_features(rows(ok[-1], 1), [3]) == [2]      # a further shot, the newest
        assert asked.enroll_windows([(ha, ok[0], 4), (ha, None, "new")], tempo=0) == {4: 2, "new": 2}
        assert ref.add_shots_features(torch.cat([rows(ok[0], 0), rows(ok[-1], 0)]), [4, "new"]) == [2, 2]
        _assert_same_classes(live, ref)
        a, b = asked.explain(ha, k=2), asked.explain(ha, k=2, tempo=2)
        assert torch.equal(_bits(a.plan), _bits(b.plan)) and torch.equal(a.pairs, b.pairs)
        assert torch.equal(asked._ring, ring) and (asked.stats(), asked.stats(ha)) == stats
        for n in (4, 6, 6, 5):                                                # the later pushes: the asked pool as the quiet one
            u, v = asked.push_features({ha: x[t:t + n]})[ha], quiet.push_features({hq: x[t:t + n]})[hq]
            assert u.first_window == v.first_window and _same(u.logits, v.logits) and _same(u.tempo, v.tempo)
            assert u.logits.shape[1] == len(live.class_ids) == C6 + 12
            t += n
