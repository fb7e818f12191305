"""GPU: enrolment (clip_fsar_amd.pool.StreamPool.enroll / enroll_windows on libclipfsar_enroll.so) -- the ring-to-support-sequence kernel
bit for bit against the indexing expression at its path and grid edges, LiveGallery's registration from features against its pixel forms,
enrol_windows against registration from the windows materialised by indexing, that the tower does not run, pixels pushed and enrolled
against add_classes of the clip, and what sessions see afterwards."""
import random

import pytest
import torch

import clip_fsar_amd.synth as synth
from _cases import maxdiff
from test_gpu_live import ARCH, BOUND, CONFIGS, DEV, IDS, T, _dense, _pair, _videos

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ 1: the kernel, exactly
def _check_kernel(Tk, rate, max_push, E, M, n_cls, rows, x0_offset=0, dev_rows=None, seed=0):
    """rows: the enrolment list (slot, pos, cls).  The ring is NaN but for the positions the rows name, so a read anywhere else shows in
    the output; X0 lies inside a larger buffer whose rest must stay as it was.  dev_rows: another list for the device copy, behind the
    valid host rows -- where it differs from rows and is out of range, the sequence must be NaN."""
    from clip_fsar_amd import enroll_hip as eh
    from clip_fsar_amd import pool_hip as ph
    cap, n = (Tk - 1) * rate + max_push, len(rows)
    g = torch.Generator().manual_seed(seed)
    ring = torch.full((M, cap, E), float("nan"))
    for slot, pos, _ in rows:
        for j in range(Tk):
            ring[slot, (pos + j * rate) % cap] = torch.randn(E, generator=g)
    ring, text = ring.to(DEV), torch.randn(n_cls, E, generator=g).to(DEV)
    size = n * (Tk + 1) * E
    buf = torch.full((x0_offset + size + E,), -7.0, device=DEV)
    X0 = buf[x0_offset:x0_offset + size].view(n, Tk + 1, E)
    assert (X0.data_ptr() % 16 != 0) == bool(x0_offset % 4)
    table = eh.table_uploader(DEV, n).upload(eh.table_rows(*zip(*rows)))
    if dev_rows is not None:
        table = ph.Table(table.host, torch.tensor(eh.table_rows(*zip(*dev_rows)), dtype=torch.int32, device=DEV), n)
    eh.ring_sequences(ring, text, table, X0, rate)
    torch.cuda.synchronize()
    assert bool((buf[:x0_offset] == -7.0).all()) and bool((buf[x0_offset + size:] == -7.0).all())        # the sentinel rows
    for i, (slot, pos, cls) in enumerate(rows):
        if dev_rows is not None and tuple(dev_rows[i]) != (slot, pos, cls):
            assert bool(torch.isnan(X0[i]).all()), i
            continue
        want = torch.cat([ring[slot, (pos + j * rate) % cap] for j in range(Tk)] + [text[cls]])
        assert bool(torch.isfinite(X0[i]).all()), (i, "a ring position outside the window was read")
        assert torch.equal(X0[i].reshape(-1), want), i
    return X0


def test_same_slot_eight_times_every_wrap():
    """cap = T = 8: the window at POS = p wraps after 8 - p rows, every window but the one at 0"""
    _check_kernel(8, 1, 1, 64, 2, 3, [(1, p, p % 3) for p in range(8)])


def test_4_byte_pieces_and_a_rate():
    _check_kernel(5, 3, 2, 33, 3, 2, [(0, 0, 0), (2, 13, 1), (2, 13, 1), (0, 5, 1), (2, 6, 0)])


def test_one_frame_one_position():
    _check_kernel(1, 1, 1, 4, 1, 1, [(0, 0, 0)])
    _check_kernel(1, 7, 1, 4, 2, 2, [(1, 0, 1), (0, 0, 0), (1, 0, 0)])


def test_more_rows_than_one_grid_pass():
    """600 sequences of 33 rows: 19 800 rows, past the 4 096 workgroups x 4 waves of one pass"""
    rng = random.Random(5)
    cap = 31 * 2 + 64
    _check_kernel(32, 2, 64, 64, 4, 9, [(rng.randrange(4), rng.randrange(cap), rng.randrange(9)) for _ in range(600)])


def test_misaligned_output_takes_the_4_byte_path():
    rows = [(2, 9, 1), (0, 0, 0), (2, 3, 1)]
    _check_kernel(8, 1, 4, 512, 3, 2, rows, x0_offset=1)
    _check_kernel(8, 1, 4, 512, 3, 2, rows, x0_offset=4)          # the same call on 16-byte pieces


def test_a_device_row_out_of_range_poisons_its_sequence_alone():
    rows = [(0, 0, 0), (2, 13, 1), (1, 4, 1), (0, 5, 1), (2, 6, 0), (1, 7, 0)]
    for bad in ({1: (3, 13, 1), 3: (0, 14, 1), 5: (1, 7, 2)}, {0: (-1, 0, 0), 2: (1, -4, 1), 4: (2, 6, -1)},
                {1: (1 << 30, 13, 1), 3: (0, 1 << 30, 1), 5: (1, 7, 1 << 30)}):
        for E in (64, 33):
            _check_kernel(5, 3, 2, E, 3, 2, rows, dev_rows=[bad.get(i, r) for i, r in enumerate(rows)])


# ------------------------------------------------------------------ 2: registration from features
def _tower(g, videos):
    out = torch.empty(videos.shape[0], T, g.E, device=DEV)
    g._features(g._fresh_engine(), videos, out)
    return out


def _bits(t):
    return t.contiguous().view(torch.int32)        # NaN-proof equality: never-written slots of a store hold whatever was there


def _state(g):
    st = g._store
    return (g.layout_version, g.class_ids, [g.shots(c) for c in g.class_ids], {k: _bits(v).clone() for k, v in st.items()},
            st["P"].data_ptr())


def _same_state(a, b):
    return a[:3] == b[:3] and a[4] == b[4] and all(torch.equal(a[3][k], b[3][k]) for k in a[3])


def _assert_same_classes(a, b):
    """two LiveGalleries hold the same classes: ids, shots, slots, and bit for bit prototypes, norms, text rows and sums"""
    assert a.class_ids == b.class_ids and [a.shots(c) for c in a.class_ids] == [b.shots(c) for c in b.class_ids]
    assert [a.slot_of(c) for c in a.class_ids] == [b.slot_of(c) for c in b.class_ids]
    (Pa, pna), (Pb, pnb) = _dense(a), _dense(b)
    assert torch.equal(Pa, Pb) and torch.equal(pna, pnb) and bool(torch.isfinite(Pa).all())
    idx = torch.tensor([a.slot_of(c) for c in a.class_ids], device=DEV)
    assert torch.equal(a._store["text"][idx], b._store["text"][idx])
    rows = T + 1 if a.merge_before else T          # the sums of context2's outputs stop at its T frame rows; row T is never written
    assert torch.equal(a._store["sums"][idx, :rows], b._store["sums"][idx, :rows])


@pytest.mark.parametrize("precision,merge_before,single_direct", CONFIGS)
def test_features_forms_equal_the_pixel_forms(precision, merge_before, single_direct):
    V, W, Q = _videos(12, 61), _videos(5, 62), _videos(6, 63)
    with torch.no_grad():
        head, px, _ = _pair(precision, merge_before, single_direct)
        ft = _pair(precision, merge_before, single_direct)[1]
        assert px.add_classes(V[:8], IDS[:8]) == ft.add_classes_features(_tower(ft, V[:8]), IDS[:8]) == [0, 1, 2, 3]
        text = {"kite": torch.randn(px.E, generator=torch.Generator().manual_seed(64))}
        ids = [7, "kite", 9, 9]
        assert px.add_classes(V[8:], ids, text=text) == ft.add_classes_features(_tower(ft, V[8:]), ids, text=text) == [4, 5, 6]
        _assert_same_classes(px, ft)
        ids = [9, 0, "kite", 9, 2]
        assert px.add_shots(W, ids) == ft.add_shots_features(_tower(ft, W), ids) == [4, 3, 2, 4]
        _assert_same_classes(px, ft)
        assert torch.equal(px.classify(Q), ft.classify(Q))
        with pytest.raises(ValueError, match="feats must be"):
            ft.add_shots_features(_tower(ft, W)[:, :T - 1], ids)
        with pytest.raises(ValueError, match="already registered"):
            ft.add_classes_features(_tower(ft, W[:1]), [9])
        _assert_same_classes(px, ft)


# ------------------------------------------------------------------ 3: the pool
def _window(hist, w, stride, rate):
    return hist[torch.tensor([w * stride + j * rate for j in range(T)], device=DEV)]


@pytest.mark.parametrize("precision,merge_before,single_direct", CONFIGS)
def test_enroll_windows_equals_registration_from_the_materialised_windows(precision, merge_before, single_direct, monkeypatch):
    from clip_fsar_amd.pool import StreamPool
    stride, rate, max_push = 2, 2, 5
    V = _videos(12, 71)
    g = torch.Generator().manual_seed(72)
    with torch.no_grad():
        head, live, _ = _pair(precision, merge_before, single_direct)
        ref = _pair(precision, merge_before, single_direct)[1]
        live.add_classes(V, IDS)
        ref.add_classes(V, IDS)
        E = live.E
        pool = StreamPool(live, max_streams=3, stride=stride, rate=rate, max_push=max_push)
        assert pool.cap == 19
        pool.close(pool.open())
        a, b = pool.open(), pool.open()                       # slots 0 and 1, handles 1 and 2
        hist = {a: torch.randn(53, E, generator=g).to(DEV), b: torch.randn(47, E, generator=g).to(DEV)}
        for f0 in range(0, 53, 7):                            # pushes of 7 (two rounds each); b ends earlier: more than two wraps each
            pool.push_features({h: x[f0:f0 + 7] for h, x in hist.items() if f0 < x.shape[0]})
        assert pool.stats(a)["frames"] == 53 and pool.stats(b)["frames"] == 47
        ra, rb = pool.enrolable(a), pool.enrolable(b)
        assert ra == range(17, 20) and rb == range(14, 17)    # windows whose first frame 2 w is one of the last 19, and complete
        stats = (pool.stats(), pool.stats(a), pool.stats(b))
        ring = pool._ring.clone()

        # the windows below and above the range, alone and behind a good item: ValueError, and nothing moved
        before = _state(live)
        for h, r in ((a, ra), (b, rb)):
            for w in (r.start - 1, r.stop):
                with pytest.raises(ValueError, match=r"session %d: window %d is not enrolable -- the ring holds its windows range\(%d, %d\)"
                                   % (h, w, r.start, r.stop)):
                    pool.enroll_windows([(a, None, 11), (b, None, 0), (h, w, 0)])
                with pytest.raises(ValueError, match="not enrolable"):
                    pool.enroll(h, 12, window=w)
        with pytest.raises(ValueError, match="class 'glider' is not an index into TEST.CLASS_NAME"):
            pool.enroll_windows([(a, None, 11), (b, None, 0), (b, None, "glider")])
        assert _same_state(_state(live), before)

        # the tower must not run from here on
        eng = live._fresh_engine()

        def no_tower(*args, **kw):
            raise AssertionError("the tower ran during enrolment")

        real = eng.vit.forward
        monkeypatch.setattr(eng.vit, "forward", no_tower)
        # new classes 11 (three shots over both sessions) and "kite" (a text row), further shots of 0 (two windows of one session) and 9:
        # the oldest and the newest enrolable window of both sessions are among them
        row = torch.randn(E, generator=g)
        items = [(a, ra[0], 11), (b, rb[-1], 0), (a, None, "kite"), (b, rb[0], 11), (b, rb[1], 0), (a, ra[-1], 11), (a, ra[1], 9)]
        got = pool.enroll_windows(items, text={"kite": row})
        assert got == {11: 3, 0: 4, "kite": 1, 9: 4} and list(got) == [11, 0, "kite", 9]
        assert pool.enroll(b, 9) == 5 and pool.enroll(b, 13, window=rb[1]) == 1
        monkeypatch.setattr(eng.vit, "forward", real)
        assert (pool.stats(), pool.stats(a), pool.stats(b)) == stats and torch.equal(pool._ring, ring)
        assert live.layout_version == before[0]

        win = lambda h, w: _window(hist[h], pool.enrolable(h)[-1] if w is None else w, stride, rate)
        shots = [(h, w, c) for h, w, c in items if c in (0, 9)]
        assert ref.add_shots_features(torch.stack([win(h, w) for h, w, _ in shots]), [c for _, _, c in shots]) == [4, 4]
        news = [(h, w, c) for h, w, c in items if c in (11, "kite")]
        assert ref.add_classes_features(torch.stack([win(h, w) for h, w, _ in news]), [c for _, _, c in news], text={"kite": row}) == [6, 7]
        assert ref.add_shots_features(win(b, None)[None], [9]) == [5]
        assert ref.add_classes_features(win(b, rb[1])[None], [13]) == [8]
        _assert_same_classes(live, ref)
        assert live.class_ids == [0, 1, 2, 5, 7, 9, 11, "kite", 13]

        # the next push of a session without a list has the new columns, and scores them as classify does
        more = torch.randn(4, E, generator=g).to(DEV)
        hist[a] = torch.cat([hist[a], more])
        out = pool.push_features({a: more})[a]
        assert out.first_window == 20 and tuple(out.logits.shape) == (2, 9)
        clips = torch.stack([_window(hist[a], w, stride, rate) for w in (20, 21)])
        assert torch.equal(out.logits, live.classify_features(clips)) and torch.equal(out.logits, ref.classify_features(clips))


def test_tenant_sessions_join_and_smoothing_pools():
    from clip_fsar_amd.pool import StreamPool
    V = _videos(12, 81)
    g = torch.Generator().manual_seed(82)
    with torch.no_grad():
        head, live, _ = _pair()
        live.add_classes(V, IDS)
        E = live.E
        pool = StreamPool(live, max_streams=3, stride=1, max_push=8)
        ten, other, free = pool.open(classes=[9, 2]), pool.open(classes=[5]), pool.open()
        hist = {h: torch.randn(12, E, generator=g).to(DEV) for h in (ten, other, free)}
        pool.push_features(hist)
        version = live.layout_version
        assert pool.enroll(ten, 15) == 1                              # a new class; no join: the tenant's list stays
        assert pool.enroll(other, 16, window=pool.enrolable(other)[0], join=True) == 1
        assert pool._sessions[ten].classes == [9, 2] and pool._sessions[other].classes == [5, 16] and pool._sessions[free].classes is None
        assert pool.enroll(ten, 9, join=True) == 4 and pool._sessions[ten].classes == [9, 2]      # a further shot of a listed class
        assert live.shots(9) == 4 and live.layout_version == version and live.class_ids == [0, 1, 2, 5, 7, 9, 15, 16]
        # one grouped launch scores the three sessions' windows: bit for bit what the gallery's grouped call gives on the materialised
        # windows, and per session classify_features of its own list -- another batch through context2, so held to the project's bound
        more = {h: torch.randn(2, E, generator=g).to(DEV) for h in hist}
        out = pool.push_features(more)
        clips = {h: torch.stack([torch.cat([hist[h], more[h]])[w:w + T] for w in (5, 6)]) for h in hist}
        lists = {ten: [9, 2], other: [5, 16], free: None}
        res = live.classify_features_grouped(torch.cat([clips[h] for h in hist]), [2, 2, 2], [lists[h] for h in hist])
        for i, h in enumerate(hist):
            width = 8 if lists[h] is None else 2
            assert tuple(out[h].logits.shape) == (2, width) and torch.equal(out[h].logits, res.group(i)), h
            want = live.classify_features(clips[h], classes=lists[h])
            d = maxdiff(out[h].logits.cpu(), want.cpu())
            print("session %d after enrolment, classes %s: |pool - classify_features| = %.2e" % (h, lists[h], d))
            assert d <= BOUND and torch.equal(out[h].logits.argmax(1), want.argmax(1)), (h, d)
        assert pool.enroll(ten, 15, join=True) == 2 and pool._sessions[ten].classes == [9, 2, 15]
        out = pool.push_features({ten: more[ten][:1]})[ten]
        assert tuple(out.logits.shape) == (1, 3)
        clip = torch.cat([hist[ten], more[ten], more[ten][:1]])[7:7 + T][None]
        assert torch.equal(out.logits, live.classify_features(clip, classes=[9, 2, 15]))          # one window, one clip: the same launches

        # smoothing on: a further shot changes no column and asks for nothing; a new class changes the count: the stale-state rule
        smooth = StreamPool(live, max_streams=2, stride=1, max_push=8, smooth=0.5)
        s = smooth.open()
        smooth.push_features({s: hist[free]})
        assert smooth.enroll(s, 0) == 3
        assert smooth.push_features({s: more[free]})[s].smoothed.shape == (2, 8)
        assert smooth.enroll(s, 17) == 1
        with pytest.raises(RuntimeError, match=r"reset\(\) the session"):
            smooth.push_features({s: more[free]})
        smooth.reset(s)
        assert smooth.enrolable(s) == range(0)
        with pytest.raises(ValueError, match="not enrolable"):
            smooth.enroll(s, 0)
        assert smooth.push_features({s: hist[free]})[s].smoothed.shape == (5, 9)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_pushed_pixels_enrolled_against_add_classes_of_the_clip(precision):
    """push of frames, then enroll, against add_classes / add_shots of the clip cut from those frames: 'same clip, another batch' (the
    tower picks its kernels by row count), so the logits of held-out queries are held to the project's 2e-5 with equal argmax.  The
    measured difference is printed."""
    from clip_fsar_amd.pool import StreamPool
    a = synth.ARCHS[ARCH]
    V, Q = _videos(12, 91), _videos(12, 92)
    frames = (torch.randn(21, 3, a["res"], a["res"], generator=torch.Generator().manual_seed(93)) * 0.5).to(DEV)
    with torch.no_grad():
        head, live, _ = _pair(precision)
        ref = _pair(precision)[1]
        live.add_classes(V, IDS)
        ref.add_classes(V, IDS)
        pool = StreamPool(live, max_streams=2, stride=3, max_push=6)           # cap 13
        h = pool.open()
        pool.push({h: frames[:10]})
        pool.push({h: frames[10:]})
        r = pool.enrolable(h)
        assert r == range(3, 5)                                                # 21 frames: windows 0 .. 4 complete, frames 8 .. 20 kept
        assert pool.enroll(h, 11) == 1 and pool.enroll(h, 2, window=3) == 4
        clip = lambda w: frames[w * 3:w * 3 + T][None]
        assert ref.add_classes(clip(4), [11]) == [6] and ref.add_shots(clip(3), [2]) == [4]
        got, want = live.classify(Q), ref.classify(Q)
    d = maxdiff(got.cpu(), want.cpu())
    print("push + enroll vs add_classes / add_shots of the clip, %s: |dlogits| = %.2e over %d queries x %d classes" % (
        precision, d, got.shape[0], got.shape[1]))
    assert tuple(got.shape) == (12, 7)
    assert d <= BOUND, d
    assert torch.equal(got.argmax(1), want.argmax(1))
