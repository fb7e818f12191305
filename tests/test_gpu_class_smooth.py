"""GPU: per-class smoothing (clip_fsar_amd.pool.StreamPool(smooth_by="class") on libclipfsar_class_smooth.so) -- the kernel through its
binding, bit for bit against cfss_smooth_logits on every (session, class) pair's own column at the workgroup edges, with shared and
overlapping lists, valid and stale marks, sessions without windows, keys out of range, aliasing and split calls, and against a float64
restatement with the derived bound; then the pool: against the column mode where both apply, with class lists, through membership changes
while sessions run (enrolment, join, further shots, removals, a slot's new owner, store growth) over a LiveGallery and a COMBINE
LiveTextGallery, and after reset() and in a reused slot."""
import random

import pytest
import torch

from test_gpu_live import DEV, T, _pair

pytestmark = pytest.mark.gpu

CAP, M = 300, 6                                   # store slots, session slots
PAD, NAN = 37, float("nan")
CHUNK = 256                                       # class_smooth_hip.CHUNK, the kernel's columns per workgroup (asserted below)


# ------------------------------------------------------------------ 1: the kernel, through the binding
def _padded(t, sentinel):
    """t inside a larger buffer with PAD sentinels on either side -> (buffer, the view holding t)"""
    buf = torch.full((t.numel() + 2 * PAD,), sentinel, dtype=t.dtype, device=DEV)
    view = buf[PAD:PAD + t.numel()].view(t.shape)
    view.copy_(t)
    return buf, view


def _intact(buf, sentinel):
    return bool((buf[:PAD] == sentinel).all()) and bool((buf[-PAD:] == sentinel).all())


def _bits(t):
    return t.contiguous().view(torch.int32)        # NaN-proof equality


def _pair_reference(x, y_before, alpha):
    """cfss_smooth_logits on one pair's own column x [n] -> (y [n], the state it leaves); y_before: a 0-dim tensor, or None: no state"""
    from clip_fsar_amd import stream_hip as sh
    n = x.shape[0]
    state = torch.full((1, 1), NAN, device=DEV) if y_before is None else y_before.reshape(1, 1).clone()
    out = torch.empty(1, n, 1, device=DEV)
    sh.smooth_logits(x.contiguous().view(1, n, 1), state, out, alpha, 0 if y_before is None else 1)
    return out.view(n), state.view(())


class _Cells:
    """state, marks and gens of a kernel test: every cell NaN with a garbage mark, but the cells `named` (slot, key) -- each of those valid
    (its mark the slot's generation, a finite y) or stale (another mark, y NaN, so a read of it shows) at random"""

    def __init__(self, named, seed, all_stale=False):
        rng = random.Random(seed)
        g = torch.Generator().manual_seed(seed)
        self.gens0 = torch.randint(1, 6, (CAP,), generator=g, dtype=torch.int32)
        state = torch.full((M, CAP), NAN)
        marks = torch.randint(-3, 9, (M, CAP), generator=g, dtype=torch.int32)
        self.valid = {}
        for slot, key in sorted(named):
            gen = int(self.gens0[key])
            ok = not all_stale and rng.random() < 0.5
            marks[slot, key] = gen if ok else rng.choice((0, gen - 1, gen + 1, -gen))
            if ok:
                state[slot, key] = rng.uniform(-20.0, 5.0)
            self.valid[(slot, key)] = ok
        self.state0, self.marks0 = state.to(DEV), marks.to(DEV)
        self.bufs = {"state": _padded(self.state0, -12345.0), "marks": _padded(self.marks0, -77), "gens": _padded(self.gens0.to(DEV), -77)}

    def __getattr__(self, name):
        return self.bufs[name][1]

    def intact(self):
        return all(_intact(buf, -77 if buf.dtype == torch.int32 else -12345.0) for buf, _ in self.bufs.values())


def _launch(cells, rows, keys, x, alpha, alias, uploader):
    """rows: (slot, nW, key0, NC) -> the flat out; logits, keys and out lie between sentinels, which must survive"""
    from clip_fsar_amd import class_smooth_hip as ch
    assert ch.CHUNK == CHUNK
    table, n_out, chunks = [], 0, 0
    for slot, nW, key0, NC in rows:
        table.append([slot, nW, n_out, NC, key0, chunks])
        n_out += nW * NC
        chunks += -(-NC // CHUNK)
    assert n_out == x.numel()
    kbuf, kd = _padded(torch.tensor(keys, dtype=torch.int32), -77)
    xbuf, xd = _padded(x, -12345.0)
    obuf, od = (xbuf, xd) if alias else _padded(torch.full_like(x, 7.0), -12345.0)
    ch.smooth_classes(xd, cells.state, cells.marks, cells.gens, kd, od, uploader.upload(table), alpha)
    torch.cuda.synchronize()
    assert _intact(kbuf, -77) and _intact(xbuf, -12345.0) and _intact(obuf, -12345.0) and cells.intact()
    assert torch.equal(kd.cpu(), torch.tensor(keys, dtype=torch.int32)) and torch.equal(cells.gens.cpu(), cells.gens0)
    if not alias:
        assert torch.equal(xd.cpu(), x)            # the input is read only
    return od.clone()


def _check_case(rows, keys, alpha, seed, alias=False, all_stale=False):
    from clip_fsar_amd import class_smooth_hip as ch
    named = {(slot, keys[key0 + j]) for slot, nW, key0, NC in rows for j in range(NC) if 0 <= keys[key0 + j] < CAP}
    cells = _Cells(named, seed, all_stale)
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.randn(sum(nW * NC for _, nW, _, NC in rows), generator=g) * 6.0 - 9.0
    out = _launch(cells, rows, keys, x, alpha, alias, ch.table_uploader(DEV, M))
    want_state, want_marks = cells.state0.clone(), cells.marks0.clone()
    xd, at = x.to(DEV), 0
    for slot, nW, key0, NC in rows:
        blk, got = xd[at:at + nW * NC].view(nW, NC), out[at:at + nW * NC].view(nW, NC)
        at += nW * NC
        for j in range(NC if nW else 0):
            key = keys[key0 + j]
            if not 0 <= key < CAP:                 # never dereferenced: a NaN column and no state write
                assert bool(torch.isnan(got[:, j]).all()), (slot, j, key)
                continue
            before = cells.state0[slot, key] if cells.valid[(slot, key)] else None
            y, last = _pair_reference(blk[:, j], before, alpha)
            assert bool(torch.isfinite(y).all()) and torch.equal(got[:, j], y), (slot, j, key, cells.valid[(slot, key)])
            want_state[slot, key] = last
            want_marks[slot, key] = cells.gens0[key]
    torch.cuda.synchronize()
    # every cell no list names -- and every cell of a session without windows -- comes back bit for bit; the named ones hold the last y
    assert torch.equal(_bits(cells.state), _bits(want_state)) and torch.equal(cells.marks, want_marks)
    return cells, out


def _perm(n, seed):
    return torch.randperm(CAP, generator=torch.Generator().manual_seed(seed))[:n].tolist()


@pytest.mark.parametrize("alpha", [0.0, 0.5, 0.9])
@pytest.mark.parametrize("width", [1, CHUNK - 1, CHUNK, CHUNK + 1])
def test_one_session_at_the_workgroup_edges(width, alpha):
    for nW, alias in ((5, False), (1, True), (0, False)):
        _check_case([(3, nW, 0, width)], _perm(width, width), alpha, seed=width + nW, alias=alias)


@pytest.mark.parametrize("alpha", [0.0, 0.5, 0.9])
def test_four_sessions_sharing_one_list_and_an_overlapping_one(alpha):
    """three sessions point at one list of 257 store slots (one of them has no window: its state and marks come back bit for bit), the
    fourth at a list that starts and ends inside it"""
    keys = _perm(CAP, 11)
    rows = [(5, 2, 0, CHUNK + 1), (0, 0, 0, CHUNK + 1), (2, 1, 0, CHUNK + 1), (4, 5, 45, CHUNK - 1)]
    for alias in (False, True):
        _check_case(rows, keys, alpha, seed=21 + alias, alias=alias)
    _check_case(rows, keys, alpha, seed=23, all_stale=True)                      # every pair starts: no state is read at all


@pytest.mark.parametrize("alpha", [0.0, 0.5, 0.9])
def test_four_sessions_of_four_widths(alpha):
    keys = _perm(CAP, 12)
    _check_case([(1, 5, 10, 1), (3, 1, 0, CHUNK - 1), (0, 2, 44, CHUNK), (5, 0, 299, 1)], keys, alpha, seed=31)
    _check_case([(1, 0, 10, 1), (3, 2, 0, CHUNK + 1), (0, 5, 43, CHUNK + 1), (5, 1, 299, 1)], keys, alpha, seed=32, alias=True)


@pytest.mark.parametrize("bad", [-1, CAP, 1 << 30])
def test_a_key_out_of_range_gives_a_nan_column_and_writes_no_state(bad):
    keys = _perm(CAP, 13)
    for j in (0, 7, CHUNK - 1, CHUNK, 298):
        keys[j] = bad
    _check_case([(2, 5, 0, CHUNK + 1), (4, 2, 200, 100), (0, 0, 0, 8)], keys, 0.5, seed=41)
    _check_case([(2, 1, 7, 1)], keys, 0.9, seed=42, alias=True)


def test_windows_split_over_several_calls_give_the_bits_of_one_call():
    from clip_fsar_amd import class_smooth_hip as ch
    keys = _perm(CAP, 14)
    geometry = [(5, 0, CHUNK + 1), (0, 0, CHUNK + 1), (2, 45, CHUNK - 1), (4, 299, 1)]              # (slot, key0, NC)
    totals, splits = [5, 0, 2, 5], [[1, 1, 3], [0, 0, 0], [1, 0, 1], [2, 3, 0]]                  # a session may sit a call out
    named = {(slot, keys[key0 + j]) for slot, key0, NC in geometry for j in range(NC)}
    g = torch.Generator().manual_seed(51)
    blocks = [torch.randn(n, NC, generator=g) * 6.0 - 9.0 for n, (_, _, NC) in zip(totals, geometry)]
    up = ch.table_uploader(DEV, M)
    for alpha in (0.5, 0.9):
        one = _Cells(named, 52)
        whole = _launch(one, [(s, n, k0, NC) for n, (s, k0, NC) in zip(totals, geometry)], keys, torch.cat([b.reshape(-1) for b in blocks]),
                        alpha, False, up)
        parts = _Cells(named, 52)
        done, pieces = [0] * 4, [[] for _ in geometry]
        for call in range(3):
            take = [sp[call] for sp in splits]
            x = torch.cat([b[d:d + n].reshape(-1) for b, d, n in zip(blocks, done, take)])
            out = _launch(parts, [(s, n, k0, NC) for n, (s, k0, NC) in zip(take, geometry)], keys, x, alpha, call == 1, up)
            at = 0
            for i, (n, (_, _, NC)) in enumerate(zip(take, geometry)):
                pieces[i].append(out[at:at + n * NC])
                at += n * NC
                done[i] += n
        assert done == totals
        assert torch.equal(torch.cat([p for ps in pieces for p in ps]), whole)
        assert torch.equal(_bits(parts.state), _bits(one.state)) and torch.equal(parts.marks, one.marks)


@pytest.mark.parametrize("alpha", [0.5, 0.9])
def test_against_float64_with_the_derived_bound(alpha):
    """Each step rounds the product (1 - alpha) * x and the fma, each by at most eps * max|x| (|y| <= max|x|: a convex combination),
    eps = 2^-24, so e_k <= alpha * e_{k-1} + 2 eps max|x| <= 2 eps max|x| / (1 - alpha); the test asserts twice that, as the stream
    library's own test does."""
    from clip_fsar_amd import class_smooth_hip as ch
    nW, NC = 157, CAP
    keys = _perm(CAP, 15)
    rows = [(1, nW, 0, NC), (4, nW, 0, NC)]
    x = torch.randn(2, nW, NC, generator=torch.Generator().manual_seed(int(alpha * 10))) * 6.0 - 9.0
    a32 = torch.tensor(alpha, dtype=torch.float32)
    a, om = float(a32), float(torch.tensor(1.0, dtype=torch.float32) - a32)      # the kernel's own fp32 alpha and fp32 1 - alpha
    ref = torch.empty(2, nW, NC, dtype=torch.float64)
    y = x[:, 0].double()
    ref[:, 0] = y
    for k in range(1, nW):
        y = a * y + om * x[:, k].double()
        ref[:, k] = y
    cells = _Cells({(s, k) for s in (1, 4) for k in keys}, 61, all_stale=True)
    out = _launch(cells, rows, keys, x.reshape(-1), alpha, False, ch.table_uploader(DEV, M)).view(2, nW, NC)
    bound = 2 * (2 * 2.0 ** -24 * float(x.abs().max()) / (1.0 - a))
    err = float((out.cpu().double() - ref).abs().max())
    print("alpha %.1f: max |y - float64| = %.3e, bound %.3e" % (alpha, err, bound))
    assert err <= bound, (err, bound)


# ------------------------------------------------------------------ 2: the pool
IDS = [1, 2, 3, 4, 7, 9]
STRIDE, MAX_PUSH, ALPHA = 1, 6, 0.5


def _gallery(kind, capacity=6, seed=5):
    """a LiveGallery, or a COMBINE LiveTextGallery, holding the classes IDS (one shot each, from random tower features: the tower is not the
    subject) in a store that is full at capacity 6"""
    if kind == "live":
        live = _pair(capacity=capacity)[1]
    else:
        from test_gpu_live_text import _galleries
        live = _galleries("fp32", "combine", capacity=capacity)[1]
    live.add_classes_features(_feats(len(IDS) * T, live.E, seed).view(len(IDS), T, live.E), IDS)
    assert live.class_ids == IDS
    return live


def _feats(n, E, seed):
    return torch.randn(n, E, generator=torch.Generator().manual_seed(seed)).to(DEV)


def _pool(live, **kw):
    from clip_fsar_amd.pool import StreamPool
    return StreamPool(live, max_streams=4, stride=STRIDE, max_push=MAX_PUSH, smooth=ALPHA, **kw)


def _smooth_reference(x, alpha=ALPHA):
    """cfss_smooth_logits over one session's consecutive windows x [n, width], from no state"""
    from clip_fsar_amd import stream_hip as sh
    out = torch.empty(1, *x.shape, device=DEV)
    sh.smooth_logits(x.contiguous()[None], torch.full((1, x.shape[1]), NAN, device=DEV), out, alpha, 0)
    return out[0]


def test_class_mode_equals_column_mode_where_both_apply():
    """no lists, no class changes, uneven pushes, one of them beyond max_push (two rounds, whose windows the device emits round-major)"""
    with torch.no_grad():
        live = _gallery("live")
        col, cls = _pool(live), _pool(live, smooth_by="class")
        hs = [(col.open(), cls.open()) for _ in range(3)]
        windows = 0
        for tick, counts in enumerate([(9, 3, 0), (2, 8, 13), (1, 0, 1), (7, 6, 5), (0, 15, 2)]):
            push = {i: _feats(n, live.E, 100 + 10 * tick + i) for i, n in enumerate(counts) if n}
            a = col.push_features_packed(torch.cat(list(push.values())), [hs[i][0] for i in push], [f.shape[0] for f in push.values()])
            b = cls.push_features_packed(torch.cat(list(push.values())), [hs[i][1] for i in push], [f.shape[0] for f in push.values()])
            assert a.offsets == b.offsets and a.first_window == b.first_window
            assert tuple(b.smoothed.shape) == tuple(b.logits.shape) == (a.offsets[-1], len(IDS))
            assert torch.equal(a.logits, b.logits) and torch.equal(a.smoothed, b.smoothed), tick
            if a.offsets[-1]:
                assert all(torch.equal(u, v) for u, v in zip(col.topk(a, 3, smoothed=True), cls.topk(b, 3, smoothed=True)))
            windows += a.offsets[-1]
        assert windows > 40 and cls._smooth_cells.planes[0].shape == (4, live.capacity) and cls._smooth_cells.planes[1].dtype == torch.int32


def test_sessions_with_class_lists():
    from clip_fsar_amd.pool import GroupedPackedOutput
    lists = [[9, 2], None, [4, 9, 1]]
    with torch.no_grad():
        live = _gallery("live")
        pool = _pool(live, smooth_by="class")
        hs = [pool.open(classes=c) for c in lists]
        raw, smooth = {h: [] for h in hs}, {h: [] for h in hs}
        for tick, counts in enumerate([(9, 10, 3), (2, 0, 8), (13, 1, 1), (1, 7, 6)]):
            push = {h: _feats(n, live.E, 200 + 10 * tick + i) for i, (h, n) in enumerate(zip(hs, counts)) if n}
            po = pool.push_features_packed(torch.cat(list(push.values())), list(push), [f.shape[0] for f in push.values()])
            assert isinstance(po, GroupedPackedOutput) and po.smoothed.shape == po.logits.shape and po.smoothed.dim() == 1
            out = pool._split(po)
            for h in push:
                width = len(IDS) if pool._sessions[h].classes is None else len(pool._sessions[h].classes)
                assert out[h].smoothed.shape == out[h].logits.shape and out[h].logits.shape[1] == width
                raw[h].append(out[h].logits)
                smooth[h].append(out[h].smoothed)
            if po.offsets[-1]:                     # top-k of the grouped output's smoothed scores: of those rows
                values, index = pool.topk(po, 2, smoothed=True)
                rows = [r for h in push for r in out[h].smoothed]
                assert values.shape[0] == len(rows)
                for r, v, i in zip(rows, values, index):
                    sv, si = torch.sort(r, descending=True, stable=True)
                    assert torch.equal(v, sv[:2]) and torch.equal(i.long(), si[:2])
        for h in hs:
            x, y = torch.cat(raw[h]), torch.cat(smooth[h])
            assert x.shape[0] > 8 and torch.equal(y, _smooth_reference(x)), h


class _Pairs:
    """What the (session, class) pairs of a pool saw, push by push: a series per pair and per registration of the class, each the
    pair's raw and smoothed values in window order.  At the end every series must be cfss_smooth_logits of its own raw values: the
    recurrence started where the series starts, and nowhere else."""

    def __init__(self):
        self.series, self.registration = {}, {}

    def registered(self, cid):
        self.registration[cid] = self.registration.get(cid, 0) + 1

    def saw(self, key, class_ids, out):
        for j, cid in enumerate(class_ids):
            raw, smooth = self.series.setdefault((key, cid, self.registration[cid]), ([], []))
            raw.append(out.logits[:, j])
            smooth.append(out.smoothed[:, j])

    def check(self):
        longest = 0
        for key, (raw, smooth) in self.series.items():
            x, y = torch.cat(raw), torch.cat(smooth)
            if not x.shape[0]:
                continue
            ref, _ = _pair_reference(x, None, ALPHA)
            assert torch.equal(y, ref), key
            longest = max(longest, x.shape[0])
        return longest


@pytest.mark.parametrize("kind", ["live", "combine"])
def test_membership_changes_while_sessions_run(kind):
    """enrolment of a new class (the full store grows), a join into a listed session, further shots, "remove 3, add 11" (11 takes 3's
    slot), "remove 7, add 7 again", with no reset() anywhere: every push succeeds and every pair's column is the per-pair reference --
    a series starts at the pair's first window after the class's registration or its joining the list, and runs through everything else"""
    with torch.no_grad():
        live = _gallery(kind)
        E = live.E
        pool = _pool(live, smooth_by="class")
        a, b, c = pool.open(), pool.open(classes=[9, 2]), pool.open(classes=[4, 9, 1])
        pairs, tick = _Pairs(), [0]
        for cid in IDS:
            pairs.registered(cid)

        def push(counts):
            tick[0] += 1
            feats = {h: _feats(n, E, 300 + 10 * tick[0] + i) for i, (h, n) in enumerate(zip((a, b, c), counts)) if n}
            out = pool.push_features(feats)
            for h in feats:
                ids = live.class_ids if pool._sessions[h].classes is None else pool._sessions[h].classes
                assert out[h].smoothed.shape == out[h].logits.shape and out[h].logits.shape[1] == len(ids)
                pairs.saw(h, list(ids), out[h])

        def new_class(cid, seed):
            live.add_classes_features(_feats(T, E, seed).view(1, T, E), [cid])
            pairs.registered(cid)

        push((9, 10, 8))
        assert live.capacity == 6 and pool._smooth_cells.planes[0].shape == (4, 6)
        assert pool.enroll(a, 15) == 1                                   # a new class while streams run: the store grows 6 -> 9
        pairs.registered(15)
        assert live.capacity == 9
        push((2, 8, 3))
        assert [t.shape for t in pool._smooth_cells.planes] == [(4, 9), (4, 9)]
        assert pool.enroll(b, 16, join=True) == 1 and pool._sessions[b].classes == [9, 2, 16]
        pairs.registered(16)
        push((3, 2, 0))
        live.add_shots_features(_feats(T, E, 71).view(1, T, E), [9])      # further shots: the prototype moves, the state stays
        assert pool.enroll(a, 2) == 2 and pool.enroll(b, 16, join=True) == 2
        push((1, 3, 4))
        slot = live.slot_of(3)
        live.remove_classes([3])
        new_class(11, 72)
        assert live.slot_of(11) == slot                                   # nothing of class 3's state may show in 11's first window
        push((7, 1, 2))
        slot, gen = live.slot_of(7), live.slot_generation(live.slot_of(7))
        live.remove_classes([7])
        new_class(7, 73)
        assert live.slot_of(7) == slot and live.slot_generation(slot) == gen + 1
        push((2, 2, 2))
        push((13, 1, 0))                                                  # beyond max_push: three rounds
        assert live.class_ids == [1, 2, 4, 9, 15, 16, 11, 7]
        assert pairs.check() > 25
        # the series that must exist: class 7 twice under session a, class 3 and its slot's next owner, the joined class from its joining
        keys = set(pairs.series)
        assert {(a, 7, 1), (a, 7, 2), (a, 3, 1), (a, 11, 1), (b, 16, 1), (a, 16, 1), (c, 4, 1)} <= keys and (b, 7, 1) not in keys


def test_a_reused_slot_and_a_reset_session_equal_a_fresh_pool():
    with torch.no_grad():
        live = _gallery("live")
        E = live.E
        first, later = [_feats(n, E, 400 + n) for n in (11, 4)], [_feats(n, E, 500 + n) for n in (9, 3, 14)]
        fresh = _pool(live, smooth_by="class")
        f = fresh.open(classes=[4, 9, 1])
        want = [fresh.push_features({f: x})[f] for x in later]
        pool = _pool(live, smooth_by="class")
        old = pool.open()                          # carries state over every class, in slot 0
        for x in first:
            pool.push_features({old: x})
        pool.close(old)
        new = pool.open(classes=[4, 9, 1])
        assert pool._sessions[new].slot == 0
        got = [pool.push_features({new: x})[new] for x in later]
        pool.reset(new)
        again = [pool.push_features({new: x})[new] for x in later]
        for w, g1, g2 in zip(want, got, again):
            assert w.first_window == g1.first_window == g2.first_window and w.logits.shape[0] > 0
            assert torch.equal(w.logits, g1.logits) and torch.equal(w.smoothed, g1.smoothed)
            assert torch.equal(w.logits, g2.logits) and torch.equal(w.smoothed, g2.smoothed)
