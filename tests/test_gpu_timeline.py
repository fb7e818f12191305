"""GPU: the timeline (clip_fsar_amd.pool.StreamPool(timeline=Timeline(...)) on libclipfsar_timeline.so) -- cftl_fold and cftl_read
through their binding, every state plane and every output bit for bit against clip_fsar_amd.timeline.reference_fold / reference_read:
widths at the workgroup edges, every span and ring length of the issue, rows of 0 / 1 / span - 1 / span / span + 1 / span * B + 3 windows
mixed in one table, first windows on and off a bucket boundary, every level, shared and overlapping key lists, keys out of range, stale
marks and marks of generation 0, the same windows cut into several calls, sentinels behind every buffer, inputs unchanged and two runs
for identical bytes; then the pool on test_gpu_events' galleries and features: outputs bit-equal to the pool without the option,
timeline(h) against reference_fold over the pushes' own planes through class lists, enrolment with join, a removal with a new class in
the freed slot, store growth, reset() and a reused slot, other cuts of the same frames, every plane `of` names, and recall against
history.reference_search of the views' planes.  No tolerance anywhere."""
import random

import numpy as np
import pytest
import torch

from test_gpu_events import IDS, _feats, _gallery, _intact, _padded
from test_gpu_history import COUNTS, _Run, _same_outputs
from test_gpu_live import DEV, T

pytestmark = pytest.mark.gpu

INF, NAN = float("inf"), float("nan")
FMAX = float(np.finfo(np.float32).max)
TEN = [-1.0, -0.5, 0.0, -0.0, 0.25, 0.5, 1.0, NAN, -INF, INF]         # the scores of every kernel case
CAP, M = 300, 8                                                         # store slots, session slots
LEVELS = [None, 0.25, FMAX]


def _bits(t):
    return t.contiguous().view(torch.int32)        # NaN-proof, sign-of-zero-proof equality


# ------------------------------------------------------------------ 1: the kernels, through the binding
def _state(B, seed, last_window):
    """(peak, at, above, marks) [M, B, CAP] and gens [CAP] on the host: every cell at random never written (mark 0), stale (another
    generation), or marked with the slot's generation over an `at` of -1 or of any window up to last_window -- this lap's bucket, an
    older lap's or none, as the window falls -- with a candidate's peak and a small count"""
    g = np.random.default_rng(seed)
    gens = g.integers(1, 6, CAP).astype(np.int32)
    kind = g.integers(0, 4, (M, B, CAP))
    marks = np.where(kind == 0, 0, np.where(kind == 1, gens[None, None, :] + g.choice([-1, 1, 7], (M, B, CAP)), gens[None, None, :])).astype(np.int32)
    at = g.integers(-1, last_window + 1, (M, B, CAP)).astype(np.int32)
    peak = g.choice(np.array([-1.0, -0.5, 0.0, -0.0, 0.25, 0.5, 1.0, INF], np.float32), (M, B, CAP))
    above = g.integers(0, 6, (M, B, CAP)).astype(np.int32)
    return (peak, at, above, marks), gens


def _table(rows):
    """(slot, nW, key0, NC) per row -> the 6-column table"""
    table, n_out, chunks = [], 0, 0
    for slot, nW, key0, NC in rows:
        table.append([slot, nW, n_out, NC, key0, chunks])
        n_out += nW * NC
        chunks += -(-NC // 256)
    return table, n_out


def _keys(NC, seed):
    """NC + 43 distinct store slots, so that lists of NC at offsets 0 .. 43 overlap; three of them out of range where the width allows"""
    keys = torch.randperm(CAP, generator=torch.Generator().manual_seed(seed))[:NC + 43].tolist()
    if NC >= 3:
        keys[1], keys[NC // 2], keys[NC - 1] = -1, CAP, 1 << 30
    return keys


class _Device:
    """the state and gens on the device, between sentinels"""

    def __init__(self, state, gens):
        self.bufs = [_padded(torch.from_numpy(p.copy())) for p in state] + [_padded(torch.from_numpy(gens.copy()))]
        self.gens0 = gens

    @property
    def planes(self):
        return [v for _, v in self.bufs[:4]]

    def fold(self, rows, keys, scores, first, span, level, uploader, firsts):
        from clip_fsar_amd import timeline_hip as th
        table, n_out = _table(rows)
        assert n_out == scores.numel()
        kbuf, kd = _padded(torch.tensor(keys, dtype=torch.int32))
        xbuf, xd = _padded(scores)
        f = firsts.upload([[w] for w in first])
        th.fold(xd, *self.planes, self.bufs[4][1], kd, uploader.upload(table), th.Table(f.host.view(-1), f.dev.view(-1), f.S), span, level)
        torch.cuda.synchronize()
        assert _intact(kbuf) and _intact(xbuf) and all(_intact(b) for b, _ in self.bufs)
        assert torch.equal(kd.cpu(), torch.tensor(keys, dtype=torch.int32)) and torch.equal(_bits(xd.cpu()), _bits(scores))
        assert torch.equal(self.bufs[4][1].cpu(), torch.from_numpy(self.gens0))

    def read(self, rows, keys, n_out, span, uploader):
        from clip_fsar_amd import timeline_hip as th
        kbuf, kd = _padded(torch.tensor(keys, dtype=torch.int32))
        outs = [_padded(torch.full((n_out,), s, dtype=d)) for s, d in ((-7.0, torch.float32), (-9, torch.int32), (-9, torch.int32))]
        before = [_bits(p.cpu()).clone() for p in self.planes]
        th.read(*self.planes, self.bufs[4][1], kd, *(v for _, v in outs), uploader.upload(rows), span)
        torch.cuda.synchronize()
        assert _intact(kbuf) and all(_intact(b) for b, _ in outs) and all(_intact(b) for b, _ in self.bufs)
        assert all(torch.equal(_bits(p.cpu()), b) for p, b in zip(self.planes, before))            # the state is only read
        return [v.cpu() for _, v in outs]

    def equals(self, state):
        return all(torch.equal(_bits(p.cpu()), _bits(torch.from_numpy(q))) for p, q in zip(self.planes, state))


def _uploaders():
    from clip_fsar_amd import class_smooth_hip as ch
    from clip_fsar_amd import timeline_hip as th
    from clip_fsar_amd.pool_hip import TableUploader
    return ch.table_uploader(DEV, M), TableUploader(DEV, M, cols=1), th.read_uploader(DEV, 16)


def _fold_case(NC, span, B):
    """One table with every row length of the issue, first windows on and off a bucket boundary, a shared list and overlapping ones, a
    random state and ten-valued scores -- the first seed whose REFERENCE shows what the case is for (the inputs are chosen on the model,
    the kernels are not asked): overwritten laps and restarted stale cells, and with span > 1 ties kept and peaks replaced ->
    (rows, counts, first, keys, scores, level, state, gens, the state afterwards, the reference's counts)"""
    from clip_fsar_amd.timeline import reference_fold
    level = LEVELS[(NC + span + B) % 3]
    counts = [0, 1, span - 1, span, span + 1, span * B + 3]
    first = [span * 2, 0, span * B + 1, span - 1, 2 * span + max(0, span - 2), 0]
    key0 = [0, 0, 17, 43, 17, 5]
    rows = [(slot, nW, k0, NC) for slot, nW, k0 in zip((3, 0, 5, 1, 4, 7), counts, key0)]
    table, n = _table(rows)
    need = ("laps", "restarted") + (("ties", "replaced") if span > 1 else ())
    for seed in range(1000 * NC + 10 * span + B, 1000 * NC + 10 * span + B + 400 * 1000, 1000):
        keys = _keys(NC, seed)
        scores = torch.tensor(TEN)[torch.randint(0, 10, (n,), generator=torch.Generator().manual_seed(seed))]
        state, gens = _state(B, seed, max(f + c for f, c in zip(first, counts)))
        want = [p.copy() for p in state]
        shown = reference_fold(want, gens, table, keys, scores.numpy(), first, span, B, level)
        if all(shown[k] > 0 for k in need):
            break
    assert all(shown[k] > 0 for k in need), shown                          # no case is vacuous
    return rows, counts, first, keys, scores, level, state, gens, want, shown, seed


@pytest.mark.parametrize("B", [1, 2, 5])
@pytest.mark.parametrize("span", [1, 2, 3, 7])
@pytest.mark.parametrize("NC", [1, 255, 256, 257])
def test_fold_and_read_equal_the_reference(NC, span, B):
    from clip_fsar_amd.timeline import read_rows, reference_read
    rows, counts, first, keys, scores, level, state, gens, want, shown, seed = _fold_case(NC, span, B)
    untouched = [np.array_equal(a[6].view(np.int32), b[6].view(np.int32)) for a, b in zip(state, want)]     # slot 6 is in no row
    assert all(untouched) and not np.array_equal(state[3], want[3])
    # ---- one call, twice from the same bytes
    table_up, first_up, read_up = _uploaders()
    runs = []
    for _ in range(2):
        dev = _Device(state, gens)
        dev.fold(rows, keys, scores, first, span, level, table_up, first_up)
        assert dev.equals(want)
        runs.append([_bits(p.cpu()) for p in dev.planes])
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    # ---- the same windows cut into three calls leave the bytes of one
    cut = _Device(state, gens)
    rng = random.Random(seed)
    cuts = [sorted(rng.randint(0, nW) for _ in range(2)) for nW in counts]
    blocks, at = [], 0
    for (_, nW, _, _) in rows:
        blocks.append(scores[at:at + nW * NC].view(nW, NC))
        at += nW * NC
    for i in range(3):
        span_of = [([0] + c + [nW])[i:i + 2] for c, nW in zip(cuts, counts)]
        part = [(slot, hi - lo, k0, NC) for (slot, _, k0, _), (lo, hi) in zip(rows, span_of)]
        piece = torch.cat([b[lo:hi].reshape(-1) for b, (lo, hi) in zip(blocks, span_of)])
        cut.fold(part, keys, piece, [f + lo for f, (lo, _) in zip(first, span_of)], span, level, table_up, first_up)
    assert cut.equals(want)
    # ---- the read: NB 0 / 1 / B, a B0 whose buckets have wrapped, a slot in two rows, out-of-range keys
    newest = lambda r: (first[r] + counts[r] - 1) // span
    rrows, n_out = read_rows([7, 7, 3, 0, 5, 6], [range(max(0, newest(5) - B + 1), newest(5) + 1), range(newest(5), newest(5) + 1), range(0),
                                                    range(0, min(B, 1)), range(newest(2) - B + 1, newest(2) + 1), range(3, 3 + B)],
                             [NC] * 6, [5, 0, 0, 0, 17, 43])
    assert rrows[0][2] == B and rrows[0][1] >= 1 and rrows[1][:3] == [7, newest(5), 1] and rrows[2][2] == 0        # the ring has wrapped
    got = dev.read(rrows, keys, n_out, span, read_up)
    ref = reference_read(want, gens, rrows, keys, span, B)
    assert all(torch.equal(_bits(a), _bits(torch.from_numpy(b))) for a, b in zip(got, ref))
    dead = dict(marks=0, negative=0, lap=0, live=0, nan=0)
    for slot, b0, nb, nc, k0, _, _ in rrows:
        for b in range(b0, b0 + nb):
            for key in keys[k0:k0 + nc]:
                if not 0 <= key < CAP:
                    dead["nan"] += 1
                    continue
                m, a = want[3][slot, b % B, key], want[1][slot, b % B, key]
                kind = "marks" if m != gens[key] else "negative" if a < 0 else "lap" if a // span != b else "live"
                dead[kind] += 1
    assert dead["live"] > 0 and dead["marks"] > 0
    if NC > 1:                                      # dead cells of each of the three kinds, and keys out of range
        assert all(dead[k] > 0 for k in ("marks", "negative", "lap", "nan")), dead


def test_the_binding_refuses_what_the_library_refuses():
    from clip_fsar_amd import timeline_hip as th
    table_up, first_up, read_up = _uploaders()
    state, gens = _state(2, 1, 9)
    dev = _Device(state, gens)
    keys = torch.arange(4, dtype=torch.int32, device=DEV)
    x = torch.zeros(8, device=DEV)
    first = lambda *ws: (lambda f: th.Table(f.host.view(-1), f.dev.view(-1), f.S))(first_up.upload([[w] for w in ws]))
    good = [[1, 2, 0, 4, 0, 0]]
    for rows, ws, span, level, words in ((good, (-1,), 3, None, "negative first window"), (good, ((1 << 31) - 2,), 3, None, "below 2\\^31"),
                                         (good, (0,), 0, None, "span=0"), (good, (0,), (1 << 20) + 1, None, "span="),
                                         (good, (0,), 3, INF, "level=inf must be finite"), (good, (0,), 3, NAN, "level=nan must be finite"),
                                         ([[1, 2, 0, 4, 1, 0]], (0,), 3, None, "keys\\["), ([[9, 2, 0, 4, 0, 0]], (0,), 3, None, "slot 9 outside"),
                                         ([[1, 1, 0, 4, 0, 0]], (0,), 3, None, "not to NOUT=8")):
        with pytest.raises(RuntimeError, match="cftl_fold failed: cftl_fold: .*" + words):
            th.fold(x, *dev.planes, dev.bufs[4][1], keys, table_up.upload(rows), first(*ws), span, level)
    outs = [torch.zeros(8, device=DEV), torch.zeros(8, device=DEV, dtype=torch.int32), torch.zeros(8, device=DEV, dtype=torch.int32)]
    for rows, words in (([[1, 0, 3, 4, 0, 0, 0]], "NB=3 buckets outside 0 .. B=2"), ([[1, -1, 2, 4, 0, 0, 0]], "negative first bucket"),
                        ([[1, 0, 1, 4, 0, 0, 0]], "not to NOUT=8"), ([[1, 0, 2, 4, 0, 1, 0]], "prefix sums"),
                        ([[8, 0, 2, 4, 0, 0, 0]], "slot 8 outside")):
        with pytest.raises(RuntimeError, match="cftl_read failed: cftl_read: .*" + words):
            th.read(*dev.planes, dev.bufs[4][1], keys, *outs, read_up.upload(rows), 3)
    with pytest.raises(RuntimeError, match="dtype"):
        th.read(*dev.planes, dev.bufs[4][1], keys.float(), *outs, read_up.upload([[1, 0, 2, 4, 0, 0, 0]]), 3)
    assert dev.equals(state)                        # nothing was launched


# ------------------------------------------------------------------ 2: the pool
STRIDE, MAX_PUSH, SPAN, RING = 2, 5, 3, 2         # test_gpu_history's pool; buckets of 3 windows in a ring of 2: laps turn over


def _timeline(**kw):
    from clip_fsar_amd.timeline import Timeline
    return Timeline(**dict(dict(span=SPAN, buckets=RING, level=None), **kw))


def _pool(live, timeline=None, **kw):
    from clip_fsar_amd.pool import StreamPool
    if timeline is not None:
        kw["timeline"] = timeline
    return StreamPool(live, max_streams=4, stride=STRIDE, max_push=MAX_PUSH, **kw)


def _plane(pool, out, of=None):
    """the plane of a session's output the pool's timeline folds"""
    of = pool._timeline.of if of is None else of
    if of is None:
        judged = getattr(out, "deviation", None)
        return judged if judged is not None else (out.logits if out.smoothed is None or not pool._by_class else out.smoothed)
    return getattr(out, of)


class _Pairs:
    """The reference over what a pool returned: a state of one cell row per (session, class id), restarted where the contract restarts a
    pair -- the session's open() / reset(), the class's registration -- and folded by reference_fold over the pair's column of every
    StreamOutput in push order"""

    def __init__(self, tl):
        self.tl, self.cells, self.shown = tl, {}, dict(ties=0, replaced=0, laps=0, restarted=0)

    def forget(self, session=None, cid=None):
        for key in [k for k in self.cells if (session is None or k[0] == session) and (cid is None or k[1] == cid)]:
            del self.cells[key]

    def saw(self, pool, outs, ids_of):
        from clip_fsar_amd.timeline import new_state, reference_fold
        one = np.ones(1, np.int32)
        for h, out in outs.items():
            plane = _plane(pool, out).cpu().numpy()
            for j, cid in enumerate(ids_of[h]):
                st = self.cells.setdefault((h, cid), new_state(1, self.tl.buckets, 1))
                got = reference_fold(st, one, [[0, plane.shape[0], 0, 1, 0, 0]], [0], plane[:, j].copy(), [out.first_window], self.tl.span,
                                     self.tl.buckets, self.tl.level)
                for k, v in got.items():
                    self.shown[k] += v

    def view(self, h, ids, buckets):
        """(peak, at, above) [len(buckets), len(ids)] as timeline(h) must return them"""
        from clip_fsar_amd.timeline import new_state, reference_read
        one = np.ones(1, np.int32)
        cols = [reference_read(self.cells.get((h, c), new_state(1, self.tl.buckets, 1)), one, [[0, buckets.start, len(buckets), 1, 0, 0, 0]],
                               [0], self.tl.span, self.tl.buckets) for c in ids]
        return [torch.from_numpy(np.stack([c[i] for c in cols], 1)) for i in range(3)]


def _check_view(pool, pairs, h, ids, classes=None, last=None):
    from clip_fsar_amd.timeline import held_buckets
    v = pool.timeline(h, classes=classes, last=last)
    held = held_buckets(pool.stats(h)["windows"], pool._timeline.span, pool._timeline.buckets, last)
    assert (v.first_bucket, v.span, v.class_ids) == (held.start, pool._timeline.span, tuple(ids)), (h, v[:3])
    want = pairs.view(h, ids, held)
    assert v.peak.is_cuda and (v.peak.dtype, v.at.dtype, v.above.dtype) == (torch.float32, torch.int32, torch.int32)
    for got, ref, name in zip((v.peak, v.at, v.above), want, ("peak", "at", "above")):
        assert tuple(got.shape) == (len(held), len(ids)) and torch.equal(_bits(got.cpu()), _bits(ref)), (h, name)
    return v


CONFIGS = {"plain": {}, "by_class": dict(smooth=0.5, smooth_by="class"), "rates": dict(rates=(1, 2))}


def _config(name):
    from clip_fsar_amd.baseline import Baseline
    from clip_fsar_amd.contest import Contest
    from clip_fsar_amd.events import EventRule
    if name == "baseline":
        return dict(baseline=Baseline(rate=1 / 8, warm_rate=0.5, warmup=2, gate=3.0))
    if name == "contest":
        return dict(smooth=0.5, smooth_by="class", events=EventRule(0.55, 0.45, 2, 2), contest=Contest(top=1))
    return CONFIGS.get(name, {})


@pytest.mark.parametrize("config", ["plain", "by_class", "combine", "baseline", "contest", "rates"])
def test_the_option_changes_no_output_bit_and_the_views_are_the_reference(config):
    """the pool shapes of the issue over test_gpu_history's uneven pushes (three rounds in one of them): the outputs are the bits of the
    pool without the option, and every session's view is reference_fold over the planes those pushes returned"""
    kw = _config(config)
    tl = _timeline(level=None if config == "baseline" else 0.5 if config == "combine" else 20.0)
    with torch.no_grad():
        live = _gallery("combine" if config == "combine" else "live")
        plain, mine = _Run(_pool(live, **kw)), _Run(_pool(live, tl, **kw))
    _same_outputs(plain.outs, mine.outs)
    assert plain.pool.stats() == mine.pool.stats() and not hasattr(plain.pool, "_tl_cells") and plain.pool._timeline is None
    if config == "contest":
        assert plain.pool.take_events() == mine.pool.take_events()
    p = mine.pool
    if config == "baseline":
        assert type(mine.outs[0][mine.hs[0]]).__name__ == "DeviationStreamOutput"      # the judged plane is the deviation
    pairs = _Pairs(tl)
    for out in mine.outs:
        pairs.saw(p, out, {h: IDS for h in out})
    assert pairs.shown["replaced"] > 0 and pairs.shown["laps"] > 0, pairs.shown     # (ties are the kernel cases': real scores seldom tie)
    with torch.no_grad():
        for h in mine.hs:
            v = _check_view(p, pairs, h, IDS)
            assert v.peak.shape[0] == RING and v.first_bucket > 0                       # the ring has turned over
            _check_view(p, pairs, h, [9, 1], classes=[9, 1])
            _check_view(p, pairs, h, IDS, last=1)
    assert tuple(p._tl_cells.planes[0].shape) == (4, RING, live.capacity)


def test_a_gated_pixel_push_returns_the_same_bits():
    """still= on pixel pushes (the fixture has a tower)"""
    import clip_fsar_amd.synth as synth
    from clip_fsar_amd.still import StillGate
    from test_gpu_live import ARCH
    res = synth.ARCHS[ARCH]["res"]
    base = (torch.randn(9, 3, res, res, generator=torch.Generator().manual_seed(3)) * 0.5).to(DEV)
    tl = _timeline()
    with torch.no_grad():
        live = _gallery("live")
        pools = [_pool(live, still=StillGate()), _pool(live, tl, still=StillGate())]
        hs = [(p.open(), p.open()) for p in pools]
        outs = [[], []]
        for pick_a, pick_b in (([0, 0, 1, 1, 1, 2, 2], [3, 4]), ([2, 2, 5, 5, 5, 5, 6, 6, 6, 6, 7, 8], [4, 4, 4, 3, 3, 3, 3, 1, 1])):
            for i, p in enumerate(pools):
                outs[i].append(p.push({hs[i][0]: base[pick_a], hs[i][1]: base[pick_b]}))
        _same_outputs(*outs)
        assert pools[0].stats() == pools[1].stats() and pools[1].stats()["still_frames"] > 8
        pairs = _Pairs(tl)
        for out in outs[1]:
            pairs.saw(pools[1], out, {h: IDS for h in out})
        for h in hs[1]:
            _check_view(pools[1], pairs, h, IDS)


def test_state_changes_under_running_sessions():
    """test_gpu_events' schedule: class lists, enroll(join=True), "remove 3, add 11" into the freed slot, a store growth, reset() and a
    reused session slot, over per-class smoothing; the model restarts a pair where the contract does, and every push is followed by the
    views of its sessions"""
    tl = _timeline(level=20.0)
    pairs = _Pairs(tl)
    with torch.no_grad():
        live = _gallery("live")
        pool = _pool(live, tl, smooth=0.5, smooth_by="class")
        E = live.E
        a, b, c = pool.open(), pool.open(classes=[9, 2]), pool.open(classes=[4, 9, 1])
        hs = {"a": a, "b": b, "c": c}
        tick = [0]

        def ids_of(h):
            return list(live.class_ids if pool._sessions[h].classes is None else pool._sessions[h].classes)

        def push(counts):
            tick[0] += 1
            feats = {hs[n]: _feats(k, E, 300 + 10 * tick[0] + i) for i, (n, k) in enumerate(zip("abc", counts)) if k}
            out = pool.push_features(feats)
            pairs.saw(pool, out, {h: ids_of(h) for h in feats})
            for h in pool.sessions:                 # the sessions that did not push as well
                _check_view(pool, pairs, h, ids_of(h))

        push((9, 10, 8))
        assert live.capacity == 6 and tuple(pool._tl_cells.planes[3].shape) == (4, RING, 6)
        assert pool.enroll(a, 15) == 1                                    # a new class while streams run: the store grows 6 -> 9
        pairs.forget(cid=15)
        push((2, 8, 3))
        assert live.capacity == 9 and tuple(pool._tl_cells.planes[3].shape) == (4, RING, 9)
        assert pool.enroll(b, 16, join=True) == 1 and pool._sessions[b].classes == [9, 2, 16]
        pairs.forget(cid=16)
        push((3, 2, 0))
        live.add_shots_features(_feats(T, E, 71).view(1, T, E), [9])      # further shots: the prototype moves, the cells stay
        push((1, 3, 4))
        slot = live.slot_of(3)
        before = _check_view(pool, pairs, a, ids_of(a))
        assert bool((before.at[:, ids_of(a).index(3)] >= 0).any())
        live.remove_classes([3])
        live.add_classes_features(_feats(T, E, 72).view(1, T, E), [11])
        pairs.forget(cid=11)
        assert live.slot_of(11) == slot                                   # 11, in 3's slot, starts empty: 3's cells are stale
        v = _check_view(pool, pairs, a, ids_of(a))
        assert bool((v.at[:, ids_of(a).index(11)] == -1).all())
        push((7, 1, 2))
        pool.reset(b)
        pairs.forget(session=b)
        assert tuple(pool.timeline(b).peak.shape) == (0, 3)               # no window yet: empty planes
        push((2, 9, 2))
        push((13, 1, 0))                                                  # beyond max_push: three rounds, one fold
        pool.close(c)
        d = pool.open(classes=[7, 11, 4])                                 # into c's slot
        assert pool._sessions[d].slot == 2
        hs["c"] = d
        push((3, 0, 12))
        push((6, 5, 4))
        assert live.class_ids == [1, 2, 4, 7, 9, 15, 16, 11]
        assert pairs.shown["replaced"] > 0 and pairs.shown["laps"] > 0
        for h, bad in ((d, [1]), (b, [9, 4])):
            with pytest.raises(ValueError, match=r"StreamPool.timeline: class %d is not registered \(classes= of session %d\)" % (bad[-1], h)):
                pool.timeline(h, classes=bad)
        with pytest.raises(ValueError, match="StreamPool.timeline: class 3 is not registered"):
            pool.timeline(a, classes=[3])


def test_the_cut_of_the_pushes_does_not_matter():
    """the same frames in other pushes: the state planes are the same bytes"""
    tl = _timeline(level=20.0)
    with torch.no_grad():
        live = _gallery("live")
        whole = _Run(_pool(live, tl))
        feats = whole.rows
        other = _pool(live, tl)
        hs = [other.open() for _ in whole.hs]
        done = [0] * 3
        for counts in ((1, 30, 2), (20, 0, 0), (3, 5, 35), (100, 100, 100)):
            part = {}
            for i, (h, k) in enumerate(zip(hs, counts)):
                rows = feats[whole.hs[i]][done[i]:done[i] + k]
                if rows.shape[0]:
                    part[h] = rows
                    done[i] += rows.shape[0]
            other.push_features(part)
        assert [other.stats(h)["frames"] for h in hs] == [whole.pool.stats(h)["frames"] for h in whole.hs]
        for h, g in zip(whole.hs, hs):
            x, y = whole.pool.timeline(h), other.timeline(g)
            assert x[:3] == y[:3] and all(torch.equal(_bits(p), _bits(q)) for p, q in zip(x[3:], y[3:]))
    marked = whole.pool._tl_cells.planes[3] != 0
    assert torch.equal(whole.pool._tl_cells.planes[3], other._tl_cells.planes[3]) and bool(marked.any())
    for p, q in zip(whole.pool._tl_cells.planes, other._tl_cells.planes):
        assert torch.equal(_bits(p)[marked], _bits(q)[marked])             # (cells never written are uninitialised memory)


@pytest.mark.parametrize("of", ["logits", "smoothed", "deviation", None])
def test_of_names_the_plane(of):
    from clip_fsar_amd.baseline import Baseline
    tl = _timeline(of=of, level=0.0)
    with torch.no_grad():
        live = _gallery("live")
        r = _Run(_pool(live, tl, smooth=0.5, smooth_by="class", baseline=Baseline(rate=1 / 8, warm_rate=0.5, warmup=2)), COUNTS[:5])
        pairs = _Pairs(tl)
        for out in r.outs:
            pairs.saw(r.pool, out, {h: IDS for h in out})
        views = [_check_view(r.pool, pairs, h, IDS) for h in r.hs]
    out = r.outs[0][r.hs[0]]
    assert _plane(r.pool, out) is (out.deviation if of is None else getattr(out, of))
    later = r.outs[1][r.hs[1]]                      # the three planes differ: a recurrence under way, a warm-up that yields NaN
    assert not torch.equal(_bits(later.logits), _bits(later.smoothed)) and bool(torch.isnan(out.deviation).any())
    assert any(bool((v.at >= 0).any()) for v in views)


def _check_recall(pool, res, ids, handles, sep, floor, top, last=None):
    """a recall's hits and peaks are history.reference_search over the plane of the views' bucket peaks"""
    from clip_fsar_amd.history import Hit, reference_search
    views = [pool.timeline(h, classes=ids, last=last) for h in handles]
    plane = torch.cat([v.peak for v in views]).cpu()
    at, above = torch.cat([v.at for v in views]).cpu(), torch.cat([v.above for v in views]).cpu()
    counts = [v.peak.shape[0] for v in views]
    offsets = [sum(counts[:i]) for i in range(len(counts))]
    want_rows, want_peaks = reference_search(plane, counts, sep, floor, top)
    owner = [i for i, n in enumerate(counts) for _ in range(n)]
    assert res.buckets == sum(counts)
    for k, c in enumerate(ids):
        order = sorted(want_rows[k], key=lambda row: (-float(plane[row, k]), row))
        want = [Hit(handles[owner[row]], c, int(at[row, k]), float(plane[row, k]), None) for row in order]
        assert res.hits[c] == want and res.peaks[c] == want_peaks[k], c
        assert [np.float32(h.score).view(np.uint32) for h in res.hits[c]] == [plane[row, k].view(torch.int32).item() & 0xFFFFFFFF for row in order]
        assert [(h.bucket, h.above) for h in res.hits[c]] == [(views[owner[row]].first_bucket + row - offsets[owner[row]], int(above[row, k]))
                                                              for row in order]
        assert all(h.window // pool._timeline.span == h.bucket for h in res.hits[c])
    return want_peaks


def test_recall_is_the_reference_search_over_the_bucket_peaks():
    from clip_fsar_amd.align import Aligner
    from clip_fsar_amd.history import History
    ids = [7, 2, 9]
    tl = _timeline(span=2, buckets=8, level=20.0)
    with torch.no_grad():
        live = _gallery("live")
        r = _Run(_pool(live, tl, history=History(frames=64)))
        p = r.pool
        for kw, sep, floor, top in ((dict(), 1, None, 16), (dict(top=2), 1, None, 2), (dict(separation=0, top=4096), 0, None, 4096),
                                    (dict(separation=3, top=3), 3, None, 3), (dict(separation=10 ** 6), 10 ** 6, None, 16)):
            res = p.recall(ids, **kw)
            peaks = _check_recall(p, res, ids, p.sessions, sep, floor, top)
            assert all(len(res.hits[c]) == min(top, n) for c, n in zip(ids, peaks)) and 16 < res.buckets <= 3 * 8
        median = float(torch.cat([p.timeline(h, classes=ids).peak for h in p.sessions]).median())
        res = p.recall(ids, min_score=median, separation=0, top=4096)
        _check_recall(p, res, ids, p.sessions, 0, median, 4096)
        assert 0 < sum(res.peaks.values()) < 3 * res.buckets                   # about half the plane
        res = p.recall([9], sessions=[r.hs[2], r.hs[0]], last=3, separation=0)
        _check_recall(p, res, [9], [r.hs[2], r.hs[0]], 0, None, 16, last=3)
        assert res.buckets == 6 and len(res.hits[9]) == 6
        # the hits' windows are the pool's own: through explain while the ring holds them, through hit_features on the history
        every = p.recall(ids, separation=0, top=4096)                           # every held bucket of every session is a hit
        hits = [h for c in ids for h in every.hits[c]]
        assert len(hits) == 3 * every.buckets and any(h.window in p.enrolable(h.session) for h in hits) and any(h.window not in p.enrolable(h.session) for h in hits)
        for h in hits:
            assert h.window in p.searchable(h.session) and torch.equal(p.hit_features(h), r.window(h.session, h.window))
            assert torch.equal(_bits(r.logits[h.session][h.window][IDS.index(h.class_id)]), _bits(torch.tensor(h.score, device=DEV)))
        h = next(h for h in hits if h.window in p.enrolable(h.session))
        want = Aligner(live).align_features(r.window(h.session, h.window).unsqueeze(0), [h.class_id])
        for got in (p.explain(h.session, [h.class_id], window=h.window), p.explain_hit(h)):
            assert all(torch.equal(getattr(got, n), getattr(want, n)) for n in ("plan", "dists", "logits"))


def test_the_order_of_the_sessions_decides_a_tie():
    """two sessions fed the same frames hold the same bucket peaks: with top = 1 the hit is the session recalled first"""
    tl = _timeline(span=2, buckets=8)
    with torch.no_grad():
        live = _gallery("live")
        p = _pool(live, tl)
        a, b = p.open(), p.open()
        f = _feats(14, live.E, 9)
        p.push_features({a: f[:9], b: f[:4]})
        p.push_features({b: f[4:], a: f[9:]})
        fwd, back = p.recall([4], top=1), p.recall([4], sessions=[b, a], top=1)
        _check_recall(p, fwd, [4], [a, b], 1, None, 1)
        _check_recall(p, back, [4], [b, a], 1, None, 1)
    (x,), (y,) = fwd.hits[4], back.hits[4]
    assert (x.session, y.session) == (a, b) and x[1:] == y[1:] and (x.bucket, x.above) == (y.bucket, y.above) and fwd.peaks == back.peaks


def test_refusals_on_the_device():
    from clip_fsar_amd.pool import StreamPool
    from clip_fsar_amd.shortlist import Shortlist
    from test_gpu_live import _pair
    tl = _timeline()
    with torch.no_grad():
        _, live, static = _pair(capacity=6)
        with pytest.raises(ValueError, match="timeline=.*slot store"):
            StreamPool(static, timeline=tl)
        live = _gallery("live")
        with pytest.raises(ValueError, match="timeline= together with shortlist="):
            StreamPool(live, shortlist=Shortlist(live, keep=3), timeline=tl)
        with pytest.raises(ValueError, match="timeline.of = 'deviation' names a plane this pool does not make"):
            StreamPool(live, timeline=tl._replace(of="deviation"))
        with pytest.raises(TypeError, match="timeline must be a Timeline"):
            StreamPool(live, timeline=(3, 2))
        r = _Run(_pool(live, tl), COUNTS[:2])
        p = r.pool
        state = [q.clone() for q in p._tl_cells.planes]
        for call, words in ((lambda: p.timeline(99), "session 99 is not open"), (lambda: p.timeline(r.hs[0], classes=[1, 1]), "appears twice"),
                            (lambda: p.timeline(r.hs[0], classes=[12]), "class 12 is not registered"), (lambda: p.timeline(r.hs[0], last=0), "last must be"),
                            (lambda: p.recall([]), "at least one class"), (lambda: p.recall([1], top=0), "top must be"),
                            (lambda: p.recall([1], separation=-1), "separation must be"), (lambda: p.recall([1], min_score=NAN), "min_score must be"),
                            (lambda: p.recall([1], sessions=[r.hs[0], r.hs[0]]), "appears twice"), (lambda: p.recall([1], last=0), "last must be")):
            with pytest.raises(ValueError, match=words):
                call()
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(state, p._tl_cells.planes)) and "timeline" not in " ".join(p.stats())
