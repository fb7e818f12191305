"""GPU: event evidence (clip_fsar_amd.pool.StreamPool(events=..., evidence=Evidence(...)) on libclipfsar_evidence.so) -- the two kernels
through their binding against clip_fsar_amd.evidence.reference_capture bit for bit on hand-built records (no scoring): where, head and
store between sentinels, the inputs unchanged, twice from the same head for identical bytes, at the placement pass's chunk edges, every
row width and piece size, a misaligned ring, every kinds mask, KEEP0 = NW, malformed records, tempo values out of range, and several
calls in sequence so that the head wraps; then the pool on a small LiveGallery fed from tower features: the evidence rows against the
test's own frame history after the rings wrapped and the sessions were closed and reset, the store's capacity, pushes of several rounds,
enrolment and explanation long after the fact, bit-equality with the pool without the option, tempo, shortlist and class lists, and the
single device-to-host copy of take_events()."""
import random

import pytest
import torch

from test_gpu_events import IDS, _feats, _gallery
from test_gpu_live import DEV, T

pytestmark = pytest.mark.gpu

F_SENTINEL, I_SENTINEL = -12345.0, -77
ONSET, OFFSET = 1, 2


# ------------------------------------------------------------------ 1: the kernels, through the binding
def _padded(t, pad=64):
    """t inside a larger buffer with `pad` sentinels on either side -> (buffer, the view holding t).  pad = 64: the view is 16-byte
    aligned as the buffer is; pad = 65: one float off"""
    sentinel = I_SENTINEL if t.dtype == torch.int32 else F_SENTINEL
    buf = torch.full((t.numel() + 2 * pad,), sentinel, dtype=t.dtype, device=DEV)
    view = buf[pad:pad + t.numel()].view(t.shape)
    view.copy_(t)
    return buf, view


def _intact(buf, pad=64):
    sentinel = I_SENTINEL if buf.dtype == torch.int32 else F_SENTINEL
    return bool((buf[:pad] == sentinel).all()) and bool((buf[-pad:] == sentinel).all())


def _bits(t):
    return t.contiguous().view(torch.int32)


def _world(seed, T_, E, cap, M, capacity, R, stride=2, ms=3, S=3, keep_all=False):
    """a ring, a table, M records and a tempo plane, at random: valid records of both kinds over every row, records of windows that
    left the ring, a row with KEEP0 = NW, and malformed ones"""
    rng = random.Random(seed)
    rates = [None, (2,), None, (1, 2, 3)][R]
    rate = 1 if rates is None else rates[-1]
    room = (cap - 1 - (T_ - 1) * rate) // stride           # NW - 1 - KEEP0 at most: the kept windows lie in the ring together
    assert room >= 0
    table, out0 = [], 0
    for s in range(S):
        keep = 0 if keep_all else rng.choice([0, 0, 1, 3])
        kept = 0 if s == 1 and not keep_all else 1 + rng.randint(0, min(room, 4))      # row 1: KEEP0 = NW, nothing to capture
        nc = rng.randint(1, 5)
        table.append([rng.randrange(ms), rng.randrange(cap), keep + kept, keep, out0, nc])
        out0 += (keep + kept) * nc
    events = []
    for _ in range(M):
        row = rng.randrange(S)
        nw, nc = table[row][2], table[row][5]
        rec = [row, rng.randrange(nc), rng.randrange(nw) if nw else 0, rng.choice([ONSET, ONSET, OFFSET]), rng.randint(1, 9)]
        if rng.random() < 0.15:                            # malformed: the row, the window, the column or the kind
            at = rng.randrange(4)
            rec[(0, 2, 1, 3)[at]] = rng.choice([(-1, S, 1 << 20), (-1, nw, 1 << 30), (-1, nc, 1 << 30), (0, 3, -2)][at])
        events.append(rec)
    events[0] = [0, 0, table[0][3], ONSET, 1]                  # the first record is a good onset: every shape captures something
    g = torch.Generator().manual_seed(seed)
    ring = torch.randn(ms, cap, E, generator=g)
    tempo = None if rates is None else torch.randint(-1, len(rates) + 1, (max(1, out0),), generator=g, dtype=torch.int32)
    return ring, table, torch.tensor(events, dtype=torch.int32), tempo, rates, rate, stride


#          T  E    cap  M    capacity R  ring pad
SHAPES = [(1, 4, 11, 1, 1, 0, 64),
          (4, 64, 11, 7, 3, 0, 64),
          (8, 66, 71, 255, 64, 3, 64),
          (4, 512, 71, 256, 3, 1, 64),
          (8, 64, 71, 257, 64, 0, 65),                     # the ring one float off 16 bytes: 4-byte pieces at E % 4 == 0
          (4, 66, 11, 600, 64, 3, 64),
          (1, 512, 71, 600, 1, 0, 64),
          (8, 4, 71, 7, 3, 3, 65)]


@pytest.mark.parametrize("T_,E,cap,M,capacity,R,pad", SHAPES)
def test_capture_against_the_reference(T_, E, cap, M, capacity, R, pad):
    from clip_fsar_amd import evidence_hip as eh
    from clip_fsar_amd.evidence import reference_capture
    ring, table, events, tempo, rates, rate, stride = _world(1000 + M + E, T_, E, cap, M, capacity, R)
    uploader = eh.table_uploader(DEV, 8)
    ring_buf, ring_d = _padded(ring, pad)
    ev_buf, ev_d = _padded(events)
    n_buf, n_d = _padded(torch.zeros(1, dtype=torch.int32))
    tp_buf, tp_d = (None, None) if tempo is None else _padded(tempo)
    g = torch.Generator().manual_seed(7)
    store = torch.randn(capacity, T_, E, generator=g)
    st_buf, st_d = _padded(store)
    hd_buf, hd_d = _padded(torch.zeros(1, dtype=torch.int32))
    wh_buf, wh_d = _padded(torch.full((M, 2), 99, dtype=torch.int32))
    wk_buf, wk_d = _padded(torch.full((eh.workspace_ints(capacity),), 55, dtype=torch.int32))
    more = {} if rates is None else dict(rates=rates)
    kept_any = wrapped = 0
    head = capacity - 1                                    # the first call starts at the store's last slot
    calls = [(kinds, n) for kinds in (1, 2, 3) for n in (M, 0, M + 5)] + [(3, M)] * 3      # the last ones in sequence: the head goes round
    for kinds, n in calls:
        n_d.fill_(n)
        hd_d.fill_(head)
        before = st_d.clone()
        runs = []
        for again in range(2):                             # twice from the same head and store: identical bytes
            hd_d.fill_(head)
            st_d.copy_(before)
            wh_d.fill_(99)
            eh.capture(ring_d, ev_d, n_d, tp_d, st_d, hd_d, wh_d, wk_d, uploader.upload(table), kinds, stride, rate, **more)
            runs.append((wh_d.clone(), hd_d.clone(), _bits(st_d).clone(), wk_d.clone()))
        assert all(torch.equal(a, b) for a, b in zip(*runs))
        where, new_head, want = reference_capture(ring, events, n, tempo, table, head, before.cpu(), kinds, T_, stride, rate, rates)
        assert torch.equal(wh_d.cpu(), where), (kinds, n)
        assert int(hd_d.item()) == new_head and 0 <= new_head < capacity, (kinds, n)
        assert torch.equal(_bits(st_d.cpu()), _bits(want)), (kinds, n)
        for buf, p in ((ring_buf, pad), (ev_buf, 64), (n_buf, 64), (st_buf, 64), (hd_buf, 64), (wh_buf, 64), (wk_buf, 64)):
            assert _intact(buf, p)
        assert torch.equal(_bits(ring_d.cpu()), _bits(ring)) and torch.equal(ev_d.cpu(), events) and int(n_d.item()) == n
        if tempo is not None:
            assert _intact(tp_buf) and torch.equal(tp_d.cpu(), tempo)
        taken = int((where[:, 0] >= 0).sum())
        if n == 0:
            assert taken == 0 and new_head == head and bool((where[:, 0] == -1).all())
        kept_any += taken
        wrapped += head + taken >= capacity
        head = new_head
    assert kept_any and wrapped >= 2                       # the cases captured something, and the head went round more than once


def test_every_code_of_where_and_a_tempo_out_of_range_in_one_call():
    """a hand-built call: 300 records over two chunks of the placement pass, every answer of `where` present, and the windows of the
    captured ones read back row by row"""
    from clip_fsar_amd import evidence_hip as eh
    from clip_fsar_amd.evidence import reference_capture
    T_, E, cap, stride, rates = 4, 8, 16, 2, (1, 3)
    ring = (torch.arange(2 * cap).view(2, cap, 1) * torch.ones(1, 1, E)).float()      # a row holds its own number
    #          slot pos0 nW keep0 out0 nc
    table = [[1, 14, 3, 1, 0, 2]]                          # windows 1 and 2 are in the ring: 2 + 9 + 1 = 12 frames of 16
    tempo = torch.tensor([0, 0, 0, 7, 1, -5], dtype=torch.int32)       # the cells (k, j); 7 and -5 read as R - 1 = 1
    recs = [[0, 0, 0, ONSET, 1], [0, 1, 1, ONSET, 1], [0, 0, 1, OFFSET, 4], [0, 0, 2, ONSET, 1], [0, 1, 2, ONSET, 1], [3, 0, 0, ONSET, 1]]
    events = torch.tensor(recs + [[0, 0, 1, ONSET, 1]] * 294, dtype=torch.int32)
    capacity = 5
    store = torch.full((capacity, T_, E), -1.0)
    where, head, want = reference_capture(ring, events, 300, tempo, table, 3, store, 1, T_, stride, 3, rates)
    assert where[:8].tolist() == [[-2, 0], [3, 1], [-1, 0], [4, 1], [0, 1], [-1, 0], [1, 0], [2, 0]] and head == 3
    assert bool((where[8:, 0] == -3).all())
    # window k of the row starts at ring position 14 + 2 k in its rmax = 3 form; tempo 0 (rate 1) lies 3 * (3 - 1) = 6 frames behind
    assert want[3, :, 0].tolist() == [16 + (0 + j * 3) % cap for j in range(T_)]                 # slot 3: k = 1 at rate 3: 16, 19, 22, 25
    assert want[1, :, 0].tolist() == [16 + (6 + j) % cap for j in range(T_)]                     # slot 1: k = 1 at rate 1: 22 .. 25
    dev = lambda t: t.to(DEV)
    st, hd, wh = dev(store), torch.tensor([3], dtype=torch.int32, device=DEV), torch.zeros(300, 2, dtype=torch.int32, device=DEV)
    eh.capture(dev(ring), dev(events), torch.tensor([300], dtype=torch.int32, device=DEV), dev(tempo), st, hd, wh,
               torch.empty(eh.workspace_ints(capacity), dtype=torch.int32, device=DEV), eh.table_uploader(DEV, 2).upload(table), 1, stride,
               3, rates=rates)
    assert torch.equal(wh.cpu(), where) and hd.item() == head and torch.equal(st.cpu(), want)


# ------------------------------------------------------------------ 2: the pool
STRIDE, MAX_PUSH = 2, 6
CAPACITY = 4


@pytest.fixture(scope="module")
def live():
    with torch.no_grad():
        return _gallery("live")


def _pool(live, rule, evidence=None, **kw):
    from clip_fsar_amd.pool import StreamPool
    kw.setdefault("stride", STRIDE)
    return StreamPool(live, max_streams=4, max_push=MAX_PUSH, events=rule, evidence=evidence, **kw)


class _Run:
    """One pool over the schedule: every push's outputs, the test's own frame history per (session, epoch), and the events taken late --
    `early` before a close() and a reset(), `late` after them."""

    def __init__(self, pool, E, big=False, lists=None):
        self.pool, self.E, self.outs, self.hist, self.tick = pool, E, [], {}, 0
        a, b = pool.open(classes=lists), pool.open()
        self.a, self.b = a, b
        for i in range(12):                                # 13-frame rings (27 with rates) wrap several times
            self.push({a: 3 + i % 4, b: 2 + (i % 3) * 2})
        if big:                                            # three rounds: the early windows of the push are overwritten by its later rounds
            self.big = self.push({a: 3 * MAX_PUSH, b: 3 * MAX_PUSH})
        self.early = pool.take_events() if pool._events is not None else []
        self.early_hist = {h: self.hist[h].clone() for h in (a, b)}
        pool.close(a)
        pool.reset(b)
        self.hist[b] = self.hist[b][:0]
        c = self.c = pool.open()                           # into a's slot
        for i in range(4):
            self.push({b: 6, c: 5})
        self.late = pool.take_events() if pool._events is not None else []

    def push(self, counts):
        self.tick += 1
        feats = {h: _feats(n, self.E, 4000 + 10 * self.tick + j) for j, (h, n) in enumerate(counts.items())}
        for h, f in feats.items():
            self.hist[h] = f.clone() if h not in self.hist else torch.cat([self.hist[h], f])
        out = self.pool.push_features(feats)
        self.outs.append(out)
        return out

    def scores(self):
        judged = lambda o: o.deviation if hasattr(o, "deviation") else (o.logits if o.smoothed is None else o.smoothed)
        flat = torch.cat([judged(o).reshape(-1) for out in self.outs for o in out.values()])
        return flat[~torch.isnan(flat)].cpu()

    def rows(self, e, hist=None, rate=1, rmax=1):
        """the frames of the event's window in the test's own history: e_k - (T - 1 - j) * rate, e_k the frame that completes it"""
        hist = self.hist if hist is None else hist
        last = e.window * self.pool.stride + (T - 1) * rmax
        return hist[e.session][[last - (T - 1 - j) * rate for j in range(T)]]

    def check_rows(self, features_of=None):
        """every event with evidence: its rows are the history's -- the early events against the history as it was before the close()
        and the reset() -> the number checked"""
        n = 0
        for events, hist in ((self.early, self.early_hist), (self.late, self.hist)):
            for e in events:
                if e.evidence is not None and self.pool.held(e):
                    assert torch.equal(self.pool.evidence_features(e), self.rows(e, hist)), e
                    n += 1
        return n


def _rule_from(scores, min_on=1, min_off=1):
    from clip_fsar_amd.events import EventRule
    on, off = (float(torch.quantile(scores, q)) for q in (0.55, 0.45))
    return EventRule(on, off, min_on, min_off)


def _same_outputs(x, y):
    assert len(x.outs) == len(y.outs)
    for ox, oy in zip(x.outs, y.outs):
        assert list(ox) == list(oy)
        for h in ox:
            assert type(ox[h]) is type(oy[h]) and ox[h].first_window == oy[h].first_window
            for name in ("logits", "smoothed", "deviation", "tempo"):
                u, v = getattr(ox[h], name, None), getattr(oy[h], name, None)
                assert (u is None) == (v is None) and (u is None or torch.equal(_bits(u), _bits(v))), (h, name)


@pytest.fixture(scope="module")
def runs(live):
    """the twin without a rule (whose scores give the thresholds), the twin with the rule alone, and the pools with evidence"""
    from clip_fsar_amd.evidence import Evidence
    with torch.no_grad():
        rule = _rule_from(_Run(_pool(live, None), live.E, big=True).scores())
        twin = _Run(_pool(live, rule), live.E, big=True)
        both = _Run(_pool(live, rule, Evidence(1024, ("onset", "offset"))), live.E, big=True)
        small = _Run(_pool(live, rule, Evidence(CAPACITY)), live.E)
    return rule, twin, both, small


def test_a_the_rows_are_the_history_after_wraps_a_close_and_a_reset(runs):
    from clip_fsar_amd.events import Event
    from clip_fsar_amd.evidence import EvidenceEvent
    rule, twin, both, small = runs
    events = both.early + both.late
    onsets = [e for e in events if e.kind == "onset"]
    assert len(onsets) >= CAPACITY + 3 and any(e.kind == "offset" for e in events)
    assert all(isinstance(e, EvidenceEvent) and e.tempo is None for e in events)
    assert all(type(e) is Event for e in twin.early + twin.late)                  # without the option: plain Events, as before
    assert {e.session for e in both.early} == {both.a, both.b} and {e.session for e in both.late} == {both.b, both.c}
    assert both.a not in both.pool.sessions and both.pool.stats(both.b)["frames"] == 24        # a is closed, b was reset
    assert max(e.window for e in both.early) * STRIDE > 3 * both.pool.cap                     # the rings wrapped several times
    checked = both.check_rows()
    captured = [e for e in events if e.evidence is not None]
    assert checked == len(captured) >= CAPACITY + 3
    assert sorted(e.evidence for e in captured) == list(range(len(captured)))                  # the serials count the captures
    # a single-round push misses nothing: every window it completes is still in the ring
    assert all(e.missed is None for e in events if e not in _of_push(both, both.big))
    # the events are the twin's, the outputs its bits
    assert [tuple(e[:8]) for e in events] == [tuple(e) for e in twin.early + twin.late]
    _same_outputs(both, twin)


def _of_push(run, out):
    """the run's events of the windows one push completed"""
    span = {h: range(o.first_window, o.first_window + o.logits.shape[0]) for h, o in out.items()}
    return [e for e in run.early if e.window in span[e.session]]


def test_b_only_the_newest_capacity_serials_are_held(runs):
    rule, twin, both, small = runs
    p = small.pool
    events = small.early + small.late
    captured = sorted((e for e in events if e.evidence is not None), key=lambda e: e.evidence)
    n = len(captured)
    assert n >= CAPACITY + 3 and [e.evidence for e in captured] == list(range(n))
    assert all(e.kind == "onset" for e in captured) and all(e.missed == "kind" for e in events if e.kind == "offset")
    assert [p.held(e) for e in captured] == [False] * (n - CAPACITY) + [True] * CAPACITY
    for e in captured[:n - CAPACITY]:
        with pytest.raises(ValueError, match="evidence %d is no longer held .* capacity = %d" % (e.evidence, CAPACITY)):
            p.evidence_features(e)
    assert small.check_rows() == CAPACITY                                         # the held ones are still the right rows
    missed = [e for e in events if e.missed in ("ring", "capacity")]
    stats = p.stats()
    assert stats["evidence"] == n and stats["evidence_missed"] == len(missed) and stats["events"] == len(events)
    assert all(e.missed == "capacity" for e in missed)                            # single-round pushes: only the store's room is missed
    with pytest.raises(TypeError, match="of another pool"):
        both.pool.held(captured[-1])


def test_c_a_push_of_three_rounds_misses_its_early_windows(runs):
    from clip_fsar_amd.evidence import keep0
    rule, twin, both, small = runs
    mine = [e for e in _of_push(both, both.big)]
    assert mine
    gone = captured = 0
    for h, o in both.big.items():
        nW = o.logits.shape[0]
        frames_after = both.early_hist[h].shape[0]
        k0 = keep0(o.first_window, nW, STRIDE, frames_after, both.pool.cap)
        assert 0 < k0 < nW
        for e in (e for e in mine if e.session == h):
            if e.window - o.first_window < k0:
                assert e.evidence is None and e.missed == "ring", e
                gone += 1
            else:
                assert e.missed is None and torch.equal(both.pool.evidence_features(e), both.rows(e, both.early_hist)), e
                captured += 1
    assert gone and captured
    assert both.pool.stats()["evidence_missed"] == gone
    for h in both.big:                                                            # the logits are the twin's
        assert torch.equal(both.big[h].logits, twin.big[h].logits)


def test_d_enrolment_and_explanation_long_after_the_fact():
    from clip_fsar_amd.align import Aligner
    from clip_fsar_amd.evidence import Evidence
    from test_gpu_enroll import _assert_same_classes
    with torch.no_grad():
        g1, g2 = _gallery("live", capacity=9), _gallery("live", capacity=9)
        rule = _rule_from(_Run(_pool(g1, None), g1.E).scores())
        late = _Run(_pool(g1, rule, Evidence(1024)), g1.E)
        e = next(e for e in late.early if e.kind == "onset" and e.window <= 3)    # an early window: dozens of pushes old
        assert e.session not in late.pool.sessions or e.window not in late.pool.enrolable(e.session)      # explain() and enroll() are past it
        rows = late.rows(e, late.early_hist)
        # explain_event: the Aligner's answer on the rows
        want = Aligner(g1).align_features(rows.unsqueeze(0), [e.class_id])
        got = late.pool.explain_event(e)
        assert all(torch.equal(getattr(got, n), getattr(want, n)) for n in ("plan", "dists", "logits")) and got.plan.shape[0] == 1
        top = late.pool.explain_event(e, k=2)
        assert top.plan.shape[0] == 2
        # the twin enrols the same window while it is in the ring
        class _Twin(_Run):
            def push(self, counts):
                out = super().push(counts)
                if e.session in self.pool.sessions and not getattr(self, "done", False) and e.window in self.pool.enrolable(e.session):
                    self.done = True
                    self.shots = (self.pool.enroll(e.session, IDS[0], window=e.window), self.pool.enroll(e.session, 15, window=e.window))
                return out
        twin = _Twin(_pool(g2, rule), g2.E)
        before = (late.pool.stats(), late.pool._ring.clone())
        assert (late.pool.enroll_event(e, IDS[0]), late.pool.enroll_event(e, 15)) == twin.shots == (2, 1)
        _assert_same_classes(g1, g2)
        assert g1.class_ids == IDS + [15]
        assert late.pool.stats() == before[0] and torch.equal(late.pool._ring, before[1])         # nothing of any session changed
        assert late.pool.take_events() == []


def test_e_bit_equal_to_the_twin_through_smoothing_a_baseline_a_removal_and_a_slot_reuse():
    from clip_fsar_amd.baseline import Baseline
    from clip_fsar_amd.evidence import Evidence

    class _Rich(_Run):
        def push(self, counts):
            out = super().push(counts)
            g = self.pool.gallery
            if self.tick == 7:                             # a class goes and another takes its slot while events run
                slot = g.slot_of(3)
                g.remove_classes([3])
                g.add_classes_features(_feats(T, self.E, 72).view(1, T, self.E), [11])
                assert g.slot_of(11) == slot
            return out

    kw = dict(smooth=0.5, smooth_by="class", baseline=Baseline(rate=1 / 8, warm_rate=0.5, warmup=3))
    with torch.no_grad():
        g0, g1, g2 = (_gallery("live") for _ in range(3))      # the schedule changes its gallery: each pool has one of its own, built alike
        rule = _rule_from(_Rich(_pool(g0, None, **kw), g0.E).scores())
        twin = _Rich(_pool(g1, rule, **kw), g1.E)
        mine = _Rich(_pool(g2, rule, Evidence(1024, ("onset", "offset")), **kw), g2.E)
    _same_outputs(mine, twin)
    events = mine.early + mine.late
    assert [tuple(e[:8]) for e in events] == [tuple(e) for e in twin.early + twin.late]
    assert sum(e.kind == "onset" for e in events) >= CAPACITY + 3 and 11 in {e.class_id for e in events}
    assert mine.check_rows() == len(events) and all(e.missed is None for e in events)
    assert mine.pool.stats()["evidence"] == len(events) and mine.pool.stats()["evidence_missed"] == 0


def test_f_with_rates_the_window_is_read_at_the_tempo_that_won_its_cell(live):
    from clip_fsar_amd.evidence import Evidence
    rates = (1, 2, 3)
    kw = dict(rates=rates)
    with torch.no_grad():
        rule = _rule_from(_Run(_pool(live, None, **kw), live.E).scores())
        twin = _Run(_pool(live, rule, **kw), live.E)
        mine = _Run(_pool(live, rule, Evidence(1024), **kw), live.E)
    _same_outputs(mine, twin)
    assert mine.pool.cap == (T - 1) * 3 + MAX_PUSH
    seen = 0                                               # cells: (session, window) -> the push's tempo row, per phase of the schedule
    for events, hist, outs in ((mine.early, mine.early_hist, mine.outs[:12]), (mine.late, mine.hist, mine.outs[12:])):
        cells = {(h, o.first_window + k): row for out in outs for h, o in out.items() for k, row in enumerate(o.tempo.tolist())}
        for e in events:
            if e.kind != "onset":
                assert e.evidence is None and e.missed == "kind" and e.tempo is None
                continue
            want = cells[(e.session, e.window)][live.class_ids.index(e.class_id)]
            assert e.tempo == want and e.missed is None, e
            assert torch.equal(mine.pool.evidence_features(e), mine.rows(e, hist, rates[e.tempo], rates[-1])), e
            seen += 1
    tempos = {e.tempo for e in mine.early + mine.late if e.evidence is not None}
    assert seen >= CAPACITY + 3 and len(tempos) >= 2 and tempos <= {0, 1, 2}


def test_g_a_shortlist_pool_and_a_session_with_a_class_list(live):
    from clip_fsar_amd.evidence import Evidence
    from clip_fsar_amd.shortlist import Shortlist
    with torch.no_grad():
        for kw, lists in ((lambda: dict(shortlist=Shortlist(live, keep=3), shortlist_hold=1), None), (dict, [9, 2, 4])):
            make = lambda rule, ev=None: _Run(_pool(live, rule, ev, **kw()), live.E, lists=lists)
            rule = _rule_from(make(None).scores())
            twin, mine = make(rule), make(rule, Evidence(1024))
            _same_outputs(mine, twin)
            events = mine.early + mine.late
            assert [tuple(e[:8]) for e in events] == [tuple(e) for e in twin.early + twin.late]      # the class ids as the events report them
            onsets = [e for e in events if e.kind == "onset"]
            assert len(onsets) >= CAPACITY + 3 and all(e.missed is None for e in onsets)
            assert mine.check_rows() == len(onsets)
            if lists is not None:
                assert {e.class_id for e in events if e.session == mine.a} <= set(lists)


def test_h_take_events_is_still_one_device_to_host_copy(live, monkeypatch):
    from clip_fsar_amd.evidence import Evidence
    from clip_fsar_amd.events import EventRule
    with torch.no_grad():
        p = _pool(live, EventRule(-1e30, -1e30), Evidence(8))                     # every pair's first window is an onset
        a, b = p.open(), p.open()
        for i in range(10):
            p.push_features({a: _feats(4, live.E, 10 + i), b: _feats(5, live.E, 50 + i)})
        assert len(p._ev_queue) == 9                                             # the first push completed no window
        calls = []
        real = torch.Tensor.cpu
        monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: (calls.append(tuple(self.shape)), real(self, *a, **k))[1])
        events = p.take_events()
        monkeypatch.undo()
        assert len(calls) == 1 and calls[0][0] == 9, calls
        assert len(events) == 2 * len(IDS) and {e.kind for e in events} == {"onset"}      # all twelve in one push: the store has room for 8
        assert p.stats()["evidence"] == 8 and p.stats()["evidence_missed"] == 4 and sum(p.held(e) for e in events) == 8
        assert sorted(e.missed for e in events if e.evidence is None) == ["capacity"] * 4
