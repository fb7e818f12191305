"""GPU: stream events (clip_fsar_amd.pool.StreamPool(events=EventRule(...)) on libclipfsar_events.so) -- the kernels through their binding,
records, values, state, marks and n_events bit for bit against clip_fsar_amd.events.reference_events in the contract's order (table row,
column, window): at the workgroup edges and every window count, over 300 rows (a scan across more than 256 workgroups), windows cut into
calls, shared and overlapping lists, valid and stale marks, a generation bumped between calls, keys out of range, NaN scores, on == off,
an event in every window, max_events below the total, and twice for identical bytes; then the pool: take_events() and active() against
the reference run per (session, class id) over the scores the same pushes returned, through class lists, enrolment with join, removals
with a new class in the freed slot, store growth, reset() and a reused slot, over a LiveGallery and a COMBINE LiveTextGallery."""
import random
import warnings

import pytest
import torch

from test_gpu_live import DEV, T, _pair

pytestmark = pytest.mark.gpu

CAP = 600                                         # store slots
PAD, NAN = 37, float("nan")
CHUNK = 256                                       # events_hip.CHUNK, the kernels' columns per workgroup (asserted below)
RULES = [(1, 1), (2, 2), (3, 2), (2, 3)]          # (min_on, min_off) at on 0.6 / off 0.4
F_SENTINEL, I_SENTINEL = -12345.0, -77


def _rule(min_on=1, min_off=1, on=0.6, off=0.4, max_events=1 << 15):
    from clip_fsar_amd.events import EventRule
    return EventRule(on, off, min_on, min_off, max_events)


# ------------------------------------------------------------------ 1: the kernels, through the binding
def _padded(t):
    """t inside a larger buffer with PAD sentinels on either side -> (buffer, the view holding t)"""
    sentinel = I_SENTINEL if t.dtype == torch.int32 else F_SENTINEL
    buf = torch.full((t.numel() + 2 * PAD,), sentinel, dtype=t.dtype, device=DEV)
    view = buf[PAD:PAD + t.numel()].view(t.shape)
    view.copy_(t)
    return buf, view


def _intact(buf):
    sentinel = I_SENTINEL if buf.dtype == torch.int32 else F_SENTINEL
    return bool((buf[:PAD] == sentinel).all()) and bool((buf[-PAD:] == sentinel).all())


def _bits(t):
    return t.contiguous().view(torch.int32)        # NaN-proof equality


class _Cells:
    """The four state arrays and gens of a kernel test, on the host (the model) and on the device between sentinels.  Every cell starts
    with a garbage mark and NaN / garbage state; the cells `named` (slot, key) are valid -- the mark is the slot's generation and the state
    one the rule can reach, idle or active -- or stale -- another mark, a NaN peak and garbage counters, so a read of them shows -- at random."""

    def __init__(self, named, rule, seed, M, all_stale=False):
        rng = random.Random(seed)
        g = torch.Generator().manual_seed(seed)
        self.M = M
        self.gens = torch.randint(1, 6, (CAP,), generator=g, dtype=torch.int32)
        self.streak = torch.randint(-9, 9, (M, CAP), generator=g, dtype=torch.int32)
        self.length = torch.randint(-9, 99, (M, CAP), generator=g, dtype=torch.int32)
        self.peak = torch.full((M, CAP), NAN)
        self.marks = torch.randint(-3, 9, (M, CAP), generator=g, dtype=torch.int32)
        for slot, key in sorted(named):
            gen = int(self.gens[key])
            if all_stale or rng.random() < 0.5:
                self.marks[slot, key] = rng.choice((0, gen - 1, gen + 1, -gen))
                continue
            self.marks[slot, key] = gen
            if rng.random() < 0.5:                 # idle, within a streak or not
                self.streak[slot, key] = rng.randrange(rule.min_on)
                self.peak[slot, key] = torch.tensor(rng.uniform(0.6, 1.0), dtype=torch.float32)
            else:                                  # active, within a run below off or not
                self.streak[slot, key] = -1 - rng.randrange(rule.min_off)
                self.length[slot, key] = rng.randrange(rule.min_on, 40)
                self.peak[slot, key] = torch.tensor(rng.uniform(0.6, 1.0), dtype=torch.float32)
        self.dev = {n: _padded(getattr(self, n)) for n in ("streak", "length", "peak", "marks", "gens")}

    def clone(self):
        other = object.__new__(_Cells)
        other.M = self.M
        for n in ("streak", "length", "peak", "marks", "gens"):
            setattr(other, n, getattr(self, n).clone())
        other.dev = {n: _padded(getattr(other, n)) for n in ("streak", "length", "peak", "marks", "gens")}
        return other

    def model(self, rows, keys, x, rule):
        """the reference over one call: advances the host arrays, -> the records [(row, j, k, kind, len)], [(score, peak)] in the
        contract's order"""
        from clip_fsar_amd.events import Cell, reference_events
        events, values, at = [], [], 0
        for r, (slot, nW, key0, NC) in enumerate(rows):
            blk = x[at:at + nW * NC].view(nW, NC).t().tolist()
            at += nW * NC
            for j in range(NC if nW else 0):
                key = keys[key0 + j]
                if not 0 <= key < CAP:
                    continue
                valid = int(self.marks[slot, key]) == int(self.gens[key])
                cell = Cell(int(self.streak[slot, key]), int(self.length[slot, key]), float(self.peak[slot, key])) if valid else None
                recs, cell = reference_events(blk[j], rule, cell)
                for rec in recs:
                    events.append((r, j, rec.k, rec.kind, rec.len))
                    values.append((rec.score, rec.peak))
                self.streak[slot, key], self.length[slot, key], self.marks[slot, key] = cell.streak, cell.length, self.gens[key]
                self.peak[slot, key] = torch.tensor(cell.peak, dtype=torch.float32)
        return events, values

    def check(self):
        """the device arrays are the model's, bit for bit, between intact sentinels"""
        for n, (buf, view) in self.dev.items():
            assert _intact(buf), n
            assert torch.equal(_bits(view.cpu()), _bits(getattr(self, n))), n


def _table(rows):
    table, n_out, chunks = [], 0, 0
    for slot, nW, key0, NC in rows:
        table.append([slot, nW, n_out, NC, key0, chunks])
        n_out += nW * NC
        chunks += -(-NC // CHUNK)
    return table, n_out, chunks


def _launch(cells, rows, keys, x, rule, uploader):
    """one cfev_detect; scores, keys, events, values, n_events and work lie between sentinels, which must survive, and scores, keys and
    gens come back unchanged -> (events [max_events, 5], values [max_events, 2], n_events) on the host"""
    from clip_fsar_amd import events_hip as eh
    assert eh.CHUNK == CHUNK
    table, n_out, chunks = _table(rows)
    assert n_out == x.numel()
    kbuf, kd = _padded(torch.tensor(keys, dtype=torch.int32))
    xbuf, xd = _padded(x)
    ebuf, ed = _padded(torch.full((rule.max_events, 5), -99, dtype=torch.int32))
    vbuf, vd = _padded(torch.full((rule.max_events, 2), -99.0))
    nbuf, nd = _padded(torch.full((1,), -99, dtype=torch.int32))
    wbuf, wd = _padded(torch.full((eh.workspace_ints(chunks),), -99, dtype=torch.int32))
    d = cells.dev
    eh.detect(xd, d["streak"][1], d["length"][1], d["peak"][1], d["marks"][1], d["gens"][1], kd, ed, vd, nd, wd, uploader.upload(table),
              rule.on, rule.off, rule.min_on, rule.min_off)
    torch.cuda.synchronize()
    for buf in (kbuf, xbuf, ebuf, vbuf, nbuf, wbuf):
        assert _intact(buf)
    assert torch.equal(kd.cpu(), torch.tensor(keys, dtype=torch.int32)) and torch.equal(_bits(xd.cpu()), _bits(x))
    return ed.cpu(), vd.cpu(), int(nd.cpu())


def _compare(got, want_events, want_values, rule):
    events, values, n = got
    total, kept = len(want_events), min(len(want_events), rule.max_events)
    assert n == total, (n, total)
    assert events[:kept].tolist() == [list(e) for e in want_events[:kept]]
    assert torch.equal(_bits(values[:kept]), _bits(torch.tensor(want_values[:kept], dtype=torch.float32).view(kept, 2)))
    assert bool((events[kept:] == -99).all()) and bool((values[kept:] == -99.0).all())       # nothing beyond the records


def _named(rows, keys):
    return {(slot, keys[key0 + j]) for slot, nW, key0, NC in rows for j in range(NC) if 0 <= keys[key0 + j] < CAP}


def _kinds(events):
    return {e[3] for e in events}


def _case(rows, keys, rule, M=6, need_both=True, scores=None, all_stale=False, seed0=0):
    """Build a case whose reference alone shows an onset and an offset (the first seed that does: the inputs are chosen on the model, the
    kernels are not asked), run it once, compare everything -> (the cells afterwards, the launch's answer, the scores, the cells before)"""
    from clip_fsar_amd import events_hip as eh
    n = sum(nW * NC for _, nW, _, NC in rows)
    for seed in range(seed0, seed0 + 400):
        x = torch.rand(n, generator=torch.Generator().manual_seed(seed)) if scores is None else scores(n, seed)
        cells = _Cells(_named(rows, keys), rule, seed, M, all_stale)
        model = cells.clone()
        want_events, want_values = model.model(rows, keys, x, rule)
        if not need_both or _kinds(want_events) == {1, 2}:
            break
    assert not need_both or _kinds(want_events) == {1, 2}              # no case is vacuous
    start = cells.clone()
    got = _launch(cells, rows, keys, x, rule, eh.table_uploader(DEV, M))
    _compare(got, want_events, want_values, rule)
    for name in ("streak", "length", "peak", "marks", "gens"):
        setattr(cells, name, getattr(model, name))
    cells.check()
    return cells, got, x, start


def _perm(n, seed):
    return torch.randperm(CAP, generator=torch.Generator().manual_seed(seed))[:n].tolist()


@pytest.mark.parametrize("min_on,min_off", RULES)
@pytest.mark.parametrize("NC", [1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1])
def test_widths_at_the_workgroup_edges_and_every_window_count(NC, min_on, min_off):
    """five sessions of one width and one window count per launch, each with a list of its own"""
    rule = _rule(min_on, min_off)
    keys = _perm(CAP, NC)
    rows = lambda nW: [(slot, nW, key0, NC) for slot, key0 in zip((3, 0, 5, 1, 4), (0, 17, 40, 86, 87))]
    for nW in (0, 1, 2, 7, 12):
        # (2 windows confirm an onset and an offset in one launch only from cells that are part of the way there, in different columns)
        _, got, _, _ = _case(rows(nW), keys, rule, need_both=nW > 1, seed0=100 * nW)
        assert nW or got[2] == 0                   # no windows: nothing is launched, the binding zeroes n_events itself


@pytest.mark.parametrize("min_on,min_off", RULES)
def test_three_hundred_rows_of_one_column(min_on, min_off):
    """300 workgroups: the scan of the workgroup totals crosses its tile of 256"""
    keys = _perm(CAP, 3)
    rows = [(slot, 12 if slot % 7 else 0, (slot * 13) % CAP, 1) for slot in range(300)]
    _, got, _, _ = _case(rows, keys, _rule(min_on, min_off), M=300)
    assert got[2] > 40


GEOMETRY = [(5, 0, CHUNK + 1), (0, 0, CHUNK + 1), (2, 45, CHUNK - 1), (4, 299, 1), (1, 87, 2 * CHUNK + 1)]   # (slot, key0, NC)


@pytest.mark.parametrize("min_on,min_off", RULES)
def test_shared_and_overlapping_lists_and_windows_cut_into_calls(min_on, min_off):
    """two sessions share one list, a third one's starts and ends inside it, over different slots; the same 12 windows in one call, as
    twelve calls of one and as 5 + 0 + 7 give the reference's records call by call -- hence one event stream -- and one final state"""
    from clip_fsar_amd import events_hip as eh
    rule = _rule(min_on, min_off)
    keys = _perm(CAP, 14)
    rows = lambda n: [(slot, n, key0, NC) for slot, key0, NC in GEOMETRY]
    cells, got, x, start = _case(rows(12), keys, rule)
    assert got[2] > 100
    whole = sorted(tuple(e) for e in got[0][:got[2]].tolist())
    blocks, at = [], 0
    for _, _, NC in GEOMETRY:
        blocks.append(x[at:at + 12 * NC].view(12, NC))
        at += 12 * NC
    up = eh.table_uploader(DEV, 6)
    for cuts in ([1] * 12, [5, 0, 7]):
        replay, model = start.clone(), start.clone()
        k0, stream = 0, []
        for n in cuts:
            xs = torch.cat([b[k0:k0 + n].reshape(-1) for b in blocks])
            want = model.model(rows(n), keys, xs, rule)
            part = _launch(replay, rows(n), keys, xs, rule, up)
            _compare(part, *want, rule)            # (a call without windows launches nothing and reports no record)
            stream += [(r, j, k + k0, kind, ln) for r, j, k, kind, ln in want[0]]
            k0 += n
        for name in ("streak", "length", "peak", "marks", "gens"):
            setattr(replay, name, getattr(model, name))
        replay.check()
        for name in ("streak", "length", "peak", "marks"):            # the final state of the single call
            assert torch.equal(_bits(getattr(replay, name)), _bits(getattr(cells, name))), (cuts, name)
        assert sorted(stream) == whole, cuts


@pytest.mark.parametrize("min_on,min_off", RULES)
def test_a_generation_bumped_between_two_calls_restarts_the_pair_without_an_offset(min_on, min_off):
    from clip_fsar_amd import events_hip as eh
    rule = _rule(min_on, min_off)
    keys = _perm(CAP, 15)
    rows = [(slot, 7, key0, NC) for slot, key0, NC in GEOMETRY[:3]]
    cells, _, _, _ = _case(rows, keys, rule)
    active = [(s, k) for s, k in sorted(_named(rows, keys)) if int(cells.streak[s, k]) < 0]
    bumped = sorted({k for _, k in active[::2]})
    assert len(bumped) > 20                        # pairs whose event is running lose their class
    for k in bumped:
        cells.gens[k] += 1
    cells.dev["gens"][1].copy_(cells.gens)
    x = torch.rand(7 * sum(NC for _, _, _, NC in rows), generator=torch.Generator().manual_seed(77)) * 0.3      # everything below off
    model = cells.clone()
    want_events, want_values = model.model(rows, keys, x, rule)
    got = _launch(cells, rows, keys, x, rule, eh.table_uploader(DEV, 6))
    _compare(got, want_events, want_values, rule)
    closed = {(rows[r][0], keys[rows[r][2] + j]) for r, j, k, kind, ln in want_events if kind == 2}
    assert closed == {(s, k) for s, k in active if k not in bumped} and closed      # every running event ends, but those of a bumped slot
    for name in ("streak", "length", "peak", "marks"):
        setattr(cells, name, getattr(model, name))
    cells.check()
    assert all(int(cells.marks[s, k]) == int(cells.gens[k]) and int(cells.streak[s, k]) == 0 for s, k in active)


@pytest.mark.parametrize("bad", [-1, CAP, 1 << 30])
def test_a_key_out_of_range_emits_nothing_and_writes_no_state(bad):
    keys = _perm(CAP, 13)
    for j in (0, 7, CHUNK - 1, CHUNK, 298):
        keys[j] = bad
    for min_on, min_off in RULES:
        _case([(2, 7, 0, CHUNK + 1), (4, 12, 200, 100), (0, 0, 0, 8)], keys, _rule(min_on, min_off))
    _case([(2, 1, 7, 1)], keys, _rule(), need_both=False)


@pytest.mark.parametrize("min_on,min_off", RULES)
def test_nan_scores_in_both_phases(min_on, min_off):
    from clip_fsar_amd.events import reference_events
    rule = _rule(min_on, min_off)

    def scores(n, seed):
        g = torch.Generator().manual_seed(seed)
        x = torch.rand(n, generator=g)
        x[torch.rand(n, generator=g) < 0.1] = NAN
        return x

    keys = _perm(CAP, 16)
    rows = [(1, 12, 3, CHUNK + 1)]
    _, _, x, _ = _case(rows, keys, rule, scores=scores, all_stale=True)
    phases = set()                                 # the NaNs met idle cells and active ones (every cell started idle: all stale)
    for col in x.view(12, CHUNK + 1).t().tolist():
        for k, s in enumerate(col):
            if s != s:
                phases.add(reference_events(col[:k], rule)[1].streak < 0)
    assert phases == {False, True}


@pytest.mark.parametrize("min_on,min_off", RULES)
def test_on_equal_to_off(min_on, min_off):
    _case([(slot, 12, key0, NC) for slot, key0, NC in GEOMETRY[:3]], _perm(CAP, 17), _rule(min_on, min_off, on=0.5, off=0.5))


def test_an_event_in_every_window():
    """the column 1, 0, 1, 0 ... under min_on = min_off = 1 from idle cells: every window of every column confirms a transition"""
    rows = [(3, 12, 0, CHUNK + 1), (0, 7, 100, 2 * CHUNK + 1 - 100)]
    n_out = sum(nW * NC for _, nW, _, NC in rows)

    def scores(n, seed):
        return torch.cat([(1 - torch.arange(nW) % 2).float()[:, None].expand(nW, NC).reshape(-1) for _, nW, _, NC in rows])

    _, got, _, _ = _case(rows, _perm(CAP, 18), _rule(max_events=n_out + 5), scores=scores, all_stale=True)
    assert got[2] == n_out


@pytest.mark.parametrize("max_events", [1, 100, 257])
def test_max_events_below_the_total_keeps_the_prefix_and_the_true_count(max_events):
    rows = [(slot, 12, key0, NC) for slot, key0, NC in GEOMETRY]
    for min_on, min_off in RULES:
        _, got, _, _ = _case(rows, _perm(CAP, 19), _rule(min_on, min_off, max_events=max_events))      # _compare: the prefix; state: advanced
        assert got[2] > max_events


def test_two_identical_runs_give_identical_bytes():
    from clip_fsar_amd import events_hip as eh
    rule = _rule(2, 2)
    keys = _perm(CAP, 20)
    rows = [(slot, 12, key0, NC) for slot, key0, NC in GEOMETRY] + [(3, 12, 9, 1)]
    x = torch.rand(sum(nW * NC for _, nW, _, NC in rows), generator=torch.Generator().manual_seed(1))
    runs = []
    for _ in range(2):
        cells = _Cells(_named(rows, keys), rule, 5, 6)
        events, values, n = _launch(cells, rows, keys, x, rule, eh.table_uploader(DEV, 6))
        runs.append([events, _bits(values), torch.tensor(n)] + [_bits(cells.dev[k][1].cpu()) for k in ("streak", "length", "peak", "marks")])
    assert runs[0][2] > 100 and all(torch.equal(a, b) for a, b in zip(*runs))


# ------------------------------------------------------------------ 2: the pool
IDS = [1, 2, 3, 4, 7, 9]
STRIDE, MAX_PUSH, ALPHA = 1, 6, 0.5


def _feats(n, E, seed):
    return torch.randn(n, E, generator=torch.Generator().manual_seed(seed)).to(DEV)


def _gallery(kind, capacity=6, seed=5):
    """test_gpu_class_smooth's: a LiveGallery, or a COMBINE LiveTextGallery, holding the classes IDS in a store that is full at 6"""
    if kind == "live":
        live = _pair(capacity=capacity)[1]
    else:
        from test_gpu_live_text import _galleries
        live = _galleries("fp32", "combine", capacity=capacity)[1]
    live.add_classes_features(_feats(len(IDS) * T, live.E, seed).view(len(IDS), T, live.E), IDS)
    assert live.class_ids == IDS
    return live


def _pool(live, smooth, rule):
    from clip_fsar_amd.pool import StreamPool
    return StreamPool(live, max_streams=4, stride=STRIDE, max_push=MAX_PUSH, smooth=smooth, smooth_by="class", events=rule)


class _Pairs:
    """The reference over what a pool returned: a cell per (session key, class id), restarted where the contract restarts a pair -- the
    session's open() / reset(), the class's registration, the class joining the session's list -- and advanced over the pair's column of
    every StreamOutput in push order."""

    def __init__(self, rule):
        self.rule, self.cells, self.events = rule, {}, []

    def forget(self, session=None, cid=None):
        for key in [k for k in self.cells if (session is None or k[0] == session) and (cid is None or k[1] == cid)]:
            del self.cells[key]

    def saw(self, outs, ids_of):
        """outs: {session: StreamOutput} of one push, in push order; ids_of: session -> its columns' class ids.  Events in take_events'
        order: the sessions as pushed, then window, then column."""
        from clip_fsar_amd.events import Event, reference_events
        for h, out in outs.items():
            scores = out.logits if out.smoothed is None else out.smoothed
            mine = []
            for j, (cid, col) in enumerate(zip(ids_of[h], scores.t().tolist())):
                recs, self.cells[(h, cid)] = reference_events(col, self.rule, self.cells.get((h, cid)))
                for r in recs:
                    w = out.first_window + r.k
                    start = w - self.rule.min_on + 1 if r.kind == 1 else w - self.rule.min_off - r.len + 1
                    mine.append((w, j, Event(h, cid, "onset" if r.kind == 1 else "offset", w, start, r.len, r.score, r.peak)))
            self.events += [e for _, _, e in sorted(mine, key=lambda t: t[:2])]

    def active(self, h, ids):
        return [(c, self.cells[(h, c)].length, self.cells[(h, c)].peak) for c in ids if (h, c) in self.cells and self.cells[(h, c)].streak < 0]


def _schedule(live, pool, pairs=None, taken=None):
    """test_gpu_class_smooth's membership schedule with a reset() and a close() + open() into the same slot added; with pairs: the model
    follows; -> every score the pushes returned, flat"""
    E = live.E
    a, b, c = pool.open(), pool.open(classes=[9, 2]), pool.open(classes=[4, 9, 1])
    hs = {"a": a, "b": b, "c": c}
    tick, seen = [0], []

    def ids_of(h):
        return list(live.class_ids if pool._sessions[h].classes is None else pool._sessions[h].classes)

    def push(counts, take=False):
        tick[0] += 1
        feats = {hs[n]: _feats(k, E, 300 + 10 * tick[0] + i) for i, (n, k) in enumerate(zip("abc", counts)) if k}
        out = pool.push_features(feats)
        for h in feats:
            seen.append((out[h].logits if out[h].smoothed is None else out[h].smoothed).reshape(-1))
        if pairs is not None:
            pairs.saw(out, {h: ids_of(h) for h in feats})
            if take:                               # some pushes are taken at once, the others wait in the queue
                taken.extend(pool.take_events())
            for h in feats:
                assert pool.active(h) == pairs.active(h, ids_of(h)), (tick[0], h)
        return out

    def new_class(cid, seed):
        live.add_classes_features(_feats(T, E, seed).view(1, T, E), [cid])
        if pairs is not None:
            pairs.forget(cid=cid)

    push((9, 10, 8))
    assert live.capacity == 6
    assert pool.enroll(a, 15) == 1                                    # a new class while streams run: the store grows 6 -> 9
    assert live.capacity == 9
    push((2, 8, 3), take=True)
    assert pool.enroll(b, 16, join=True) == 1 and pool._sessions[b].classes == [9, 2, 16]
    push((3, 2, 0))
    live.add_shots_features(_feats(T, E, 71).view(1, T, E), [9])      # further shots: the prototype moves, the state stays
    push((1, 3, 4))
    slot = live.slot_of(3)
    live.remove_classes([3])                                          # a running event of class 3 ends silently ...
    new_class(11, 72)
    assert live.slot_of(11) == slot                                   # ... and 11, in its slot, starts idle
    push((7, 1, 2), take=True)
    pool.reset(b)
    if pairs is not None:
        pairs.forget(session=b)
    push((2, 9, 2))
    push((13, 1, 0))                                                  # beyond max_push: three rounds, one detector call
    pool.close(c)
    d = pool.open(classes=[7, 11, 4])                                 # into c's slot
    assert pool._sessions[d].slot == 2
    hs["c"] = d
    push((3, 0, 12), take=True)
    push((6, 5, 4))
    assert live.class_ids == [1, 2, 4, 7, 9, 15, 16, 11]
    return torch.cat(seen)


@pytest.mark.parametrize("kind,smooth,min_on,min_off", [("live", ALPHA, 2, 2), ("live", 0.0, 1, 1), ("combine", ALPHA, 2, 1),
                                                        ("combine", 0.0, 3, 2)])
def test_the_pool_reports_the_reference_events(kind, smooth, min_on, min_off):
    """the thresholds are quantiles of the scores a first pool without a rule returns over the same pushes; that pool's scores are the
    bits of the pool with a rule, whose events are the reference's over them"""
    from clip_fsar_amd.events import EventRule
    with torch.no_grad():                          # the schedule changes its gallery: each pool runs it over a gallery of its own, built alike
        live = _gallery(kind)
        plain_scores = _schedule(live, _pool(live, smooth, None))
    on, off = (float(torch.quantile(plain_scores.cpu(), q)) for q in (0.6, 0.4))
    rule = EventRule(on, off, min_on, min_off)
    pairs, taken = _Pairs(rule), []
    with torch.no_grad():
        live = _gallery(kind)
        pool = _pool(live, smooth, rule)
        scores = _schedule(live, pool, pairs, taken)
        taken.extend(pool.take_events())
    assert torch.equal(scores, plain_scores)                           # events=None returns the same bits
    kinds = [e.kind for e in pairs.events]
    assert kinds.count("onset") >= 10 and kinds.count("offset") >= 5, (kinds.count("onset"), kinds.count("offset"))
    assert taken == pairs.events
    assert pool.take_events() == [] and pool.stats()["events"] == len(taken) and pool.stats()["events_dropped"] == 0
    assert {e.session for e in taken} >= set(pool.sessions) and {11, 15, 16} & {e.class_id for e in taken}


def test_dropped_records_warn_and_are_counted_and_a_full_queue_translates_its_oldest_batch(monkeypatch):
    from clip_fsar_amd import pool as pool_mod
    from clip_fsar_amd.events import EventRule
    with torch.no_grad():
        live = _gallery("live")
        rule = EventRule(-1e30, -1e30, 1, 1, max_events=4)            # every score is at or above on: an onset per pair, 6 a push
        pool = _pool(live, 0.0, rule)
        monkeypatch.setattr(pool_mod, "EVENT_QUEUE", 2)
        hs = [pool.open() for _ in range(3)]
        with warnings.catch_warnings():
            warnings.simplefilter("error", RuntimeWarning)            # the pushes below do not warn ...
            for h in hs[:2]:
                pool.push_features({h: _feats(T + 1, live.E, 2 + h)})
        assert len(pool._ev_queue) == 2
        with pytest.warns(RuntimeWarning, match="2 event records beyond max_events = 4"):
            pool.push_features({hs[2]: _feats(T + 1, live.E, 9)})         # ... a third one onto the full queue translates the first
        assert len(pool._ev_queue) == 2 and len(pool._ev_ready) == 4 and pool.stats()["events_dropped"] == 2
        with pytest.warns(RuntimeWarning, match="4 event records"):
            events = pool.take_events()
        assert [e.session for e in events] == [hs[0]] * 4 + [hs[1]] * 4 + [hs[2]] * 4 and {e.kind for e in events} == {"onset"}
        assert [e.class_id for e in events[:4]] == IDS[:4] and pool.stats()["events"] == 12 and pool.stats()["events_dropped"] == 6
        assert [c for c, _, _ in pool.active(hs[0])] == IDS            # the state advanced all the same


def test_constructor_refusals():
    from clip_fsar_amd.events import EventRule
    from clip_fsar_amd.pool import StreamPool
    rule = EventRule(0.6, 0.4)
    _, live, static = _pair(capacity=6)
    with pytest.raises(ValueError, match="events=.*slot store"):
        StreamPool(static, events=rule)
    with pytest.raises(ValueError, match="events=.*smooth_by=\"class\""):
        StreamPool(live, smooth=0.5, events=rule)
    with pytest.raises(TypeError, match="EventRule"):
        StreamPool(live, events=(0.6, 0.4))
    assert StreamPool(live, smooth=0.5, smooth_by="class", events=rule).stats()["events"] == 0
