"""GPU: adaptive baselines (clip_fsar_amd.pool.StreamPool(baseline=Baseline(...)) on libclipfsar_baseline.so) -- the kernel through its
binding, `out` and the four state arrays bit for bit against clip_fsar_amd.baseline.reference_baseline, with sentinels behind every
buffer and scores, keys and gens unchanged: at the workgroup edges and every window count, over 300 rows, shared and overlapping lists,
valid and stale marks, a generation bumped between calls, keys out of range, non-finite scores, warmup = 1, gate = +inf, out aliasing
scores, windows cut into calls, and twice for identical bytes; then the pool: deviation, baseline(h), take_events() and active() against
reference_baseline followed by reference_events, run per (session, class id) over the scores a pool without the option returned over the
same pushes, through class lists, enrolment with join, removals with a new class in the freed slot, store growth, reset() and a reused
slot, over a LiveGallery and a COMBINE LiveTextGallery; and one rule in deviation units that finds the same events on both galleries.

The inputs of the kernel tests are the three scales the pool's scores come in -- N(-8, 0.5), N(0.02, 0.004), N(-40, 3), the scale a
property of the class's store slot -- with a plateau of +8 sigma; the rates are powers of two.  Every case first asserts on the reference
alone that a window was gated, that a window after warm-up was folded in, and that EventRule(4, 2, 2, 2) finds an onset and an offset in
the deviations."""
import random

import pytest
import torch

from test_gpu_live import DEV, T, _pair

pytestmark = pytest.mark.gpu

CAP = 600                                         # store slots
PAD, NAN, INF = 37, float("nan"), float("inf")
CHUNK = 256                                       # baseline_hip.CHUNK, the kernel's columns per workgroup (asserted below)
F_SENTINEL, I_SENTINEL = -12345.0, -77
SCALES = [(-8.0, 0.5), (0.02, 0.004), (-40.0, 3.0)]        # (mean, sigma) of a store slot's scores: slot % 3
STATE = ("mean", "dev", "count", "marks", "gens")


def _base(rate=1 / 16, warm_rate=0.25, warmup=4, gate=3.0, floor=1e-6):
    from clip_fsar_amd.baseline import Baseline
    return Baseline(rate, warm_rate, warmup, gate, floor)


def _event_rule():
    from clip_fsar_amd.events import EventRule
    return EventRule(4, 2, 2, 2)


# ------------------------------------------------------------------ 1: the kernel, through the binding
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
    with a garbage mark, NaN mean and deviation and a garbage count; the cells `named` (slot, key) are valid -- the mark is the slot's
    generation and the cell one the recurrence can reach, in warm-up or past it, at the key's scale -- or stale -- another mark, NaN and
    garbage left in place, so a read of them shows -- at random.  history: the deviations of every pair, call after call."""

    def __init__(self, named, rule, seed, M, all_stale=False):
        rng = random.Random(seed)
        g = torch.Generator().manual_seed(seed)
        self.M = M
        self.gens = torch.randint(1, 6, (CAP,), generator=g, dtype=torch.int32)
        self.mean = torch.full((M, CAP), NAN)
        self.dev = torch.full((M, CAP), NAN)
        self.count = torch.randint(-9, 99, (M, CAP), generator=g, dtype=torch.int32)
        self.marks = torch.randint(-3, 9, (M, CAP), generator=g, dtype=torch.int32)
        self.history = {}
        for slot, key in sorted(named):
            gen = int(self.gens[key])
            if all_stale or rng.random() < 0.5:
                self.marks[slot, key] = rng.choice((0, gen - 1, gen + 1, -gen))
                continue
            mu, sigma = SCALES[key % 3]
            self.marks[slot, key] = gen
            self.count[slot, key] = rng.randrange(1, rule.warmup + 1)
            self.mean[slot, key] = torch.tensor(rng.gauss(mu, 0.3 * sigma), dtype=torch.float32)
            self.dev[slot, key] = torch.tensor(rng.uniform(0.6, 1.0) * sigma, dtype=torch.float32)
        self.upload()

    def upload(self):
        self.device = {n: _padded(getattr(self, n)) for n in STATE}

    def clone(self):
        other = object.__new__(_Cells)
        other.M, other.history = self.M, {k: list(v) for k, v in self.history.items()}
        for n in STATE:
            setattr(other, n, getattr(self, n).clone())
        other.upload()
        return other

    def model(self, rows, keys, x, rule):
        """the reference over one call: advances the host arrays -> the deviations, flat in the layout of x"""
        from clip_fsar_amd.baseline import Cell, reference_baseline
        out, at = torch.empty_like(x), 0
        for slot, nW, key0, NC in rows:
            blk = x[at:at + nW * NC].view(nW, NC).t().tolist()
            z = out[at:at + nW * NC].view(nW, NC)
            at += nW * NC
            for j in range(NC if nW else 0):
                key = keys[key0 + j]
                if not 0 <= key < CAP:
                    z[:, j] = NAN
                    continue
                valid = int(self.marks[slot, key]) == int(self.gens[key])
                cell = Cell(float(self.mean[slot, key]), float(self.dev[slot, key]), int(self.count[slot, key])) if valid else None
                if not valid:
                    self.history[(slot, key)] = []         # the pair starts anew: so does the rule that would judge it
                zs, cell = reference_baseline(blk[j], rule, cell)
                z[:, j] = torch.tensor(zs, dtype=torch.float32)
                self.history.setdefault((slot, key), []).extend(zs)
                self.mean[slot, key] = torch.tensor(cell.mean, dtype=torch.float32)
                self.dev[slot, key] = torch.tensor(cell.dev, dtype=torch.float32)
                self.count[slot, key], self.marks[slot, key] = cell.n, self.gens[key]
        return out

    def adopt(self, model):
        for n in STATE:
            setattr(self, n, getattr(model, n))
        self.history = model.history

    def check(self):
        """the device arrays are the model's, bit for bit, between intact sentinels"""
        for n, (buf, view) in self.device.items():
            assert _intact(buf), n
            assert torch.equal(_bits(view.cpu()), _bits(getattr(self, n))), n

    def shows(self, rule, gated=True):
        """what every case asserts on the reference alone: a window was gated (gate = +inf: none was, though one stood out), a window
        after warm-up was folded in, and EventRule(4, 2, 2, 2) finds an onset and an offset in the deviations"""
        from clip_fsar_amd.events import reference_events
        zs = [z for h in self.history.values() for z in h if z == z]
        out_standing = sum(z >= (rule.gate if gated else 3.0) for z in zs)
        assert out_standing >= 1 and sum(z < rule.gate for z in zs) >= 1, (out_standing, len(zs))
        assert gated or not any(z >= rule.gate for z in zs)
        kinds = {r.kind for h in self.history.values() for r in reference_events(h, _event_rule())[0]}
        assert kinds == {1, 2}, kinds


def _table(rows):
    table, n_out, chunks = [], 0, 0
    for slot, nW, key0, NC in rows:
        table.append([slot, nW, n_out, NC, key0, chunks])
        n_out += nW * NC
        chunks += -(-NC // CHUNK)
    return table, n_out, chunks


def _scores(rows, keys, seed, plateau=(5, 9), bad=0.0):
    """the rows' blocks, flat: every column N(mean, sigma) of its key's scale, + 8 sigma over the windows `plateau` of the call; bad: the
    share of non-finite scores"""
    g = torch.Generator().manual_seed(seed)
    blocks = []
    for slot, nW, key0, NC in rows:
        scale = torch.tensor([SCALES[keys[key0 + j] % 3] for j in range(NC)])
        blk = scale[:, 0] + scale[:, 1] * torch.randn(nW, NC, generator=g)
        blk[plateau[0]:plateau[1]] += 8 * scale[:, 1]
        if bad:
            kind = torch.rand(nW, NC, generator=g)
            blk[kind < bad] = NAN
            blk[(kind >= bad) & (kind < 1.5 * bad)] = INF
            blk[(kind >= 1.5 * bad) & (kind < 2 * bad)] = -INF
        blocks.append(blk.reshape(-1))
    return torch.cat(blocks) if blocks else torch.empty(0)


def _launch(cells, rows, keys, x, rule, uploader, alias=False):
    """one cfbl_normalize; scores, keys and out lie between sentinels, which must survive, and scores, keys and gens come back unchanged
    (alias: out is scores) -> out on the host"""
    from clip_fsar_amd import baseline_hip as bh
    assert bh.CHUNK == CHUNK
    table, n_out, _ = _table(rows)
    assert n_out == x.numel()
    kbuf, kd = _padded(torch.tensor(keys, dtype=torch.int32))
    xbuf, xd = _padded(x)
    obuf, od = (xbuf, xd) if alias else _padded(torch.full((n_out,), -99.0))
    d = cells.device
    bh.normalize(xd, d["mean"][1], d["dev"][1], d["count"][1], d["marks"][1], d["gens"][1], kd, od, uploader.upload(table), *rule)
    torch.cuda.synchronize()
    for buf in (kbuf, xbuf, obuf):
        assert _intact(buf)
    assert torch.equal(kd.cpu(), torch.tensor(keys, dtype=torch.int32))
    assert alias or torch.equal(_bits(xd.cpu()), _bits(x))
    return od.cpu()


def _named(rows, keys):
    return {(slot, keys[key0 + j]) for slot, nW, key0, NC in rows for j in range(NC) if 0 <= keys[key0 + j] < CAP}


def _step(cells, rows, keys, x, rule, uploader, alias=False):
    """one call on the device and on a clone of the model; out and the state compared bit for bit; the cells adopt the model -> out"""
    model = cells.clone()
    want = model.model(rows, keys, x, rule)
    got = _launch(cells, rows, keys, x, rule, uploader, alias)
    assert torch.equal(_bits(got), _bits(want))
    cells.adopt(model)
    cells.check()
    return got


def _case(rows, keys, rule, M=6, seed=0, all_stale=False, gated=True, alias=False, **scores):
    """one call over cells made for it; everything compared; the reference shows what every case must -> (the cells afterwards, out, the
    scores, the cells before)"""
    from clip_fsar_amd import baseline_hip as bh
    x = _scores(rows, keys, seed, **scores)
    cells = _Cells(_named(rows, keys), rule, seed, M, all_stale)
    start = cells.clone()
    got = _step(cells, rows, keys, x, rule, bh.table_uploader(DEV, M), alias)
    cells.shows(rule, gated)
    return cells, got, x, start


def _perm(seed):
    return torch.randperm(CAP, generator=torch.Generator().manual_seed(seed)).tolist()


@pytest.mark.parametrize("NC", [1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1])
def test_widths_at_the_workgroup_edges_and_every_window_count(NC):
    """five sessions of one width, each with a list of its own, through launches of 0, 1, 2, 7 and 12 windows over the same cells: the
    case is the sequence, its 22 windows hold the plateaus (one in the launch of 7, one in the launch of 12) the reference must show"""
    from clip_fsar_amd import baseline_hip as bh
    rule = _base()
    keys = _perm(NC)
    rows = lambda nW: [(slot, nW, key0, NC) for slot, key0 in zip((3, 0, 5, 1, 4), (0, 17, 40, 86, 87))]
    cells = _Cells(_named(rows(1), keys), rule, NC, 6)
    up = bh.table_uploader(DEV, 6)
    for nW in (0, 1, 2, 7, 12):
        before = cells.clone()
        _step(cells, rows(nW), keys, _scores(rows(nW), keys, 100 * NC + nW, plateau=(2, 6) if nW >= 7 else (0, 0)), rule, up)
        if nW == 0:                                # no windows: nothing is launched, nothing moves
            for n in STATE:
                assert torch.equal(_bits(getattr(cells, n)), _bits(getattr(before, n))), n
    cells.shows(rule)


def test_three_hundred_rows_of_one_column():
    keys = _perm(3)
    rows = [(slot, 12 if slot % 7 else 0, (slot * 13) % CAP, 1) for slot in range(300)]
    _case(rows, keys, _base(), M=300)


GEOMETRY = [(5, 0, CHUNK + 1), (0, 0, CHUNK + 1), (2, 45, CHUNK - 1), (4, 299, 1), (1, 87, 2 * CHUNK + 1)]   # (slot, key0, NC)


def test_shared_and_overlapping_lists_and_windows_cut_into_calls():
    """two sessions share one list, a third one's starts and ends inside it, over different slots; the same 12 windows in one call, as
    twelve calls of one and as 5 + 0 + 7 give the same deviations and one final state"""
    from clip_fsar_amd import baseline_hip as bh
    rule = _base()
    keys = _perm(14)
    rows = lambda n: [(slot, n, key0, NC) for slot, key0, NC in GEOMETRY]
    cells, whole, x, start = _case(rows(12), keys, rule, seed=14)
    blocks, at = [], 0
    for _, _, NC in GEOMETRY:
        blocks.append((at, x[at:at + 12 * NC].view(12, NC)))
        at += 12 * NC
    up = bh.table_uploader(DEV, 6)
    for cuts in ([1] * 12, [5, 0, 7]):
        replay, k0 = start.clone(), 0
        for n in cuts:
            xs = torch.cat([b[k0:k0 + n].reshape(-1) for _, b in blocks])
            got = _step(replay, rows(n), keys, xs, rule, up)
            o = 0
            for (at, b), (_, _, NC) in zip(blocks, GEOMETRY):          # the piece's deviations are the single call's
                assert torch.equal(_bits(got[o:o + n * NC]), _bits(whole[at + k0 * NC:at + (k0 + n) * NC])), (cuts, k0)
                o += n * NC
            k0 += n
        for name in STATE:
            assert torch.equal(_bits(getattr(replay, name)), _bits(getattr(cells, name))), (cuts, name)


def test_a_generation_bumped_between_two_calls_restarts_warm_up():
    from clip_fsar_amd import baseline_hip as bh
    rule = _base()
    keys = _perm(15)
    rows = [(slot, 7, key0, NC) for slot, key0, NC in GEOMETRY[:3]]
    cells, _, _, _ = _case(rows, keys, rule, seed=15, plateau=(2, 5))       # 7 windows: the pairs that start warm show the plateau
    named = sorted(_named(rows, keys))
    assert all(int(cells.count[s, k]) == rule.warmup for s, k in named)            # 7 windows: every pair is past warm-up
    bumped = sorted({k for _, k in named[::2]})
    assert len(bumped) > 20
    for k in bumped:
        cells.gens[k] += 1
    cells.device["gens"][1].copy_(cells.gens)
    x = _scores(rows, keys, 77, plateau=(0, 0))
    got = _step(cells, rows, keys, x, rule, bh.table_uploader(DEV, 6))
    at = 0
    for slot, nW, key0, NC in rows:
        z = got[at:at + nW * NC].view(nW, NC)
        at += nW * NC
        for j in range(NC):
            fresh = keys[key0 + j] in bumped
            assert bool(z[:rule.warmup, j].isnan().all()) == fresh and not bool(z[rule.warmup:, j].isnan().any()), (slot, j)
    assert all(int(cells.marks[s, k]) == int(cells.gens[k]) and int(cells.count[s, k]) == rule.warmup for s, k in named)


@pytest.mark.parametrize("bad", [-1, CAP, 1 << 30])
def test_a_key_out_of_range_gives_a_nan_column_and_writes_no_state(bad):
    keys = _perm(13)
    for j in (0, 7, CHUNK - 1, CHUNK, 298):
        keys[j] = bad
    _, got, _, _ = _case([(2, 7, 0, CHUNK + 1), (4, 12, 200, 100), (0, 0, 0, 8)], keys, _base(), seed=13)
    z = got[:7 * (CHUNK + 1)].view(7, CHUNK + 1)
    assert all(bool(z[:, j].isnan().all()) for j in (0, 7, CHUNK - 1, CHUNK))
    from clip_fsar_amd import baseline_hip as bh
    keys = [bad] + _perm(2)                        # a launch of nothing but such a column
    cells = _Cells(set(), _base(), 1, 6)
    assert bool(_step(cells, [(2, 3, 0, 1)], keys[:8], _scores([(2, 3, 0, 1)], keys, 1), _base(), bh.table_uploader(DEV, 6)).isnan().all())


def test_non_finite_scores_before_and_after_warm_up():
    """a tenth of the scores NaN, a twentieth each +inf and -inf, over cells that all start anew: such a window gets NaN and leaves its
    cell alone, whether the pair has seen nothing yet, is warming up or is warm"""
    from clip_fsar_amd.baseline import reference_baseline
    rule = _base()
    keys = _perm(16)
    rows = [(1, 12, 3, CHUNK + 1)]
    _, got, x, _ = _case(rows, keys, rule, seed=16, all_stale=True, bad=0.1)
    phases, kinds = set(), set()
    for col in x.view(12, CHUNK + 1).t().tolist():
        for k, s in enumerate(col):
            if s != s or s in (INF, -INF):
                n = reference_baseline(col[:k], rule)[1].n
                phases.add(0 if n == 0 else 1 if n < rule.warmup else 2)
                kinds.add(str(s))
    assert phases == {0, 1, 2} and kinds == {"nan", "inf", "-inf"}
    assert torch.equal(got.isnan() & ~x.isfinite(), ~x.isfinite())


def test_warmup_of_one():
    rule = _base(warmup=1)
    _, got, _, _ = _case([(slot, 12, key0, NC) for slot, key0, NC in GEOMETRY[:3]], _perm(17), rule, seed=17, all_stale=True)
    z = got[:12 * (CHUNK + 1)].view(12, CHUNK + 1)
    assert bool(z[0].isnan().all()) and not bool(z[1:].isnan().any())             # the first window sets the mean, the second is judged


def test_a_gate_of_infinity_folds_every_window_in():
    from clip_fsar_amd.baseline import reference_baseline
    rule = _base(gate=INF)
    rows = [(slot, 12, key0, NC) for slot, key0, NC in GEOMETRY[:3]]
    _, got, x, _ = _case(rows, _perm(18), rule, seed=18, gated=False)
    col = x[:12 * (CHUNK + 1)].view(12, CHUNK + 1)[:, 0].tolist()                  # and the plateau erases itself, as the gate is there to prevent
    open_gate, closed = reference_baseline(col, rule)[0], reference_baseline(col, _base())[0]
    assert open_gate[8] < closed[8] - 2.0


def test_out_may_be_scores():
    rows = [(slot, 12, key0, NC) for slot, key0, NC in GEOMETRY]
    _, aliased, _, _ = _case(rows, _perm(19), _base(), seed=19, alias=True)
    _, apart, _, _ = _case(rows, _perm(19), _base(), seed=19)
    assert torch.equal(_bits(aliased), _bits(apart))


def test_two_identical_runs_give_identical_bytes():
    from clip_fsar_amd import baseline_hip as bh
    rule = _base()
    keys = _perm(20)
    rows = [(slot, 12, key0, NC) for slot, key0, NC in GEOMETRY] + [(3, 12, 9, 1)]
    x = _scores(rows, keys, 1)
    runs = []
    for _ in range(2):
        cells = _Cells(_named(rows, keys), rule, 5, 6)
        out = _launch(cells, rows, keys, x, rule, bh.table_uploader(DEV, 6))
        runs.append([_bits(out)] + [_bits(cells.device[k][1].cpu()) for k in STATE])
    assert all(torch.equal(a, b) for a, b in zip(*runs)) and not bool(runs[0][0].eq(_bits(torch.tensor([-99.0]))).any())


# ------------------------------------------------------------------ 2: the pool
IDS = [1, 2, 3, 4, 7, 9]
STRIDE, MAX_PUSH, ALPHA = 1, 6, 0.5


def _feats(n, E, seed):
    return torch.randn(n, E, generator=torch.Generator().manual_seed(seed)).to(DEV)


def _gallery(kind, capacity=6, seed=5, aligned=False):
    """test_gpu_events': a LiveGallery, or a COMBINE LiveTextGallery, holding the classes IDS in a store that is full at 6.  aligned: a
    class's text row is the mean of its shot's tower rows -- text and video of a class agree, as CLIP's towers make them; the synthetic
    head's TEST.CLASS_NAME rows are independent of any video, and the text term of COMBINE then hides the class's own shot"""
    if kind == "live":
        live = _pair(capacity=capacity)[1]
    else:
        from test_gpu_live_text import _galleries
        live = _galleries("fp32", "combine", capacity=capacity)[1]
    shots = _feats(len(IDS) * T, live.E, seed).view(len(IDS), T, live.E)
    live.add_classes_features(shots, IDS, text={c: shots[i].mean(0) for i, c in enumerate(IDS)} if aligned else None)
    assert live.class_ids == IDS
    return live


def _pool(live, smooth, base, rule, stride=STRIDE, max_push=MAX_PUSH):
    from clip_fsar_amd.pool import StreamPool
    return StreamPool(live, max_streams=4, stride=stride, max_push=max_push, smooth=smooth, smooth_by="class", events=rule, baseline=base)


class _Pairs:
    """The reference over what a pool WITHOUT the option returned: per (session key, class id) a baseline cell and, behind it, the
    rule's cell, both restarted where the contract restarts a pair -- the session's open() / reset(), the class's registration, the class
    joining the session's list -- and advanced over the pair's column of every push in order."""

    def __init__(self, base, rule):
        self.base, self.rule, self.cells, self.ev_cells, self.events, self.z = base, rule, {}, {}, [], []

    def forget(self, session=None, cid=None):
        for cells in (self.cells, self.ev_cells):
            for key in [k for k in cells if (session is None or k[0] == session) and (cid is None or k[1] == cid)]:
                del cells[key]

    def saw(self, first_window, scores, ids_of):
        """first_window, scores: {session: its first window, its [nW, C] scores} of one push, in push order; ids_of: session -> its
        columns' class ids -> {session: the deviations [nW, C]}.  Events in take_events' order: sessions as pushed, window, column."""
        from clip_fsar_amd.baseline import reference_baseline
        from clip_fsar_amd.events import Event, reference_events
        out = {}
        for h, s in scores.items():
            z = torch.empty_like(s)
            mine = []
            if not s.shape[0]:                     # no window: the pair's cells are not even made
                out[h] = z
                continue
            for j, (cid, col) in enumerate(zip(ids_of[h], s.t().tolist())):
                zs, self.cells[(h, cid)] = reference_baseline(col, self.base, self.cells.get((h, cid)))
                z[:, j] = torch.tensor(zs, dtype=torch.float32)
                recs, self.ev_cells[(h, cid)] = reference_events(zs, self.rule, self.ev_cells.get((h, cid)))
                for r in recs:
                    w = first_window[h] + r.k
                    start = w - self.rule.min_on + 1 if r.kind == 1 else w - self.rule.min_off - r.len + 1
                    mine.append((w, j, Event(h, cid, "onset" if r.kind == 1 else "offset", w, start, r.len, r.score, r.peak)))
            self.events += [e for _, _, e in sorted(mine, key=lambda t: t[:2])]
            out[h] = z
        return out

    def active(self, h, ids):
        return [(c, self.ev_cells[(h, c)].length, self.ev_cells[(h, c)].peak) for c in ids
                if (h, c) in self.ev_cells and self.ev_cells[(h, c)].streak < 0]

    def baseline(self, h, ids):
        return [(c,) + tuple(self.cells[(h, c)]) for c in ids if (h, c) in self.cells]


def _same_cells(got, want):
    """[(class id, mean, dev, n)] bit for bit (the pool's floats went through fp32 tensors, the reference's are fp32 values)"""
    assert [(c, n) for c, _, _, n in got] == [(c, n) for c, _, _, n in want]
    assert torch.equal(_bits(torch.tensor([g[1:3] for g in got], dtype=torch.float32)),
                       _bits(torch.tensor([w[1:3] for w in want], dtype=torch.float32)))


def _schedule(live, pool, pairs=None, plain=None, taken=None):
    """test_gpu_events' membership schedule.  Without pairs: a pool without the option, -> the scores of every push, per session (what a
    rule would judge: the smoothed scores when the pool smooths).  With pairs: the pool with the option, checked push by push against
    the reference over `plain`, the scores the first pool returned."""
    from clip_fsar_amd import pool as pm
    from clip_fsar_amd.stream import StreamOutput
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
        scores = {h: (out[h].logits if out[h].smoothed is None else out[h].smoothed).cpu() for h in feats}
        seen.append(scores)
        if pairs is None:
            assert all(type(o) is StreamOutput for o in out.values())             # a pool without the option: the plain types
            return out
        want = plain[tick[0] - 1]
        assert list(scores) == list(want) and all(torch.equal(_bits(scores[h]), _bits(want[h])) for h in feats), tick[0]
        z = pairs.saw({h: out[h].first_window for h in feats}, want, {h: ids_of(h) for h in feats})
        for h in feats:
            assert type(out[h]) is pm.DeviationStreamOutput and out[h].deviation.shape == out[h].logits.shape
            assert torch.equal(_bits(out[h].deviation.cpu()), _bits(z[h])), (tick[0], h)
            pairs.z.append(z[h].reshape(-1))
        if take:                                   # some pushes are taken at once, the others wait in the queue
            taken.extend(pool.take_events())
        for h in feats:
            assert pool.active(h) == pairs.active(h, ids_of(h)), (tick[0], h)
            _same_cells(pool.baseline(h), pairs.baseline(h, ids_of(h)))
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
    live.add_shots_features(_feats(T, E, 71).view(1, T, E), [9])      # further shots: the prototype moves, the baseline stays
    push((1, 3, 4))
    slot = live.slot_of(3)
    live.remove_classes([3])
    new_class(11, 72)
    assert live.slot_of(11) == slot                                   # 11, in the freed slot, starts its warm-up
    push((7, 1, 2), take=True)
    if pairs is not None:
        assert 11 in [c for c, _, _, _ in pool.baseline(a)] and 3 not in [c for c, _, _, _ in pool.baseline(a)]
    pool.reset(b)
    if pairs is not None:
        pairs.forget(session=b)
        assert pool.baseline(b) == []
    push((2, 9, 2))
    push((13, 1, 0))                                                  # beyond max_push: three rounds, one call
    pool.close(c)
    d = pool.open(classes=[7, 11, 4])                                 # into c's slot
    assert pool._sessions[d].slot == 2
    if pairs is not None:
        assert pool.baseline(d) == []                                 # nothing of the slot's previous owner is read
    hs["c"] = d
    push((3, 0, 12), take=True)
    push((6, 5, 4))
    assert live.class_ids == [1, 2, 4, 7, 9, 15, 16, 11]
    return seen


@pytest.mark.parametrize("kind,smooth", [("live", 0.0), ("live", ALPHA), ("combine", 0.0), ("combine", ALPHA)])
def test_the_pool_reports_the_reference_deviations_and_events(kind, smooth):
    """a rule low enough (on 1, off 0, in deviations) that random features set it off: the events and the running ones are the
    reference's over the deviations, the deviations and the cells the reference's over the scores of a pool without the option"""
    from clip_fsar_amd.events import EventRule
    base, rule = _base(rate=1 / 8), EventRule(1.0, 0.0, 2, 1)
    with torch.no_grad():                          # the schedule changes its gallery: each pool runs it over a gallery of its own, built alike
        live = _gallery(kind)
        plain = _schedule(live, _pool(live, smooth, None, None))
    pairs, taken = _Pairs(base, rule), []
    with torch.no_grad():
        live = _gallery(kind)
        pool = _pool(live, smooth, base, rule)
        _schedule(live, pool, pairs, plain, taken)
        taken.extend(pool.take_events())
    z = torch.cat(pairs.z)
    kinds = [e.kind for e in pairs.events]
    print("deviations: %d, NaN %d, >= gate %d; onsets %d, offsets %d" % (z.numel(), int(z.isnan().sum()), int((z >= base.gate).sum()),
                                                                        kinds.count("onset"), kinds.count("offset")))
    assert int(z.isnan().sum()) and int((~z.isnan()).sum()) > z.numel() // 3      # warm-ups, restarts included, and deviations proper
    assert kinds.count("onset") >= 1 and kinds.count("offset") >= 1
    assert taken == pairs.events
    assert pool.take_events() == [] and pool.stats()["events"] == len(taken) and pool.stats()["events_dropped"] == 0


STORY_SEED = 1100                                 # of the story's random windows


def _story(live, pool, hot, quiet=10, plateau=4, seed=STORY_SEED):
    """one session, windows that do not overlap (stride T): `quiet` windows of random features, `plateau` windows that are class `hot`'s
    own shot, `quiet` random ones, a blip of 2, `quiet` random ones -> [(first window, scores [nW, C], the push's output)] per push"""
    E = live.E
    shot = _feats(len(IDS) * T, E, 5).view(len(IDS), T, E)[IDS.index(hot)]         # _gallery's seed: the features class `hot` was made of
    h = pool.open()
    pushes = []
    for n, own in ((quiet, False), (plateau, True), (quiet, False), (2, True), (quiet, False)):
        for _ in range(n):
            seed += 1
            out = pool.push_features({h: shot if own else _feats(T, E, seed)})[h]
            pushes.append((out.first_window, (out.logits if out.smoothed is None else out.smoothed).cpu(), out))
    return h, pushes


def test_one_rule_in_deviation_units_serves_both_galleries():
    """EventRule(4, 2, 2, 2) and one Baseline, the same objects, on OTAM logits and on COMBINE probabilities, whose raw scales differ:
    asserted first on the reference alone (over the scores of pools without the option) that the deviations of each gallery show the
    onset and the offset of the class whose shot was played, and that the same rule on the raw scores finds nothing; then the pools
    with the option report exactly those events"""
    from clip_fsar_amd.events import reference_events
    base, rule = _base(warmup=8), _event_rule()
    hot, col = 4, IDS.index(4)
    raw_kinds, scales = {}, {}
    for kind in ("live", "combine"):
        with torch.no_grad():
            live = _gallery(kind, aligned=True)
            _, plain = _story(live, _pool(live, 0.0, None, None, stride=T, max_push=T), hot)
        raw = torch.cat([s for _, s, _ in plain])
        scales[kind] = float(raw.abs().median())
        raw_kinds[kind] = {r.kind for c in raw.t().tolist() for r in reference_events(c, rule)[0]}
        pairs = _Pairs(base, rule)
        z = torch.cat([pairs.saw({0: w}, {0: s}, {0: IDS})[0] for w, s, _ in plain])
        mine = [e for e in pairs.events if e.class_id == hot]
        print(kind, "raw median |score| %.4g" % scales[kind], "z of the played class:", [round(v, 1) for v in z[:, col].tolist()])
        assert [e.kind for e in mine] == ["onset", "offset", "onset", "offset"], mine          # the reference alone, first
        assert [e.window for e in mine] == [11, 15, 25, 27]
        with torch.no_grad():
            live = _gallery(kind, aligned=True)
            pool = _pool(live, 0.0, base, rule, stride=T, max_push=T)
            h, got = _story(live, pool, hot)
            events = pool.take_events()
        assert all(torch.equal(_bits(s), _bits(p)) for (_, s, _), (_, p, _) in zip(got, plain))
        assert torch.equal(_bits(torch.cat([o.deviation.cpu() for _, _, o in got])), _bits(z))
        assert events == pairs.events and pool.active(h) == []
        _same_cells(pool.baseline(h), pairs.baseline(0, IDS))
    assert not raw_kinds["live"] or not raw_kinds["combine"], raw_kinds               # the rule means nothing on (one of) the raw scales
    assert max(scales.values()) > 20 * min(scales.values()), scales                 # which differ
