"""GPU: the contest (clip_fsar_amd.pool.StreamPool(events=..., contest=Contest(...)) on libclipfsar_contest.so) -- the kernel through its
binding, the demoted plane's bits, leaders and n_leaders against clip_fsar_amd.contest.reference_contest, bit for bit and without a
tolerance: at the workgroup edges and every window count, every top and margin, ties on every threshold, rows that exercise each radix
pass, special values, all-equal rows, keys out of range, no keys at all, the grouped layout, 300 rows of one column, and twice for
identical bytes; then the pool: outputs bit-equal to the pool without the option, take_events() and active() against reference_events
over reference_contest of the judged planes the same pushes returned, Contest(top=len(g)) against the pool without the option, the same
frames cut into different pushes, and leaders(out) -- over a LiveGallery with per-class smoothing, a COMBINE LiveTextGallery, a pool with
baseline=, a pool with shortlist= and a pool with rates=(1, 2)."""
import numpy as np
import pytest
import torch

from test_gpu_events import MAX_PUSH, STRIDE, _Pairs, _feats, _gallery, _schedule
from test_gpu_live import DEV, T

pytestmark = pytest.mark.gpu

PAD, NAN, INF = 37, float("nan"), float("inf")
FMAX = float(np.finfo(np.float32).max)
F_SENTINEL, I_SENTINEL = -12345.0, -77
NONE = 0x7FFFFFFF
CAP = 600                                         # store slots of the kernel tests
MARGINS = [None, 0.0, 0.25, FMAX]


# ------------------------------------------------------------------ 1: the kernel, through the binding
def _padded(t):
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


def _table(rows):
    """rows: (nW, key0, NC) per table row -> the descriptor table and NOUT"""
    table, n_out, chunks = [], 0, 0
    for r, (nW, key0, NC) in enumerate(rows):
        table.append([r, nW, n_out, NC, key0, chunks])
        n_out += nW * NC
        chunks += -(-NC // 256)
    return table, n_out


def _reference(rows, keys, x, top, margin):
    """reference_contest block by block -> (out flat fp32, leaders [sum NW, top], n_leaders, and what the case shows: demoted cells,
    leaders, and cells that equal a row's lowest leader without being kept)"""
    from clip_fsar_amd.contest import leaders_table, reference_contest, score_keys
    outs, lists, at = [], [], 0
    shown = {"demoted": 0, "leaders": 0, "ties": 0}
    for nW, key0, NC in rows:
        blk = x[at:at + nW * NC].view(nW, NC).numpy()
        at += nW * NC
        mine = None if keys is None else keys[key0:key0 + NC]
        out, lead = reference_contest(blk, mine, CAP, top, margin)
        outs.append(torch.from_numpy(out).reshape(-1))
        lists += lead
        valid = None if mine is None else [0 <= k < CAP for k in mine]
        for row, o, l in zip(blk, out, lead):
            shown["demoted"] += int((np.isneginf(o) & ~np.isneginf(row)).sum())
            shown["leaders"] += len(l)
            if l:
                key = score_keys(row, valid)
                low = min(int(key[j]) for j in l)
                shown["ties"] += int((key == low).sum()) - sum(int(key[j]) == low for j in l)
    table, counts = leaders_table(lists, top)
    return torch.cat(outs) if outs else torch.zeros(0), torch.from_numpy(table), torch.from_numpy(counts), shown


def _launch(rows, keys, x, top, margin, with_leaders=True, out_fill=F_SENTINEL):
    """one cfct_contest; every buffer lies between sentinels, which must survive, and scores, keys and the table come back unchanged ->
    (out, leaders, n_leaders) on the host (None, None without leader lists)"""
    from clip_fsar_amd import contest_hip as ch
    table, n_out = _table(rows)
    assert n_out == x.numel()
    n_rows = sum(nW for nW, _, _ in rows)
    xbuf, xd = _padded(x)
    kbuf, kd = (None, None) if keys is None else _padded(torch.tensor(keys, dtype=torch.int32))
    obuf, od = _padded(torch.full((n_out,), out_fill))
    lbuf, ld = _padded(torch.full((n_rows, top), -99, dtype=torch.int32))
    nbuf, nd = _padded(torch.full((n_rows,), -99, dtype=torch.int32))
    wbuf, wd = _padded(torch.full((ch.workspace_words(n_out),), -99, dtype=torch.int32))
    t = ch.table_uploader(DEV, max(len(rows), 1)).upload(table)
    ch.contest(xd, kd, od, ld if with_leaders else None, nd if with_leaders else None, wd, t, CAP, top, margin)
    torch.cuda.synchronize()
    for buf in (xbuf, kbuf, obuf, lbuf, nbuf, wbuf):
        assert buf is None or _intact(buf)
    assert torch.equal(_bits(xd.cpu()), _bits(x)) and (keys is None or kd.cpu().tolist() == list(keys))
    assert t.host.tolist() == table and t.dev.cpu().tolist() == table
    if not with_leaders:
        assert bool((ld == -99).all()) and bool((nd == -99).all())
        return od.cpu(), None, None
    return od.cpu(), ld.cpu(), nd.cpu()


def _quantised(n, seed):
    """seven values: ties on every threshold"""
    return (torch.randint(0, 7, (n,), generator=torch.Generator().manual_seed(seed)).float() - 3) / 4


def _case(rows, keys, top, margin, scores=_quantised, need=("demoted", "leaders"), seed0=0, with_leaders=True):
    """Build a case whose reference alone shows what `need` names (the first seed that does: the inputs are chosen on the model, the
    kernel is not asked), run it once and compare everything"""
    n = sum(nW * NC for nW, _, NC in rows)
    for seed in range(seed0, seed0 + 200):
        x = scores(n, seed)
        want = _reference(rows, keys, x, top, margin)
        if all(want[3][k] > 0 for k in need):
            break
    assert all(want[3][k] > 0 for k in need), (need, want[3])          # no case is vacuous
    out, leaders, n_leaders = _launch(rows, keys, x, top, margin, with_leaders)
    assert torch.equal(_bits(out), _bits(want[0]))
    if with_leaders:
        assert torch.equal(n_leaders, want[2]) and torch.equal(leaders, want[1])
    return x, want


def _perm(n, seed):
    return torch.randperm(CAP, generator=torch.Generator().manual_seed(seed))[:n].tolist()


def _tops(NC):
    return sorted({t for t in (1, 2, NC - 1, NC, NC + 5) if t >= 1})


def _needs(NC, top, margin, ties=True):
    """what a configuration can show at all: a row of one column, or top >= NC without a margin that bites, demotes nothing; a tie at
    the threshold needs top < NC"""
    need = ["leaders"]
    if NC > 1 and (top < NC or margin in (0.0, 0.25)):
        need.append("demoted")
    if ties and NC > 2 and top < NC and margin is None:
        need.append("ties")
    return need


@pytest.mark.parametrize("NC", [1, 63, 64, 65, 255, 256, 257, 513, 1025])
def test_widths_at_the_workgroup_edges_every_window_count_top_and_margin(NC):
    """four sessions of one width, with 0, 1, 2 and 7 windows and a key list each, per launch"""
    keys = _perm(CAP, NC) + _perm(CAP, NC + 1)                 # 1 200 keys: a list may name a slot twice, the contest keeps no state
    rows = [(nW, key0, NC) for nW, key0 in zip((0, 1, 2, 7), (0, 17, 40, 86))]
    for top in _tops(NC):
        for margin in MARGINS:
            _case(rows, keys, top, margin, need=_needs(NC, top, margin), seed0=NC + top)


def _byte_rows(which):
    def scores(n, seed):
        g = torch.Generator().manual_seed(seed)
        b = torch.randint(0, 256, (n,), generator=g, dtype=torch.int64)
        if which == "low":                         # one sign, exponent and upper mantissa: the first three passes see one value
            u = 0x3F800000 | b
        elif which == "high":                      # every sign and exponent over one mantissa (no NaN, no infinity: the mantissa's top bit is 0)
            u = (b << 24) | 0x00123456
        else:                                      # the second and the third byte
            u = 0x3F000000 | (b << (16 if which == "second" else 8)) | 0x55
        return torch.from_numpy(u.numpy().astype(np.uint32).view(np.float32))
    return scores


@pytest.mark.parametrize("which", ["low", "second", "third", "high"])
def test_rows_whose_keys_differ_in_one_byte_only(which):
    """each radix pass decides alone; 300 columns over 256 byte values: ties at the threshold"""
    rows = [(3, 0, 300), (2, 100, 257)]
    keys = _perm(CAP, 3)
    for top in (1, 7, 150, 299):
        for margin in (None, 0.0) if which != "high" else (None, 0.0, FMAX):
            x, _ = _case(rows, keys, top, margin, scores=_byte_rows(which), need=["demoted", "leaders"] + (["ties"] if margin is None else []))
    assert bool(torch.isfinite(x).all()) and (which != "high" or (bool((x < 0).any()) and bool((x.abs() < 1e-38).any())))


SPECIALS = [0.0, -0.0, INF, -INF, NAN, 1e-45, -1e-45, 1e-39, -1e-39, FMAX, -FMAX]


def _sprinkled(n, seed):
    g = torch.Generator().manual_seed(seed)
    x = _quantised(n, seed)
    at = torch.rand(n, generator=g) < 0.3
    pick = torch.tensor(SPECIALS)[torch.randint(0, len(SPECIALS), (n,), generator=g)]
    return torch.where(at, pick, x)


@pytest.mark.parametrize("margin", MARGINS + [1e-39])
def test_special_values_sprinkled_in(margin):
    rows = [(7, 0, 257), (2, 9, 64), (1, 300, 5)]
    keys = _perm(CAP, 4)
    for top in (1, 3, 40, 200):
        x, want = _case(rows, keys, top, margin, scores=_sprinkled, need=["demoted", "leaders"] + (["ties"] if margin is None else []))
    src = _bits(x)
    assert all(bool((src == _bits(torch.tensor([v]))[0]).any()) for v in SPECIALS)             # every special value took part
    nan = torch.isnan(x)
    assert bool(torch.isnan(want[0])[nan].all()) and not bool(torch.isnan(want[0])[~nan].any())    # a NaN never disappears, none appears


def test_all_equal_rows():
    rows = [(2, 0, 513), (1, 5, 1), (3, 7, 256)]
    keys = _perm(CAP, 5)
    for value in (0.5, 0.0, -0.0, -FMAX, INF, 1e-45):
        for top in (1, 2, 255, 256, 600):
            for margin in (None, 0.0):
                _, want = _case(rows, keys, top, margin, scores=lambda n, seed: torch.full((n,), value),
                                need=["leaders"] + (["demoted", "ties"] if top < 513 else []))
                assert want[2].tolist() == [min(top, 513)] * 2 + [1] + [min(top, 256)] * 3        # the lowest columns, top of them
    for value in (NAN, -INF):                      # no candidate: the plane is the input, no leader
        _, want = _case(rows, keys, 2, 0.0, scores=lambda n, seed: torch.full((n,), value), need=[])
        assert want[3] == {"demoted": 0, "leaders": 0, "ties": 0}


@pytest.mark.parametrize("bad", [-1, CAP, NONE])
def test_a_key_out_of_range_is_copied_and_never_leads(bad):
    keys = _perm(CAP, 6)
    spoiled = (0, 7, 255, 256, 298)
    for j in spoiled:
        keys[j] = bad
    rows = [(7, 0, 257), (2, 200, 100), (0, 0, 8), (3, 298, 1)]        # the last row's one column has no valid key
    for top in (1, 5, 250):                        # (253 of the first row's columns have a valid key)
        for margin in (None, 0.25):
            x, want = _case(rows, keys, top, margin, seed0=3)
            blk, out = x[:7 * 257].view(7, 257), want[0][:7 * 257].view(7, 257)
            assert torch.equal(blk[:, list(spoiled[:4])], out[:, list(spoiled[:4])])              # among them a row's best score
            assert not set(want[1][:7].reshape(-1).tolist()) & set(spoiled[:4]) and want[2][-3:].tolist() == [0, 0, 0]
    best = x[:7 * 257].view(7, 257)
    assert bool((best[:, list(spoiled[:4])].max(1).values == best.max(1).values).any())


def test_without_keys_every_column_competes_and_leader_lists_are_optional():
    rows = [(2, 77, 300), (5, -5, 64), (1, 1 << 30, 1025)]              # KEY0 is ignored
    for top in (1, 64, 2000):
        for margin in MARGINS:
            _case(rows, None, top, margin, need=_needs(64, top, margin))
    _case(rows, None, 3, None, with_leaders=False)
    _case([(7, 0, 257)], _perm(CAP, 8), 3, 0.25, with_leaders=False)


def test_the_grouped_layout_several_widths_in_one_call():
    """table rows of different NC, shared and overlapping key lists, rows without windows in between"""
    keys = _perm(CAP, 9)
    rows = [(3, 0, 257), (0, 0, 257), (2, 45, 255), (7, 299, 1), (1, 87, 513), (12, 0, 2), (2, 17, 64)]
    for top in (1, 2, 64, 300):
        for margin in MARGINS:
            _case(rows, keys, top, margin, need=_needs(513, top, margin), seed0=top)


def test_three_hundred_rows_of_one_column():
    """300 table rows: a window's ordinal is the sum of up to 299 counts before it (more than one pass of the workgroup's 256 threads)"""
    keys = _perm(CAP, 10)
    keys[5] = -1
    rows = [(slot % 4, (slot * 13) % CAP, 1) for slot in range(300)]
    for top, margin in ((1, None), (2, 0.0)):
        x, want = _case(rows, keys, top, margin, scores=_sprinkled, need=["leaders"])
        assert want[1].shape[0] == 450 and 0 < int(want[2].sum()) < 450 and want[3]["demoted"] == 0


def test_two_identical_runs_give_identical_bytes():
    keys = _perm(CAP, 11) + _perm(CAP, 12)
    rows = [(7, 0, 1025), (2, 45, 255), (12, 299, 1), (3, 87, 513)]
    x = _sprinkled(sum(nW * NC for nW, _, NC in rows), 1)
    runs = [_launch(rows, keys, x, 5, 0.25, out_fill=fill) for fill in (F_SENTINEL, 7.0)]         # whatever `out` held before
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(*runs))
    assert int(runs[0][2].sum()) > 24 and bool(torch.isneginf(runs[0][0]).any())


# ------------------------------------------------------------------ 2: the pool
ALPHA = 0.5


def _judged(o):
    """the plane the rule judges: deviation with a baseline, else smoothed with per-class smoothing, else logits"""
    z = getattr(o, "deviation", None)
    return z if z is not None else (o.logits if o.smoothed is None else o.smoothed)


class _Gated(_Pairs):
    """test_gpu_events' reference over what a pool returned, with the contest in front: reference_contest over each session's judged
    plane, reference_events over its columns.  gate: the Contest, or None (the ungated run over the same planes).  A shortlist output's
    columns name the class behind each place; a pair that was not listed at the session's previous scoring push starts anew."""

    def __init__(self, rule, gate):
        super().__init__(rule)
        self.gate, self.leaders, self.tick, self.listed = gate, [], {}, {}

    def saw(self, outs, ids_of):
        from clip_fsar_amd.contest import reference_contest
        from clip_fsar_amd.events import Event, reference_events
        for h, out in outs.items():
            plane = _judged(out).cpu()
            if not plane.shape[0]:
                continue
            ids, keys, cols = list(ids_of[h]), None, None
            if hasattr(out, "columns"):
                cols = out.columns.tolist()
                ids = [ids[c] if c != NONE else None for c in cols]
                keys = [0 if c != NONE else -1 for c in cols]
                self.tick[h] = self.tick.get(h, 0) + 1
                for cid in ids:
                    if cid is not None and self.listed.get((h, cid)) != self.tick[h] - 1:
                        self.cells.pop((h, cid), None)
                    self.listed[(h, cid)] = self.tick[h]
            if self.gate is not None:
                shown, lead = reference_contest(plane, keys, 1, self.gate.top, self.gate.margin)
                self.leaders.append((h, out.first_window, lead if cols is None else [[cols[j] for j in l] for l in lead]))
                plane = torch.from_numpy(shown)
            mine = []
            for j, (cid, col) in enumerate(zip(ids, plane.t().tolist())):
                if cid is None:
                    continue
                recs, self.cells[(h, cid)] = reference_events(col, self.rule, self.cells.get((h, cid)))
                for r in recs:
                    w = out.first_window + r.k
                    start = w - self.rule.min_on + 1 if r.kind == 1 else w - self.rule.min_off - r.len + 1
                    mine.append((w, j, Event(h, cid, "onset" if r.kind == 1 else "offset", w, start, r.len, r.score, r.peak)))
            self.events += [e for _, _, e in sorted(mine, key=lambda t: t[:2])]


class _Both:
    """two models over the same outputs: the gated one answers, the ungated one follows"""

    def __init__(self, main, other):
        self.main, self.other = main, other

    def saw(self, outs, ids_of):
        self.main.saw(outs, ids_of)
        self.other.saw(outs, ids_of)

    def forget(self, **kw):
        self.main.forget(**kw)
        self.other.forget(**kw)

    def active(self, h, ids):
        return self.main.active(h, ids)


def _make(config, rule=None, contest=None):
    """a gallery and a pool of one of the configurations; each pool runs over a gallery of its own, built alike"""
    from clip_fsar_amd.baseline import Baseline
    from clip_fsar_amd.pool import StreamPool
    from clip_fsar_amd.shortlist import Shortlist
    live = _gallery("combine" if config == "combine" else "live")
    kw = dict(max_streams=4, stride=STRIDE, max_push=MAX_PUSH, events=rule)
    if contest is not None:
        kw["contest"] = contest
    if config == "live":
        kw.update(smooth=ALPHA, smooth_by="class")
    elif config == "baseline":
        kw.update(smooth=ALPHA, smooth_by="class", baseline=Baseline(rate=0.25, warm_rate=0.5, warmup=2, gate=3.0))
    elif config == "shortlist":
        kw.update(smooth=ALPHA, smooth_by="class", shortlist=Shortlist(live, keep=3), shortlist_hold=1)
    elif config == "rates":
        kw.update(rates=(1, 2))
    return live, StreamPool(live, **kw)


CUTS = [(5, 7, 4), (3, 0, 6), (6, 2, 1), (1, 4, 0), (2, 6, 5), (9, 1, 2), (4, 3, 6)]            # frames per push of three sessions
RECUT = [(8, 7, 10), (6, 6, 1), (3, 0, 0), (13, 10, 13)]                                         # the same 30 / 23 / 24 frames


def _steady(live, pool, pairs=None, taken=None, cuts=CUTS):
    """three sessions over every class, each fed its own fixed stream of frames cut into pushes as `cuts` says (a push beyond max_push:
    several rounds); with pairs: the model follows"""
    hs = [pool.open() for _ in range(3)]
    total = [sum(c[i] for c in cuts) for i in range(3)]
    streams = [_feats(n, live.E, 900 + i) for i, n in enumerate(total)]
    done = [0, 0, 0]
    for k, counts in enumerate(cuts):
        feats = {hs[i]: streams[i][done[i]:done[i] + n] for i, n in enumerate(counts) if n}
        for i, n in enumerate(counts):
            done[i] += n
        out = pool.push_features(feats)
        if pairs is not None:
            pairs.saw(out, {h: list(live.class_ids) for h in feats})
            if k % 3 == 1:
                taken.extend(pool.take_events())
            if pool._shortlist is None:            # (a shortlist pool lists the pairs of the last scoring push alone)
                for h in feats:
                    assert pool.active(h) == pairs.active(h, list(live.class_ids)), (k, h)
    assert done == total


def _drive(config, live, pool, pairs=None, taken=None, steady=False):
    if steady or config in ("shortlist", "rates"):                     # open(classes=) and enroll(join=True) are refused there
        return _steady(live, pool, pairs, taken)
    return _schedule(live, pool, pairs, taken)     # test_gpu_events' schedule: class lists on two sessions, enrolment, removals, reset


def _collect(pool):
    """pool.push_features, every output kept"""
    kept, push = [], pool.push_features

    def recorded(feats):
        kept.append(push(feats))
        return kept[-1]
    pool.push_features = recorded
    return kept


PLAIN = {}


def _plain(config, steady=False):
    """the pool WITHOUT a rule over the configuration's pushes, once per configuration: its outputs, and the 0.6 / 0.4 quantiles and the
    spread of the judged scores it returned (NaN, a baseline's warm-up, left out) -- where on, off and a margin sit"""
    key = (config, steady or config in ("shortlist", "rates"))
    if key not in PLAIN:
        with torch.no_grad():
            live, pool = _make(config)
            outs = _collect(pool)
            _drive(config, live, pool, steady=steady)
        scores = torch.cat([_judged(o).reshape(-1) for out in outs for o in out.values()]).cpu()
        scores = scores[~torch.isnan(scores)]
        PLAIN[key] = (outs, float(torch.quantile(scores, 0.6)), float(torch.quantile(scores, 0.4)), float(scores.std()))
    return PLAIN[key]


def _same_outputs(a, b):
    """every tensor of two runs' outputs, bit for bit"""
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert list(x) == list(y)
        for h in x:
            assert x[h].first_window == y[h].first_window and type(x[h]).__name__ == type(y[h]).__name__
            for f in ("logits", "smoothed", "deviation", "tempo", "columns", "pinned"):
                u, v = getattr(x[h], f, None), getattr(y[h], f, None)
                assert (u is None) == (v is None) and (u is None or (u.shape == v.shape and torch.equal(_bits(u), _bits(v)))), (h, f)


def _same_where_listed(a, b):
    """two shortlist pools' outputs.  A pin follows the detector's own cell (an event that runs, a streak that counts), and the detector
    of the pool with the contest sees the demoted plane: an outranked pair's pin lapses, which is the one way the contest reaches a
    later push's lists.  So: every tensor bit for bit while a session's lists have agreed so far, and the exact logit of every
    (window, class) pair both pools list whatever the lists -- a pair's logit does not depend on the other columns."""
    agree, compared, apart = {}, 0, 0
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert list(x) == list(y)
        for h in x:
            assert x[h].first_window == y[h].first_window and x[h].logits.shape == y[h].logits.shape
            same = torch.equal(x[h].columns, y[h].columns) and torch.equal(x[h].pinned, y[h].pinned)
            agree[h] = agree.get(h, True) and same
            apart += not same
            if agree[h]:
                for f in ("logits", "smoothed"):
                    assert torch.equal(_bits(getattr(x[h], f)), _bits(getattr(y[h], f))), (h, f)
            ix, iy = x[h].class_ids(), y[h].class_ids()
            for cid in set(ix) & set(iy) - {None}:
                assert torch.equal(_bits(x[h].logits[:, ix.index(cid)]), _bits(y[h].logits[:, iy.index(cid)])), (h, cid)
                compared += x[h].logits.shape[0]
    assert compared > 100
    return apart


@pytest.mark.parametrize("config,min_on,min_off,top,margin", [("live", 2, 2, 1, False), ("combine", 1, 1, 2, False),
                                                              ("baseline", 2, 1, 1, False), ("shortlist", 1, 2, 1, False),
                                                              ("rates", 2, 2, 2, True), ("live", 1, 2, 3, True)])
def test_the_pool_reports_the_reference_events_over_the_contested_planes(config, min_on, min_off, top, margin):
    """on and off sit at the 0.6 / 0.4 quantiles of what a pool without a rule returned over the same pushes (a margin at half their
    standard deviation); the pool with the contest returns that pool's bits, and its events are reference_events over
    reference_contest of the judged planes"""
    from clip_fsar_amd.contest import Contest
    from clip_fsar_amd.events import EventRule
    plain_outs, on, off, spread = _plain(config)
    rule, gate = EventRule(on, off, min_on, min_off), Contest(top, 0.5 * spread if margin else None)
    pairs, ungated, taken = _Gated(rule, gate), _Gated(rule, None), []
    with torch.no_grad():
        live, pool = _make(config, rule, gate)
        outs = _collect(pool)
        _drive(config, live, pool, _Both(pairs, ungated), taken)
        taken.extend(pool.take_events())
    if config == "shortlist":                                          # 1: nothing but the detector sees the demoted plane
        with torch.no_grad():                      # (the pool with the rule alone: its pins follow its own detector)
            live0, pool0 = _make(config, rule)
            outs0 = _collect(pool0)
            _drive(config, live0, pool0)
        _same_where_listed(outs0, outs)
    else:
        _same_outputs(plain_outs, outs)
    # on the reference alone: the ungated run over the same planes has an onset the gated run lacks, the gated run has one all the
    # same, and an OFFSET whose score is -inf: its class was outranked
    onsets = lambda events: {(e.session, e.class_id, e.window) for e in events if e.kind == "onset"}
    assert onsets(ungated.events) - onsets(pairs.events) and onsets(pairs.events)
    assert any(e.kind == "offset" and e.score == -INF for e in pairs.events)
    assert taken == pairs.events                                       # 2
    assert pool.take_events() == [] and pool.stats()["events"] == len(taken) and pool.stats()["events_dropped"] == 0
    # 5: leaders(out) of every session's output
    shown = [o[h] for o in outs for h in o if _judged(o[h]).shape[0]]
    assert len(shown) == len(pairs.leaders)
    n = 0
    for out, (h, first, lead) in zip(shown, pairs.leaders):
        columns, counts = pool.leaders(out)
        assert out.first_window == first and columns.dtype == counts.dtype == torch.int32 and columns.is_cuda and counts.is_cuda
        assert counts.tolist() == [len(l) for l in lead], (h, first)
        assert columns.tolist() == [l + [NONE] * (gate.top - len(l)) for l in lead], (h, first)
        n += sum(len(l) for l in lead)
    assert n > 20


@pytest.mark.parametrize("config", ["live", "combine", "baseline", "shortlist", "rates"])
def test_top_at_least_the_class_count_is_the_pool_without_the_option(config):
    from clip_fsar_amd.contest import Contest
    from clip_fsar_amd.events import EventRule
    plain_outs, on, off, _ = _plain(config)
    rule = EventRule(on, off, 1, 2)
    runs = []
    for gate in (None, Contest(top=64)):          # more than the classes the schedule ever holds
        with torch.no_grad():
            live, pool = _make(config, rule, gate)
            outs = _collect(pool)
            _drive(config, live, pool)
            assert len(live) <= 64
            runs.append((outs, pool.take_events(), [pool.active(h) for h in pool.sessions]))
    _same_outputs(runs[0][0], runs[1][0])
    if config != "shortlist":                     # (a shortlist pool without a rule pins nothing on a detector's state)
        _same_outputs(plain_outs, runs[1][0])
    kinds = [e.kind for e in runs[0][1]]
    assert kinds.count("onset") >= 3 and kinds.count("offset") >= 1, kinds
    assert repr(runs[0][1]) == repr(runs[1][1]) and repr(runs[0][2]) == repr(runs[1][2])


@pytest.mark.parametrize("config", ["live", "baseline", "rates"])
def test_the_same_frames_cut_into_other_pushes_give_the_same_events(config):
    from clip_fsar_amd.contest import Contest
    from clip_fsar_amd.events import EventRule
    _, on, off, spread = _plain(config, steady=True)
    rule, gate = EventRule(on, off, 2, 2), Contest(2, 0.5 * spread)
    found = []
    for cuts in (CUTS, RECUT):
        with torch.no_grad():
            live, pool = _make(config, rule, gate)
            _steady(live, pool, cuts=cuts)
            found.append(sorted(pool.take_events(), key=lambda e: (e.session, e.class_id, e.window, e.kind)))
    kinds = [e.kind for e in found[0]]
    assert kinds.count("onset") >= 3 and any(e.kind == "offset" and e.score == -INF for e in found[0]), kinds
    assert repr(found[0]) == repr(found[1])


def test_leaders_of_packed_grouped_and_shortlist_outputs():
    """the packed forms: a dense PackedOutput, a GroupedPackedOutput (the index counts in the session's own list) and a shortlist
    pool's (mapped through columns into gallery.class_ids), each against the reference over the output's own planes"""
    from clip_fsar_amd.contest import Contest, leaders_table, reference_contest
    from clip_fsar_amd.events import EventRule
    from clip_fsar_amd.pool import GroupedPackedOutput
    checked = 0
    with torch.no_grad():
        for config in ("live", "shortlist"):
            gate = Contest(2, 0.5 * _plain(config, steady=True)[3])
            live, pool = _make(config, EventRule(0.0, -1.0), gate)
            a, b = pool.open(), pool.open()
            c = pool.open(classes=[9, 2, 4]) if config == "live" else pool.open()
            for members in ([a, b], [a, c, b], [c]):
                counts = [T + 2, 1, T + 4][:len(members)]              # the second session of a push completes no window early on
                po = pool.push_features_packed(_feats(sum(counts), live.E, 40 + len(members)), members, counts)
                assert isinstance(po, GroupedPackedOutput) == (config == "live" and c in members)
                columns, n = pool.leaders(po)
                want = []
                for i, h in enumerate(po.sessions):
                    w0, w1 = po.offsets[i], po.offsets[i + 1]
                    if w1 == w0:
                        continue
                    if isinstance(po, GroupedPackedOutput):
                        plane = _judged(po)[po.logit_offsets[i]:po.logit_offsets[i + 1]].view(w1 - w0, po.widths[i]).cpu()
                    else:
                        plane = _judged(po)[w0:w1].cpu()
                    cols = po.columns[i].tolist() if config == "shortlist" else None
                    keys = None if cols is None else [0 if col != NONE else -1 for col in cols]
                    lead = reference_contest(plane, keys, 1, gate.top, gate.margin)[1]
                    want += lead if cols is None else [[cols[j] for j in l] for l in lead]
                table, counted = leaders_table(want, gate.top)
                assert len(want) == po.offsets[-1] > 0
                assert columns.cpu().tolist() == table.tolist() and n.cpu().tolist() == counted.tolist(), (config, members)
                checked += int(counted.sum())
    assert checked > 20
