"""GPU: the history search (clip_fsar_amd.pool.StreamPool(history=History(...)) on libclipfsar_history.so) -- cfhs_peaks through its
binding against clip_fsar_amd.history.reference_search bit for bit: row lengths at the tile edges mixed in one table, 1, 3 and 64
classes, every separation and top that takes another path, with and without min_score, on planes of eight dyadic values (ties
everywhere) with NaN, both infinities, both zeros and +-FLT_MAX injected, on planes whose scores differ in their low mantissa bytes
alone, on an all-equal plane, between sentinels and twice for identical bytes; then the pool over test_gpu_events' gallery, features
and uneven push counts, with a store three frames longer than the ring and pushes of several rounds: the option changes no output bit
(also with per-class smoothing, events, rates= and still= on pixel pushes), the plane is classify_features of the windows rebuilt on
the host and the pushes' own logits, hits and peaks are the reference's, reset() and a reused slot hide the past, the *_hit methods
read the pushed rows, tempo= reads the frames tempo_positions names, and the cut of the pushes does not matter."""
import numpy as np
import pytest
import torch

from test_gpu_events import IDS, _feats, _gallery, _intact, _padded
from test_gpu_live import DEV, T

pytestmark = pytest.mark.gpu

INF, NAN = float("inf"), float("nan")
FMAX = float(np.finfo(np.float32).max)
NONE = 0x7FFFFFFF
DYADIC = [-1.5, -0.5, 0.0, 0.25, 0.5, 0.75, 1.0, 2.0]
SPECIALS = [NAN, -INF, INF, 0.0, -0.0, FMAX, -FMAX]
LENGTHS = [257, 0, 1, 513, 2, 255, 0, 256]        # every row length of the issue, mixed in one table: 1 284 windows
SEEN = {}                                         # case id -> (suppressed, equal-score suppressions, last-place ties dropped)


def _bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------ 1: the kernels, through the binding
def _dyadic(NW, K, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.tensor(DYADIC)[torch.randint(0, len(DYADIC), (NW, K), generator=g)]
    at = torch.randint(0, NW * K, (max(8, NW * K // 9),), generator=g)
    x.view(-1)[at] = torch.tensor(SPECIALS)[torch.randint(0, len(SPECIALS), at.shape, generator=g)]
    return x


def _keys(plane, floor):
    from clip_fsar_amd.contest import score_keys
    x = plane.numpy()
    with np.errstate(invalid="ignore"):
        return score_keys(x, None if floor is None else x >= np.float32(floor)).astype(np.int64)


def _counts(key, counts, sep, hits, peaks):
    """what a case shows, from the reference's answer: candidates that are no peaks, those of them that no neighbour outscores (an
    equal score at a lower window did it), and peaks equal to the class's last kept one that `top` dropped"""
    beaten, outscored, at = np.zeros(key.shape, dtype=bool), np.zeros(key.shape, dtype=bool), 0
    for n in counts:
        blk = key[at:at + n]
        for d in range(1, min(sep, n - 1) + 1):
            beaten[at + d:at + n] |= blk[:-d] >= blk[d:]
            beaten[at:at + n - d] |= blk[d:] > blk[:-d]
            outscored[at + d:at + n] |= blk[:-d] > blk[d:]
            outscored[at:at + n - d] |= blk[d:] > blk[:-d]
        at += n
    peak = (key != 0) & ~beaten
    assert peak.sum(0).tolist() == peaks
    suppressed = int((key != 0).sum()) - sum(peaks)
    equal = int(((key != 0) & ~outscored).sum()) - sum(peaks)
    dropped = 0
    for k, (rows, n) in enumerate(zip(hits, peaks)):
        if n > len(rows):                          # `top` cut the class: the peaks that share the last kept key and were not kept
            last = key[rows, k].min()
            dropped += int((key[peak[:, k], k] == last).sum()) - int((key[rows, k] == last).sum())
    return suppressed, equal, dropped


def _peak_rows(key, counts, sep, k):
    """the peaks of class k window by window, the rule as it is written"""
    out, at = [], 0
    for n in counts:
        col = key[at:at + n, k]
        for j in np.flatnonzero(col):
            a, b = max(0, j - sep), min(n - 1, j + sep)
            if not (col[a:j] >= col[j]).any() and not (col[j + 1:b + 1] > col[j]).any():
                out.append(at + int(j))
        at += n
    return out


def _peaks_case(name, plane, counts, sep, floor, top):
    """one cfhs_peaks between sentinels, twice, against reference_search -> the reference's (hits, peaks)"""
    from clip_fsar_amd import history_hip as hh
    from clip_fsar_amd import pool_hip as php
    from clip_fsar_amd.history import reference_search
    NW, K = plane.shape
    assert sum(counts) == NW
    rows, off = [], 0
    for i, n in enumerate(counts):
        rows.append([i, 3, 0, 0, 1, n, off, 0])     # SLOT, PUT_POS, N, FEAT_OFF, WIN_POS are the gather's business: never read here
        off += n
    want_hits, want_peaks = reference_search(plane, counts, sep, floor, top)
    key = _keys(plane, floor)
    if NW * K <= 4000:                             # the rule window by window, under the reference's vectorised statement of it
        assert [len(_peak_rows(key, counts, sep, k)) for k in range(K)] == want_peaks
    uploader = php.TableUploader(DEV, len(counts))
    dev_sep = max(0, min(sep, max(counts) - 1))
    runs = []
    for _ in range(2):
        table = uploader.upload(rows)
        sbuf, sd = _padded(plane)
        wbuf, wd = _padded(torch.full((hh.workspace_words(NW, K),), -99, dtype=torch.int32))
        rbuf, rd = _padded(torch.full((K, top), -99, dtype=torch.int32))
        vbuf, vd = _padded(torch.full((K, top), -99.0))
        nbuf, nd = _padded(torch.full((K,), -99, dtype=torch.int32))
        pbuf, pd = _padded(torch.full((K,), -99, dtype=torch.int32))
        hh.peaks(sd, wd, rd, vd, nd, pd, table, dev_sep, floor, top)
        torch.cuda.synchronize()
        for buf in (sbuf, wbuf, rbuf, vbuf, nbuf, pbuf):
            assert _intact(buf), name
        assert torch.equal(_bits(sd.cpu()), _bits(plane)) and table.host.tolist() == rows and table.dev.cpu().tolist() == rows
        runs.append([rd.cpu(), _bits(vd.cpu()), nd.cpu(), pd.cpu(), wd.cpu()])
    assert all(torch.equal(a, b) for a, b in zip(*runs)), name            # two runs, identical bytes (the workspace too)
    got_rows, got_vals, got_n, got_peaks, _ = runs[0]
    assert got_peaks.tolist() == want_peaks, name
    assert got_n.tolist() == [len(h) for h in want_hits], name
    pbits = _bits(plane)
    for k, h in enumerate(want_hits):
        assert got_rows[k].tolist() == h + [NONE] * (top - len(h)), (name, k)
        assert got_vals[k].tolist() == [int(pbits[r, k]) for r in h] + [0] * (top - len(h)), (name, k)
    SEEN[name] = _counts(key, counts, sep, want_hits, want_peaks)
    return want_hits, want_peaks


MATRIX = [(3, sep, top, floor) for sep in (0, 1, 2, 7, 300) for top in (1, 2, 5, 4096) for floor in (None, 0.25)]
MATRIX += [(1, 0, 4096, None), (1, 1, 1, 0.5), (1, 7, 5, None), (1, 300, 2, -0.5)]
MATRIX += [(64, 0, 5, None), (64, 1, 4096, 0.25), (64, 2, 1, None), (64, 7, 2, 0.0), (64, 300, 5, None)]


def _dyadic_case(K, sep, top, floor):
    name = "dyadic-%d-%d-%d-%r" % (K, sep, top, floor)
    plane = _dyadic(sum(LENGTHS), K, 1000 * K + 10 * sep + top)
    hits, peaks = _peaks_case(name, plane, LENGTHS, sep, floor, top)
    assert max(peaks) > 0
    return name


@pytest.mark.parametrize("K,sep,top,floor", MATRIX)
def test_peaks_and_hits_equal_the_reference(K, sep, top, floor):
    _dyadic_case(K, sep, top, floor)


@pytest.mark.parametrize("top", [1, 7, 300, 4096])
def test_scores_that_differ_in_their_low_mantissa_bytes_alone(top):
    """the keys of the first plane share their top byte and those of the second their top three, so the first radix passes decide nothing and the
    last everything (with ties in every bin); the third plane holds random finite bit patterns, denormals too: every pass decides"""
    g = torch.Generator().manual_seed(top)
    NW = sum(LENGTHS)
    for name, base, bits in (("low23", 0x3F800000, 23), ("low8", 0x3F81A500, 8), ("any", 0, 32)):
        raw = torch.randint(0, 1 << bits, (NW, 2), generator=g, dtype=torch.int64) + base
        raw = torch.where((raw & 0x7F800000) == 0x7F800000, raw & ~0x00800000, raw)          # no NaN, no infinity
        plane = torch.where(raw >= 1 << 31, raw - (1 << 32), raw).to(torch.int32).view(torch.float32)
        assert bool(torch.isfinite(plane).all())
        _peaks_case("%s-%d" % (name, top), plane, LENGTHS, 2, None, top)


@pytest.mark.parametrize("sep,top", [(0, 4096), (0, 3), (1, 2), (300, 4096)])
def test_an_all_equal_plane(sep, top):
    """a plateau yields its first window only; with separation = 0 every window is a peak and `top` keeps the lowest plane rows"""
    plane = torch.full((sum(LENGTHS), 3), 0.5)
    hits, peaks = _peaks_case("equal-%d-%d" % (sep, top), plane, LENGTHS, sep, None, top)
    starts = [sum(LENGTHS[:i]) for i, n in enumerate(LENGTHS) if n]
    if sep == 0:
        assert peaks == [sum(LENGTHS)] * 3 and hits[0] == list(range(min(top, sum(LENGTHS))))
    else:                                          # window 2 is beaten by window 1, which is no peak itself: a filter, not suppression
        assert peaks == [len(starts)] * 3 and hits[1] == starts[:top]


def test_a_single_row_and_a_single_window():
    for counts in ([1], [0, 0, 1], [5]):
        plane = _dyadic(sum(counts), 3, 7)
        _peaks_case("tiny-%r" % (counts,), plane, counts, 1, None, 2)


def test_every_count_is_non_zero_over_the_cases():
    """a degenerate generator -- no ties, nothing suppressed, no cut at a tie -- cannot pass.  (A case that was deselected runs here.)"""
    names = [name if name in SEEN else _dyadic_case(*params) for params, name in ((p, "dyadic-%d-%d-%d-%r" % p) for p in MATRIX)]
    total = [sum(SEEN[name][i] for name in names) for i in range(3)]
    assert all(n > 0 for n in total), total      # suppressed candidates, equal-score suppressions, last-place ties dropped
    for K in (1, 3, 64):                         # and at every width
        mine = [sum(SEEN[name][i] for name in names if name.startswith("dyadic-%d-" % K)) for i in range(3)]
        assert all(n > 0 for n in mine), (K, mine)


# ------------------------------------------------------------------ 2: the pool
STRIDE, MAX_PUSH, EXTRA = 2, 5, 3                 # a ring of (T - 1) + 5 = 12 frames, a store of 15: it wraps three times, pushes run 3 rounds
COUNTS = [(9, 10, 8), (2, 8, 3), (3, 2, 0), (1, 3, 4), (7, 1, 2), (2, 9, 2), (13, 1, 0), (3, 0, 12), (6, 5, 4)]      # test_gpu_events' schedule
SEARCH = [7, 2, 9]                                # in another order than the gallery's columns


def _history(rate=1, extra=EXTRA):
    from clip_fsar_amd.history import History
    return History(frames=(T - 1) * rate + MAX_PUSH + extra)


def _pool(live, history=True, **kw):
    from clip_fsar_amd.pool import StreamPool
    rate = kw["rates"][-1] if "rates" in kw else 1
    if history:
        kw["history"] = _history(rate)
    return StreamPool(live, max_streams=4, stride=STRIDE, max_push=MAX_PUSH, **kw)


class _Run:
    """a pool driven through COUNTS with features everybody can rebuild: per session the rows pushed so far and the logits row of every
    window a push completed"""

    def __init__(self, pool, counts=COUNTS, sessions=3, seed=300):
        self.pool, self.E = pool, pool.E
        self.hs = [pool.open() for _ in range(sessions)]
        self.rows = {h: torch.empty(0, self.E, device=DEV) for h in self.hs}
        self.logits, self.outs, self.tick, self.seed = {h: {} for h in self.hs}, [], 0, seed
        for c in counts:
            self.push(c)

    def push(self, counts):
        self.tick += 1
        feats = {h: _feats(k, self.E, self.seed + 10 * self.tick + i) for i, (h, k) in enumerate(zip(self.hs, counts)) if k}
        out = self.pool.push_features(feats)
        for h, f in feats.items():
            self.rows[h] = torch.cat([self.rows[h], f])
            for k in range(out[h].logits.shape[0]):
                self.logits[h][out[h].first_window + k] = out[h].logits[k]
        self.outs.append(out)
        return out

    def window(self, h, w, rate=1, rmax=1):
        """the T pushed rows of window w of session h read at `rate` in a pool that plans with rmax"""
        e = w * STRIDE + (T - 1) * rmax
        return self.rows[h][[e - (T - 1 - j) * rate for j in range(T)]]

    def rebuilt(self, result, rate=1, rmax=1):
        """the windows of a search's plane, rebuilt on the host side from the pushed rows: [NW, T, E]"""
        X = [self.window(h, first + k, rate, rmax) for h, first, (o0, o1) in zip(result.sessions, result.first_window, zip(
            result.offsets, result.offsets[1:])) for k in range(o1 - o0)]
        return torch.stack(X) if X else torch.empty(0, T, self.E, device=DEV)


def _scored(live, X, ids):
    per = max(1, live._fresh_engine().max_frames // T)
    return torch.cat([live.classify_features(X[w0:w0 + per].contiguous(), classes=ids).clone() for w0 in range(0, X.shape[0], per)])


def _same_outputs(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert list(x) == list(y)
        for h in x:
            assert x[h].first_window == y[h].first_window
            for name in ("logits", "smoothed", "deviation", "tempo"):
                p, q = getattr(x[h], name, None), getattr(y[h], name, None)
                assert (p is None) == (q is None) and (p is None or torch.equal(_bits(p), _bits(q))), (h, name)


def _store_is_the_ring(pool):
    """white box: the newest cap frames of every session lie in both, at f mod F and at f mod cap"""
    F = pool._history.frames
    for h in pool.sessions:
        s = pool._sessions[h]
        for f in range(max(0, s.t - pool.cap), s.t):
            assert torch.equal(pool._hs_store[s.slot, f % F], pool._ring[s.slot, f % pool.cap]), (h, f)


@pytest.mark.parametrize("config", ["plain", "by_class", "events", "rates"])
def test_the_option_changes_no_output_bit(config):
    from clip_fsar_amd.events import EventRule
    kw = {"plain": {}, "by_class": dict(smooth=0.5, smooth_by="class"), "rates": dict(rates=(1, 2)),
          "events": dict(smooth=0.5, smooth_by="class", events=EventRule(0.55, 0.45, 2, 2))}[config]
    with torch.no_grad():
        live = _gallery("live")
        plain, mine = _Run(_pool(live, history=False, **kw)), _Run(_pool(live, **kw))
    _same_outputs(plain.outs, mine.outs)
    assert plain.pool.stats() == mine.pool.stats() and not hasattr(plain.pool, "_hs_store")
    if config == "events":
        assert plain.pool.take_events() == mine.pool.take_events()
    _store_is_the_ring(mine.pool)
    assert tuple(mine.pool._hs_store.shape) == (4, mine.pool.cap + EXTRA, live.E)
    assert max(max(c) for c in COUNTS) > 2 * MAX_PUSH and max(s.t for s in mine.pool._sessions.values()) > 2 * mine.pool._history.frames


def test_the_option_changes_no_output_bit_of_a_gated_pixel_push():
    """still= on pixel pushes (the fixture has a tower): repeated frames skip it, and the store holds the rows the ring holds"""
    import clip_fsar_amd.synth as synth
    from clip_fsar_amd.still import StillGate
    from test_gpu_live import ARCH
    res = synth.ARCHS[ARCH]["res"]
    g = torch.Generator().manual_seed(3)
    base = (torch.randn(9, 3, res, res, generator=g) * 0.5).to(DEV)
    with torch.no_grad():
        live = _gallery("live")
        pools = [_pool(live, history=False, still=StillGate()), _pool(live, still=StillGate())]
        hs = [(p.open(), p.open()) for p in pools]
        outs = [[], []]
        for pick_a, pick_b in (([0, 0, 1, 1, 1, 2, 2], [3, 4]), ([2, 2, 5, 5, 5, 5, 6, 6, 6, 6, 7, 8], [4, 4, 4, 3, 3, 3, 3, 1, 1])):
            for i, p in enumerate(pools):
                outs[i].append(p.push({hs[i][0]: base[pick_a], hs[i][1]: base[pick_b]}))
    _same_outputs(*outs)
    assert pools[0].stats() == pools[1].stats() and pools[1].stats()["still_frames"] > 8
    assert pools[0].last_kept() == pools[1].last_kept()
    _store_is_the_ring(pools[1])
    r = pools[1].search(SEARCH)
    assert r.windows == len(pools[1].searchable(hs[1][0])) + len(pools[1].searchable(hs[1][1])) > 4


@pytest.fixture(scope="module")
def run():
    with torch.no_grad():
        live = _gallery("live")
        return live, _Run(_pool(live))


def test_the_plane_is_classify_features_of_the_held_windows_and_the_pushes_own_logits(run):
    live, r = run
    p = r.pool
    with torch.no_grad():
        res = p.search(SEARCH)
        want = _scored(live, r.rebuilt(res), SEARCH)
    F = p._history.frames
    assert res.sessions == r.hs and res.windows == res.offsets[-1] == res.scores.shape[0] and tuple(res.scores.shape)[1] == 3
    for h, first, o0, o1 in zip(res.sessions, res.first_window, res.offsets, res.offsets[1:]):
        ws = p.searchable(h)
        assert (first, o1 - o0) == (ws.start, len(ws)) and len(ws) >= (F - T) // STRIDE           # the store is all but full of windows
        assert ws.start * STRIDE >= p._sessions[h].t - F > (ws.start - 1) * STRIDE
    assert torch.equal(_bits(res.scores), _bits(want))
    cols = [live.class_ids.index(c) for c in SEARCH]
    own = torch.stack([r.logits[h][first + k][cols] for h, first, o0, o1 in zip(res.sessions, res.first_window, res.offsets, res.offsets[1:])
                       for k in range(o1 - o0)])
    assert torch.equal(_bits(res.scores), _bits(own))


def _check_hits(res, ids, sep, floor, top, tempo=None):
    from clip_fsar_amd.history import Hit, reference_search
    plane = res.scores.cpu()
    counts = [o1 - o0 for o0, o1 in zip(res.offsets, res.offsets[1:])]
    want_rows, want_peaks = reference_search(plane, counts, sep, floor, top)
    owner = [i for i, n in enumerate(counts) for _ in range(n)]
    for k, c in enumerate(ids):
        order = sorted(want_rows[k], key=lambda row: (-float(plane[row, k]), row))
        want = [Hit(res.sessions[owner[row]], c, res.first_window[owner[row]] + row - res.offsets[owner[row]], float(plane[row, k]), tempo)
                for row in order]
        assert res.hits[c] == want and res.peaks[c] == want_peaks[k], c
        assert [np.float32(h.score).view(np.uint32) for h in res.hits[c]] == [plane[row, k].view(torch.int32).item() & 0xFFFFFFFF for row in order]
    return want_rows, want_peaks


def test_hits_and_peaks_are_the_reference_over_the_downloaded_plane(run):
    live, r = run
    default = ((T - 1) * 1) // STRIDE
    with torch.no_grad():
        for kw, sep, floor, top in ((dict(), default, None, 16), (dict(top=2), default, None, 2), (dict(separation=0, top=4096), 0, None, 4096),
                                    (dict(separation=1, top=3), 1, None, 3), (dict(separation=10 ** 6), 10 ** 6, None, 16)):
            res = r.pool.search(SEARCH, **kw)
            _, peaks = _check_hits(res, SEARCH, sep, floor, top)
            assert all(len(res.hits[c]) == min(top, n) for c, n in zip(SEARCH, peaks))
        median = float(res.scores.median())
        res = r.pool.search(SEARCH, min_score=median, separation=0, top=4096)
        _check_hits(res, SEARCH, 0, median, 4096)
        assert 0 < sum(res.peaks.values()) < res.scores.numel()                # about half the plane
        # last=: the windows completed by the newest frames alone, and a subset of the sessions in another order
        res = r.pool.search([9], sessions=[r.hs[2], r.hs[0]], last=5)
        newest = [[w for w in r.pool.searchable(h) if w * STRIDE + T - 1 >= r.pool._sessions[h].t - 5] for h in res.sessions]
        assert res.sessions == [r.hs[2], r.hs[0]] and sorted(len(ws) for ws in newest) == [2, 3]
        assert [(f, o1 - o0) for f, o0, o1 in zip(res.first_window, res.offsets, res.offsets[1:])] == [(ws[0], len(ws)) for ws in newest]
        assert torch.equal(_bits(res.scores), _bits(_scored(live, r.rebuilt(res), [9])))
        _check_hits(res, [9], default, None, 16)


def test_the_order_of_the_sessions_decides_a_tie_as_the_reference_says():
    """two sessions fed the same frames score the same bits: with top = 1 the hit is the session searched first"""
    with torch.no_grad():
        live = _gallery("live")
        p = _pool(live)
        a, b = p.open(), p.open()
        f = _feats(14, live.E, 9)
        p.push_features({a: f[:9], b: f[:4]})
        p.push_features({b: f[4:], a: f[9:]})
        fwd, back = p.search([4], top=1), p.search([4], sessions=[b, a], top=1)
    assert torch.equal(_bits(fwd.scores), _bits(back.scores)) and fwd.windows == 2 * len(p.searchable(a)) == 8
    _check_hits(fwd, [4], 3, None, 1)
    _check_hits(back, [4], 3, None, 1)
    (x,), (y,) = fwd.hits[4], back.hits[4]
    assert (x.session, y.session) == (a, b) and x[1:] == y[1:] and fwd.peaks == back.peaks


def test_reset_and_a_reused_slot_hide_the_past():
    with torch.no_grad():
        live = _gallery("live")
        r = _Run(_pool(live), COUNTS[:3])
        p, (a, b, c) = r.pool, r.hs
        assert len(p.searchable(a)) and len(p.searchable(c))
        p.reset(a)
        assert p.searchable(a) == range(0) and p.search(SEARCH, sessions=[a]).windows == 0
        slot = p._sessions[c].slot
        p.close(c)
        with pytest.raises(ValueError, match="session %d is not open" % c):
            p.search(SEARCH, sessions=[c])
        d = p.open()
        assert p._sessions[d].slot == slot and p.searchable(d) == range(0)
        res = p.search(SEARCH)
        assert res.sessions == [a, b, d] and [o1 - o0 for o0, o1 in zip(res.offsets, res.offsets[1:])] == [0, len(p.searchable(b)), 0]
        assert all(h.session == b for hits in res.hits.values() for h in hits)
        # the new lives: fewer frames than a window, then windows of the new rows alone
        r.hs = [a, b, d]
        r.rows[a], r.rows[d], r.logits[d] = r.rows[a][:0], torch.empty(0, live.E, device=DEV), {}
        r.push((T - 1, 0, T + 4))
        assert p.searchable(a) == range(0) and p.searchable(d) == range(0, 3)
        res = p.search(SEARCH, sessions=[d, a])
        assert res.windows == 3 and torch.equal(_bits(res.scores), _bits(_scored(live, r.rebuilt(res), SEARCH)))
        r.push((9, 0, 9))
        res = p.search(SEARCH, sessions=[a, d])
        assert res.first_window == [p.searchable(a).start, p.searchable(d).start] and res.windows > 6
        assert torch.equal(_bits(res.scores), _bits(_scored(live, r.rebuilt(res), SEARCH)))


def test_hit_features_explain_hit_and_enroll_hit_read_the_pushed_rows():
    from clip_fsar_amd.align import Aligner
    from test_gpu_enroll import _assert_same_classes
    with torch.no_grad():
        live, twin = _gallery("live"), _gallery("live")
        r = _Run(_pool(live))
        p = r.pool
        res = p.search(SEARCH, top=12, separation=0)                              # every held window of every session is a hit
        hits = [h for c in SEARCH for h in res.hits[c]]
        assert len(hits) == 36 and len({h.session for h in hits}) == 3
        assert any(h.window not in p.enrolable(h.session) for h in hits)          # the ring has moved past some of them
        for h in hits:
            assert h.window in p.searchable(h.session) and h.tempo is None
            assert torch.equal(p.hit_features(h), r.window(h.session, h.window))
        h = next(h for h in hits if h.window not in p.enrolable(h.session))
        rows = r.window(h.session, h.window)
        want = Aligner(live).align_features(rows.unsqueeze(0), [h.class_id])
        got = p.explain_hit(h)
        assert all(torch.equal(getattr(got, n), getattr(want, n)) for n in ("plan", "dists", "logits")) and got.plan.shape[0] == 1
        assert p.explain_hit(h, k=2).plan.shape[0] == 2
        before = (p.stats(), p._ring.clone(), p._hs_store.clone())
        assert (p.enroll_hit(h, IDS[0]), p.enroll_hit(h, 15)) == (2, 1)
        assert list(twin.add_shots_features(rows.unsqueeze(0), [IDS[0]])) == [2]
        twin.add_classes_features(rows.unsqueeze(0), [15])
        _assert_same_classes(live, twin)
        assert live.class_ids == IDS + [15] and live.shots(IDS[0]) == 2
        assert p.stats() == before[0] and torch.equal(p._ring, before[1]) and torch.equal(p._hs_store, before[2])
        found = p.search([15], sessions=[h.session], top=1).hits[15][0]           # the enrolled window is where the class happened
        assert found.window == h.window
        # a hit that has left the history raises, and changes nothing
        r.push((MAX_PUSH + EXTRA + 2 * STRIDE + 9, 1, 1))
        old = next(x for x in hits if x.session == r.hs[0])
        assert old.window not in p.searchable(old.session)
        state = (live.class_ids, live.shots(IDS[0]), p.stats(), p._hs_store.clone())
        for call in (lambda: p.hit_features(old), lambda: p.explain_hit(old), lambda: p.enroll_hit(old, IDS[0])):
            with pytest.raises(ValueError, match=r"session %d: window %d is not enrolable -- the ring holds its windows range\(\d+, \d+\) "
                               r"\(\d+ frames since open\(\) / reset\(\), cap = %d\)" % (old.session, old.window, p._history.frames)):
                call()
        assert state[:3] == (live.class_ids, live.shots(IDS[0]), p.stats()) and torch.equal(state[3], p._hs_store)


def test_tempo_reads_the_frames_tempo_positions_names():
    from clip_fsar_amd.history import plan_search
    from clip_fsar_amd.pool import tempo_positions
    rates = (1, 2)
    with torch.no_grad():
        live = _gallery("live")
        r = _Run(_pool(live, rates=rates))
        p = r.pool
        F = p._history.frames
        assert p.cap == (T - 1) * 2 + MAX_PUSH and F == p.cap + EXTRA
        planes = []
        for tempo, at in ((None, 1), (1, 1), (0, 0)):
            res = p.search(SEARCH, tempo=tempo, top=3)
            assert torch.equal(_bits(res.scores), _bits(_scored(live, r.rebuilt(res, rates[at], rates[-1]), SEARCH)))
            _check_hits(res, SEARCH, (T - 1) * 2 // STRIDE, None, 3, tempo=at)
            for h in res.hits[7]:
                assert h.tempo == at and torch.equal(p.hit_features(h), r.window(h.session, h.window, rates[at], rates[-1]))
            planes.append(res.scores)
        assert torch.equal(planes[0], planes[1]) and not torch.equal(planes[0], planes[2])
        # the store rows behind a window are the ones tempo_positions names over the search's table
        s = p._sessions[r.hs[0]]
        row = plan_search([(s.slot, s.t)], T, STRIDE, rates[-1], F).rows[0]
        first = p.searchable(r.hs[0]).start
        for w in (0, row[5] - 1):
            for i, at in enumerate(tempo_positions(row[4], w, STRIDE, T, rates, F)):
                assert torch.equal(p._hs_store[s.slot][at], r.window(r.hs[0], first + w, rates[i], rates[-1]))
        # the tempo the reduced logits name is where the search finds the score
        out_logits = r.logits[r.hs[0]][first]
        cols = [live.class_ids.index(c) for c in SEARCH]
        assert torch.equal(torch.maximum(planes[1][0], planes[2][0]), out_logits[cols])
        with pytest.raises(ValueError, match=r"StreamPool.search: tempo must be an index into rates = \(1, 2\)"):
            p.search(SEARCH, tempo=2)
        q = _pool(live)
        q.open()
        with pytest.raises(ValueError, match="StreamPool.search: tempo = 0 on a pool without rates="):
            q.search(SEARCH, tempo=0)


def test_the_cut_of_the_pushes_does_not_matter(run):
    live, r = run
    totals = [sum(c[i] for c in COUNTS) for i in range(3)]
    with torch.no_grad():
        whole = r.pool.search(SEARCH, top=5)
        other = _pool(live)
        hs = [other.open() for _ in range(3)]
        for i, h in enumerate(hs):                 # one session at a time, in pushes of 4 and of everything left
            other.push_features({h: r.rows[r.hs[i]][:4]})
            other.push_features({h: r.rows[r.hs[i]][4:totals[i]]})
        again = other.search(SEARCH, top=5)
    assert again.first_window == whole.first_window and again.offsets == whole.offsets
    assert torch.equal(_bits(again.scores), _bits(whole.scores))
    assert {c: [h[1:] for h in hits] for c, hits in again.hits.items()} == {c: [h[1:] for h in hits] for c, hits in whole.hits.items()}
    assert again.peaks == whole.peaks


def test_search_refusals_on_the_device(run):
    live, r = run
    p = r.pool
    for kw, words in ((dict(top=0), "top must be an integer in"), (dict(top=4097), "top must be an integer in"),
                      (dict(separation=-1), "separation must be an integer >= 0"), (dict(last=0), "last must be None or an integer >= 1"),
                      (dict(min_score=NAN), "min_score must be None or a number that is not NaN"),
                      (dict(sessions=[r.hs[0], r.hs[0]]), "a session appears twice")):
        with pytest.raises(ValueError, match="StreamPool.search: " + words):
            p.search(SEARCH, **kw)
    with pytest.raises(ValueError, match=r"StreamPool.search: a class appears twice in classes=: \[7, 7\]"):
        p.search([7, 7])
    with pytest.raises(ValueError, match="StreamPool.search"):
        p.search([7, 12345])
