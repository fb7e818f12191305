"""GPU: the pinned selection (libclipfsar_pool_select.so) through its C ABI, bit for bit against reference_select_pinned and a host
restatement of the commit, at every chunk edge, keep, group size and pin count, through every clause of the pin rule and its near-misses;
then StreamPool(shortlist=...) on the small LiveGallery of tests/test_gpu_shortlist.py: keep >= C against the pool without a shortlist,
keep = 3 against the host rule with the pins read back from the pool's cells, a gap schedule, a host replay of the three recurrences of
every listed pair with restarts at gaps, the hold, the refusals, the no-crossing check, growth of the store and a reused slot.

Every output and plane lives inside a larger buffer of sentinels that must be intact afterwards."""
import pytest
import torch

from test_gpu_shortlist import C, DEV, NAN, T, _bits, _group_scores, _guarded, _scores, world  # noqa: F401  (world: the fixture)
from test_shortlist_abi import NONE

pytestmark = pytest.mark.gpu
EV, HOLD = 1, 2                                   # CFPS_PIN_EVENT, CFPS_PIN_HOLD


# ------------------------------------------------------------------ 1: selection and commit through the C ABI
class _Case:
    """One call's inputs, made on the host: scores, columns, the table and the six planes, with `want[j]` pins planted in group j on its
    WORST columns (so that a kept pin is kept against better scores), each through one clause of the rule in turn, and every other cell of
    the group's rows a near-miss of the rule."""

    def __init__(self, NC, counts, keep, want, hold, null, seed):
        g = torch.Generator().manual_seed(seed)
        self.NC, self.counts, self.keep, self.hold, self.null = NC, counts, keep, hold, null
        self.K = K = min(keep, NC)
        G = self.G = len(counts)
        self.ms, self.cap = G + 3, NC + 9
        self.S = _scores(sum(counts), NC, counts, seed)
        self.cols = torch.randperm(NC + 7, generator=g)[:NC].to(torch.int32)      # keys in [0, NC + 7), all below cap, none twice
        if NC >= 5:                                                                # and two columns whose key is outside the store
            self.cols[1], self.cols[NC - 2] = -1, self.cap
        self.slots = torch.randperm(self.ms, generator=g)[:G].tolist()             # permuted SLOTs
        self.ticks = [hold + 1 + j % 4 for j in range(G)]
        if G > 2:
            self.ticks[2] = 1 << 30
        self.gens = torch.randint(1, 6, (self.cap,), generator=g).to(torch.int32)
        shape = (self.ms, self.cap)
        rnd = lambda lo, hi: torch.randint(lo, hi, shape, generator=g).to(torch.int32)
        # every row starts as noise: the rows of slots that are in no group must come back unchanged
        self.planes = {"ev_streak": rnd(-3, 4), "ev_marks": rnd(0, 7), "seen": rnd(0, 5), "merit": rnd(0, 5), "smooth_marks": rnd(1, 9),
                       "base_marks": rnd(1, 9)}
        scores = _group_scores(self.S, counts)
        key = self.cols.long()
        ok = (key >= 0) & (key < self.cap)
        keyc = key.clamp(0, self.cap - 1)
        for j, (n, s, t) in enumerate(zip(counts, self.slots, self.ticks)):
            p = self.planes
            gen = self.gens[keyc]
            past = t - hold - 1 if t - hold - 1 >= 1 else 0                        # a merit one past the hold (or none)
            c = torch.arange(NC)
            # the near-misses, by column: a stale mark; seen = t - 2; an idle cell; an idle cell again; seen = t
            kind = c % 5
            seen = torch.where(kind == 1, t - 2, torch.where(kind == 4, t, torch.where(kind == 2, 0 if t > 1 else 5, t - 1)))
            marks = torch.where(kind == 0, gen + 1, gen)
            streak = torch.tensor([3, -1, 2, 0, 5])[kind]
            merit = torch.tensor([past, t - 1, 0, 0, t])[kind]
            merit = torch.where(kind == 3, torch.zeros_like(merit), merit)
            # the pins: the group's worst columns with a key inside the store (no score first, then the lowest scores)
            if want[j]:
                sj, inside = scores[j].tolist(), ok.tolist()
                order = sorted((cc for cc in range(NC) if inside[cc]), key=lambda cc: (sj[cc] == sj[cc], sj[cc] if sj[cc] == sj[cc] else 0.0, cc))
                at = torch.tensor(order[:want[j]], dtype=torch.long)
                clause = torch.arange(at.shape[0]) % (3 if hold > 0 else 2)
                # clause 0: a counting onset streak, no hold; 1: a running event, the hold one past; 2: a stale mark, the hold exactly
                # at `hold`
                seen[at] = t - 1
                marks[at] = torch.where(clause == 2, gen[at] + 1, gen[at])
                streak[at] = torch.tensor([2, -1, -2])[clause]
                merit[at] = torch.tensor([0, past, t - hold])[clause]
            for name, values in (("seen", seen), ("ev_marks", marks), ("ev_streak", streak), ("merit", merit)):
                p[name][s, keyc[ok]] = values[ok].to(torch.int32)
        self.scores = scores

    def given(self, name):
        return not (name in self.null or (name == "ev_streak" and "ev_marks" in self.null))

    def pins(self):
        """per group {column: bits}: the rule of the header restated over the planes"""
        out = []
        key = self.cols.long()
        ok = (key >= 0) & (key < self.cap)
        keyc = key.clamp(0, self.cap - 1)
        p = self.planes
        for s, t in zip(self.slots, self.ticks):
            at_prev = ok & (p["seen"][s, keyc] == t - 1)
            ev = at_prev & (p["ev_marks"][s, keyc] == self.gens[keyc]) & (p["ev_streak"][s, keyc] != 0) & self.given("ev_marks")
            m = p["merit"][s, keyc].long()
            hd = at_prev & (m >= 1) & (t - m <= self.hold) & (self.hold > 0)
            bits = ev.long() * EV + hd.long() * HOLD
            out.append({c: b for c, b in enumerate(bits.tolist()) if b})
        return out

    def expected(self):
        """(columns, slots, pins [G, K], n_pins [G], the planes after the commit) by reference_select_pinned and the header's commit"""
        from clip_fsar_amd.shortlist import reference_select_pinned
        if getattr(self, "_expected", None) is not None:
            return self._expected
        pinned = self.pins()
        cols, bits, n = reference_select_pinned(self.S, self.counts, self.keep, pinned)
        after = {k: v.clone() for k, v in self.planes.items()}
        slots = []
        for row, brow, s, t in zip(cols, bits, self.slots, self.ticks):
            row, brow = torch.tensor(row, dtype=torch.long), torch.tensor(brow, dtype=torch.long)
            key = torch.where(row != NONE, self.cols[row.clamp(max=self.NC - 1)].long(), torch.full_like(row, -1))
            slots.append(key.tolist())
            inside = (key >= 0) & (key < self.cap)
            key, brow = key[inside], brow[inside]
            gap = key[after["seen"][s, key] != t - 1]              # new, or back after a gap: every state starts anew
            for name in ("smooth_marks", "base_marks", "ev_marks"):
                if self.given(name):
                    after[name][s, gap] = 0
            after["seen"][s, key] = t
            after["merit"][s, key[brow == 0]] = t
        i32 = lambda rows: torch.tensor(rows, dtype=torch.int32).view(self.G, self.K)
        self._expected = i32(cols), i32(slots), i32(bits), torch.tensor(n, dtype=torch.int32), after, pinned
        return self._expected

    def claims(self, cols, pinned):
        """(a kept pin beats a better score that is left out, P > K occurs) -- from the scores and the reference alone"""
        against = over = False
        for j, (row, pin) in enumerate(zip(cols.tolist(), pinned)):
            if not self.counts[j]:
                continue
            over = over or len(pin) > self.K
            sc, kept = self.scores[j].tolist(), set(row)
            left = [sc[c] for c in range(self.NC) if c not in kept and c not in pin and sc[c] == sc[c]]
            best = max(left) if left else None
            against = against or any(c in pin and best is not None and (sc[c] != sc[c] or best > sc[c]) for c in row if c != NONE)
        return against, over

    def run(self, work_fill):
        from clip_fsar_amd import pool_select_hip as ph
        G, K = self.G, self.K
        outs = [_guarded((G, K), torch.int32, f) for f in (12345, 54321, 777)] + [_guarded((G,), torch.int32, -9)]
        work, check_w = _guarded((ph.workspace_floats(G, self.NC),), torch.float32, work_fill)
        planes, checks = {}, [check_w] + [c for _, c in outs]
        for name, host in self.planes.items():
            planes[name], check = _guarded(tuple(host.shape), torch.int32, -77)
            planes[name].copy_(host)
            checks.append(check)
        s, c, gens = self.S.to(DEV), self.cols.to(DEV), self.gens.to(DEV)
        rows, total = ph.table_rows(self.counts, self.slots, self.ticks)
        assert total == self.S.shape[0]
        arg = lambda name: planes[name] if self.given(name) else None
        ph.select_pinned(s, c, gens, arg("ev_streak"), arg("ev_marks"), planes["seen"], planes["merit"], arg("smooth_marks"),
                         arg("base_marks"), ph.table_uploader(DEV, G).upload(rows), self.keep, self.hold, *(o for o, _ in outs), work)
        torch.cuda.synchronize()
        for check in checks:
            check()
        assert torch.equal(_bits(s.cpu()), _bits(self.S)) and torch.equal(c.cpu(), self.cols) and torch.equal(gens.cpu(), self.gens)
        return [o.cpu() for o, _ in outs], {k: v.cpu() for k, v in planes.items()}


def _check(case, label):
    """the device against the host's expectation; what the case shows was asserted by the caller, on the host, before this is called"""
    cols, slots, bits, n, after, pinned = case.expected()
    outs, planes = case.run(3.0)
    for got, ref, name in zip(outs, (cols, slots, bits, n), ("sel_cols", "sel_slots", "sel_pin", "n_pins")):
        assert torch.equal(got, ref), (label, name)
    for name, ref in after.items():                # the whole plane: the other slots' rows and the unselected cells are unchanged
        assert torch.equal(planes[name], ref if case.given(name) else case.planes[name]), (label, name)
    outs2, planes2 = case.run(-1.5)                # another run from the same planes, other garbage in the workspace: identical bytes
    assert all(torch.equal(a, b) for a, b in zip(outs, outs2)) and all(torch.equal(planes[k], planes2[k]) for k in planes), label


NULLS = ((), ("smooth_marks",), ("base_marks",), ("ev_marks",), ("smooth_marks", "base_marks"))


@pytest.mark.parametrize("NC", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_select_pinned_equals_the_reference_and_the_commit_bit_for_bit(NC):
    keeps = sorted({k for k in (1, 2, NC - 1, NC, NC + 5) if k >= 1})
    many = [(0, 1, 3, 17)[i % 4] for i in range(300)]
    call = 0
    shown = {"against": 0, "over": 0, "fit": 0}
    for counts in ([1], [3], [17], [0, 1], many):
        for keep in keeps:
            K = min(keep, NC)
            settings = sorted({w for w in (0, 1, K - 1, K, K + 3) if w >= 0})
            # G = 1 (and the lone empty group that rides with one clip): a call per pin count; G = 300: the counts in turn, group by group
            plans = [[settings[(i + call) % len(settings)] for i in range(300)]] if counts is many else [[w] * len(counts) for w in settings]
            for want in plans:
                hold, null = (2, 0, 3)[call % 3], NULLS[call % len(NULLS)]
                case = _Case(NC, counts, keep, want, hold, null, seed=NC * 131 + call)
                cols, pinned = case.expected()[0], case.expected()[5]
                if not null and hold:              # every clause is available: the planted count is the true one wherever columns exist
                    inside = int(((case.cols >= 0) & (case.cols < case.cap)).sum())
                    assert [len(p) for p in pinned] == [min(w, inside) for w in want], (NC, counts[:4], keep)
                against, over = case.claims(cols, pinned)
                live = [j for j, n in enumerate(counts) if n]
                assert over == any(len(pinned[j]) > K for j in live)
                # a kept pin sits on the group's worst columns: wherever a scored column is left out it beats the pin
                if any(pinned[j] and K < NC - 4 for j in live):
                    assert against, (NC, counts[:4], keep, want[:4])
                shown["against"] += against
                shown["over"] += over
                shown["fit"] += any(0 < len(pinned[j]) <= K for j in live)
                _check(case, (NC, counts[:4], keep, want[:4], hold, null))
                call += 1
    if NC >= 63:                                   # no size passes vacuously
        assert min(shown.values()) > 0, shown


# ------------------------------------------------------------------ 2: StreamPool(shortlist=...) on the small LiveGallery
# The world's clips by class: 0-2 class 2, 3 class 7, 4-8 class 17, 9-10 class 22, 11-14 class 3, 15-19 class 8 (families of three classes).
# A pool with stride = T, rate = 1 turns a clip's T tower rows into exactly one window, so a push of clips is a push of windows.
A, OTHER = 17, 3
A_CLIPS, OTHER_CLIPS = [4, 5, 6, 7, 8], [11, 12, 13, 14]


def _pool(live, **kw):
    from clip_fsar_amd.pool import StreamPool
    return StreamPool(live, max_streams=4, stride=T, rate=1, max_push=3 * T, **kw)     # more than 3 clips of a session: a second round


def _frames(world, clips):
    return world.feats[torch.tensor(clips, device=DEV)].reshape(len(clips) * T, -1).contiguous()


def _same(a, b):
    return (a is None and b is None) or (a.shape == b.shape and torch.equal(_bits(a), _bits(b)))


def _rule(world):
    """thresholds from the gallery's own full logits, not from the pool: with `low` the best logit of class A on the other class's clips
    and `gap` what its weakest logit on its own clips has above that, on = low + 0.8 gap and off = low + 0.6 gap.  Smoothed with
    alpha = 0.5 from a value v, the score is below `off` from the third window of the other class on when v - low < 4.8 gap."""
    from clip_fsar_amd.events import EventRule
    full = world.live.classify_features(world.feats)
    a_col = world.live.class_ids.index(A)
    own, other = full[A_CLIPS, a_col], full[OTHER_CLIPS, a_col]
    low, gap = float(other.max()), float(own.min() - other.max())
    assert gap > 0 and float(own.max()) - low < 4.8 * gap, (own.tolist(), other.tolist())
    return EventRule(on=low + 0.8 * gap, off=low + 0.6 * gap, min_on=2, min_off=2), full


SCHEDULE = [{0: [0, 1], 1: [4]}, {0: [2], 1: [5, 6, 7, 8, 11]}, {1: [12, 13]}, {0: [3, 9, 10, 15], 1: [14]}, {0: [16], 1: [7]},
            {0: [17, 18]}, {1: [8, 4]}]


@pytest.mark.parametrize("keep", [C, 64])
def test_keep_at_least_c_is_the_pool_without_a_shortlist_bit_for_bit(world, keep):
    from clip_fsar_amd.baseline import Baseline
    from clip_fsar_amd.events import EventRule
    from clip_fsar_amd.shortlist import Shortlist
    live = world.live
    with torch.no_grad():
        kw = dict(smooth=0.5, smooth_by="class", events=EventRule(on=0.5, off=-0.5, min_on=1, min_off=1),
                  baseline=Baseline(rate=0.25, warm_rate=0.5, warmup=2, gate=3.0))
        plain, listed = _pool(live, **kw), _pool(live, shortlist=Shortlist(live, keep=keep), shortlist_hold=2, **kw)
        hp, hl = [plain.open(), plain.open()], [listed.open(), listed.open()]
        rounds = 0
        for push in SCHEDULE:
            rounds += any(len(c) > 3 for c in push.values())
            a = plain.push_features({hp[i]: _frames(world, c) for i, c in push.items()})
            b = listed.push_features({hl[i]: _frames(world, c) for i, c in push.items()})
            for i in push:
                x, y = a[hp[i]], b[hl[i]]
                assert x.first_window == y.first_window and tuple(y.logits.shape) == (len(push[i]), C)
                assert _same(x.logits, y.logits) and _same(x.smoothed, y.smoothed) and _same(x.deviation, y.deviation), (push, i)
                assert y.columns.tolist() == list(range(C)) and y.class_ids() == live.class_ids
                va, ia = plain.topk(x, k=3)
                vb, ib = listed.topk(y, k=3)
                assert torch.equal(va, vb) and torch.equal(ia, ib)
        assert rounds                                   # a push of several rounds (round-major -> session-major) is among them
        ea, eb = plain.take_events(), listed.take_events()
        assert ea and repr(ea) == repr(eb)
        assert repr(plain.active(hp[1])) == repr(listed.active(hl[1])) and repr(plain.baseline(hp[0])) == repr(listed.baseline(hl[0]))
        assert listed.stats()["pins_dropped"] == 0 and listed.stats()["pins"] > 0


def _cell_pins(p, h, hold):
    """{column: bits} of session h at its next scoring push: the header's rule over the pool's cells, read back before the push"""
    live = p.gallery
    s = p._sessions[h]
    keys = live._columns(None).long()
    t = s.tick + 1
    if p._sl_cells.planes is None or s.slot in p._sl_cells.forgotten:
        return {}
    width = p._sl_cells.planes[0].shape[1]                     # a store that grew since the last push: its new slots were never scored
    inside, at = keys < width, keys.clamp(max=width - 1)
    seen, merit = (x[s.slot][at] for x in p._sl_cells.planes)
    prev = inside & (seen == t - 1)
    bits = torch.zeros_like(seen)
    if p._events is not None and p._ev_cells.planes is not None and s.slot not in p._ev_cells.forgotten:
        streak, _, _, marks = p._ev_cells.planes
        bits += (prev & (marks[s.slot][at] == live.slot_generations()[keys]) & (streak[s.slot][at] != 0)).int() * EV
    if hold:
        bits += (prev & (merit >= 1) & (t - merit <= hold)).int() * HOLD
    return {c: b for c, b in enumerate(bits.tolist()) if b}


def test_keep_3_columns_are_the_host_rule_and_logits_are_classify_features(world):
    from clip_fsar_amd.shortlist import Shortlist, reference_select_pinned
    live, ids = world.live, world.live.class_ids
    with torch.no_grad():
        rule, _ = _rule(world)
        sl = Shortlist(live, keep=3)
        p = _pool(live, smooth=0.5, smooth_by="class", events=rule, shortlist=sl, shortlist_hold=1)
        h = [p.open(), p.open()]
        kinds = set()
        for push in SCHEDULE:
            pinned = [_cell_pins(p, h[i], 1) for i in push]
            clips = [c for i in push for c in push[i]]
            S = Shortlist(live, keep=3).coarse_features(world.feats[torch.tensor(clips, device=DEV)]).cpu()
            want, bits, n = reference_select_pinned(S, [len(push[i]) for i in push], 3, pinned)
            out = p.push_features({h[i]: _frames(world, c) for i, c in push.items()})
            for j, i in enumerate(push):
                o = out[h[i]]
                assert o.columns.tolist() == want[j] and o.pinned.tolist() == bits[j], (push, i)
                assert o.class_ids() == [ids[c] if c != NONE else None for c in want[j]]
                exact = live.classify_features(world.feats[torch.tensor(push[i], device=DEV)], classes=[ids[c] for c in want[j]])
                assert torch.equal(o.logits, exact), (push, i)                     # bit for bit
                kinds |= set(bits[j])
        assert {EV, HOLD} <= {b & EV for b in kinds} | {b & HOLD for b in kinds}, kinds      # both clauses pinned something
        assert p.stats()["pins"] > 0


def _place(o, cls, ids):
    cols = o.columns.tolist()
    c = ids.index(cls)
    return cols.index(c) if c in cols else None


def test_a_gap_ends_nothing_early_and_a_return_starts_anew(world):
    """A session follows class A until its onset, switches to a class of another family, returns to A.  With a rule, A stays listed
    through its offset although its coarse rank is outside keep, and is dropped afterwards; at its return its detector cell starts idle.
    In a pool with a baseline and no rule A is dropped at once, and at its return its baseline counts from one.  (The smoothing's fresh
    start is the next test's.)"""
    from clip_fsar_amd.baseline import Baseline
    from clip_fsar_amd.shortlist import Shortlist
    live, ids = world.live, world.live.class_ids
    with torch.no_grad():
        rule, full = _rule(world)
        a_col = ids.index(A)
        # stated on the coarse scores alone: on the other class's clips A's rank is outside keep = 3
        S = Shortlist(live, keep=3).coarse_features(world.feats[torch.tensor(OTHER_CLIPS, device=DEV)])
        rank = (S > S[:, a_col:a_col + 1]).sum(1)
        assert int(rank.min()) >= 3, rank.tolist()
        pe = _pool(live, smooth=0.5, smooth_by="class", events=rule, shortlist=Shortlist(live, keep=3))
        pb = _pool(live, smooth=0.5, smooth_by="class", baseline=Baseline(warmup=16), shortlist=Shortlist(live, keep=3))     # n counts the windows up to warmup
        he, hb = pe.open(), pb.open()
        listed_e, listed_b, counts_b, streaks = [], [], [], []
        seq = A_CLIPS[:3] + OTHER_CLIPS + OTHER_CLIPS[:2] + A_CLIPS[3:]            # windows 0-2: A; 3-8: the other class; 9, 10: A again
        for clip in seq:
            oe = pe.push_features({he: _frames(world, [clip])})[he]
            ob = pb.push_features({hb: _frames(world, [clip])})[hb]
            listed_e.append(_place(oe, A, ids))
            listed_b.append(_place(ob, A, ids))
            counts_b.append({c: n for c, _, _, n in pb.baseline(hb)}.get(A))
            streaks.append(int(pe._ev_cells.planes[0][pe._sessions[he].slot, live.slot_of(A)]))
        events = [e for e in pe.take_events() if e.class_id == A]
        assert [(e.kind, e.window) for e in events[:1]] == [("onset", 1)] and [e.kind for e in events[1:2]] == ["offset"], events
        off_at = events[1].window                                                  # the window that confirmed the offset
        assert 3 < off_at <= 7, events                                             # while the stream shows the other class
        assert all(x is not None for x in listed_e[:off_at + 1]), listed_e         # listed through its offset, outside keep by its coarse rank
        assert listed_e[off_at + 1:9] and all(x is None for x in listed_e[off_at + 1:9]), listed_e      # dropped afterwards
        assert listed_e[9] is not None and listed_e[10] is not None
        assert streaks[9] == 1 and streaks[10] == -1 and [(e.kind, e.window) for e in events[2:]] == [("onset", 10)]    # idle at its return
        assert [a[0] for a in pe.active(he) if a[0] == A] == [A]
        # the pool without a rule drops A with the first window of the other class, and A's baseline starts anew at its return
        assert all(x is not None for x in listed_b[:3]) and all(x is None for x in listed_b[3:9]) and listed_b[9] is not None, listed_b
        assert counts_b[:3] == [1, 2, 3] and counts_b[3:9] == [None] * 6 and counts_b[9:] == [1, 2], counts_b


REPLAY = [{0: [4, 5]}, {0: [6], 1: [15]}, {0: [11, 12, 13], 1: [16, 17]}, {1: [0]}, {0: [14, 11], 1: [1, 2]}, {0: [12]}, {0: [7, 8], 1: [18]},
          {0: [4], 1: [19, 15]}]                  # session 0: class A, the other class, A again; session 1: classes 8, 2, 8; uneven pushes


def test_every_listed_pair_follows_a_replay_of_the_three_recurrences_with_restarts_at_gaps(world):
    """Every (session, class) pair the pushes list, A or not, against a host replay driven by the push's `columns` alone: the smoothing
    (y = x at a start, else fl(0.5 y + 0.5 x): with alpha = 0.5 both products are exact, so the one rounding is fmaf's), the baseline
    (reference_baseline over the smoothed scores) and the detector (reference_events over the deviations).  A pair's three states restart
    together wherever it was not listed at the session's previous scoring push, and at nothing else.  Compared: `smoothed` and
    `deviation` of every listed place, `baseline(h)` and `take_events()` after every push."""
    import numpy as np
    from clip_fsar_amd.baseline import Baseline, reference_baseline
    from clip_fsar_amd.events import Event, EventRule, KINDS, ONSET, reference_events
    from clip_fsar_amd.shortlist import Shortlist
    live, ids = world.live, world.live.class_ids
    f, half = np.float32, np.float32(0.5)
    with torch.no_grad():
        base, rule = Baseline(rate=0.25, warm_rate=0.5, warmup=2, gate=3.0), EventRule(on=0.5, off=-0.5, min_on=2, min_off=2)
        p = _pool(live, smooth=0.5, smooth_by="class", baseline=base, events=rule, shortlist=Shortlist(live, keep=3), shortlist_hold=1)
        h = [p.open(), p.open()]
        state, tick = {}, {0: 0, 1: 0}               # (session, class) -> [tick last listed, y, baseline cell, detector cell]
        shown = {"restart": 0, "continue": 0, "events": 0, "z": 0, "pinned": 0}
        for push in REPLAY:
            out = p.push_features({h[i]: _frames(world, c) for i, c in push.items()})
            want_events = []
            for i in push:
                o = out[h[i]]
                tick[i] += 1
                cols, x_all, y_all, z_all = o.columns.tolist(), o.logits.tolist(), o.smoothed.tolist(), o.deviation.tolist()
                shown["pinned"] += sum(1 for b in o.pinned.tolist() if b)
                mine, cells = [], []
                for j, c in enumerate(cols):
                    assert c != NONE
                    key = (i, ids[c])
                    was = state.get(key)
                    if was is None or was[0] != tick[i] - 1:                      # new, or back after a gap: all three start anew
                        shown["restart"] += was is not None and key != (0, A)
                        was = [0, None, None, None]
                    else:
                        shown["continue"] += 1
                    y, ys = was[1], []
                    for row in x_all:
                        y = f(row[j]) if y is None else half * y + half * f(row[j])
                        ys.append(float(y))
                    z, bl = reference_baseline(ys, base, was[2])
                    records, ev = reference_events(z, rule, was[3])
                    assert [repr(r[j]) for r in y_all] == [repr(v) for v in ys], (push, key)
                    assert [repr(r[j]) for r in z_all] == [repr(v) for v in z], (push, key)
                    shown["z"] += sum(v == v for v in z)
                    state[key] = [tick[i], y, bl, ev]
                    cells.append((ids[c], bl.mean, bl.dev, bl.n))
                    for r in records:
                        w = o.first_window + r.k
                        start = w - rule.min_on + 1 if r.kind == ONSET else w - rule.min_off - r.len + 1
                        mine.append((w, j, Event(h[i], ids[c], KINDS[r.kind], w, start, r.len, r.score, r.peak)))
                want_events.extend(e for _, _, e in sorted(mine, key=lambda t: t[:2]))           # window, then column
                assert repr(p.baseline(h[i])) == repr(cells), (push, i)
            got = p.take_events()
            assert repr(got) == repr(want_events), push
            shown["events"] += len(got)
        assert min(shown.values()) > 0, shown          # pairs other than A restarted after a gap, pairs continued, events and pins occurred


def test_the_return_window_is_y_equals_x(world):
    from clip_fsar_amd.shortlist import Shortlist
    live, ids = world.live, world.live.class_ids
    with torch.no_grad():
        p = _pool(live, smooth=0.5, smooth_by="class", shortlist=Shortlist(live, keep=3))
        h = p.open()
        seq = A_CLIPS[:2] + OTHER_CLIPS[:2] + A_CLIPS[2:3]
        outs = [p.push_features({h: _frames(world, [clip])})[h] for clip in seq]
        first, second, back = outs[0], outs[1], outs[4]
        j0, j1, j4 = (_place(o, A, ids) for o in (first, second, back))
        assert _place(outs[2], A, ids) is None and _place(outs[3], A, ids) is None
        assert float(first.smoothed[0, j0]) == float(first.logits[0, j0])
        assert float(second.smoothed[0, j1]) != float(second.logits[0, j1])         # the recurrence runs while the pair is listed
        assert float(back.smoothed[0, j4]) == float(back.logits[0, j4])             # and starts anew after the gap


def test_shortlist_hold_keeps_a_once_selected_class_exactly_two_more_ticks(world):
    from clip_fsar_amd.shortlist import Shortlist, reference_select
    live = world.live
    with torch.no_grad():
        probe = Shortlist(live, keep=3)
        first = reference_select(probe.coarse_features(world.feats[A_CLIPS[0]:A_CLIPS[0] + 1]).cpu(), [1], 3)[0]
        later = [reference_select(probe.coarse_features(world.feats[c:c + 1]).cpu(), [1], 3)[0] for c in OTHER_CLIPS]
        assert all(set(first) != set(l) for l in later)       # stated on the coarse scores: without a hold the list would change at once
        p = _pool(live, shortlist=Shortlist(live, keep=3), shortlist_hold=2)
        h = p.open()
        outs = [p.push_features({h: _frames(world, [clip])})[h] for clip in [A_CLIPS[0]] + OTHER_CLIPS]
        assert outs[0].columns.tolist() == first and outs[0].pinned.tolist() == [0, 0, 0]
        for o in outs[1:3]:                                   # ticks 2 and 3: held, whatever the coarse scores say
            assert o.columns.tolist() == first and o.pinned.tolist() == [HOLD] * 3
        assert outs[3].columns.tolist() == later[2] and outs[3].pinned.tolist() == [0, 0, 0]      # tick 4: on the scores again
        assert outs[4].pinned.tolist() == [HOLD] * 3 and outs[4].columns.tolist() == later[2]      # tick 5: tick 4's own selection is held
        assert p.stats()["pins"] == 9 and p.stats()["pins_dropped"] == 0       # three pins each at ticks 2, 3 and 5


def test_open_with_classes_raises_and_the_store_may_grow_and_reuse_a_slot(world):
    from clip_fsar_amd.live_gallery import LiveGallery
    from clip_fsar_amd.shortlist import Shortlist, reference_select_pinned
    E = world.live.E
    g = torch.Generator().manual_seed(5)
    f = lambda n: torch.randn(n, T, E, generator=g).to(DEV)
    with torch.no_grad():
        live = LiveGallery(world.head, DEV, capacity=8)
        live.add_classes_features(f(7), list(range(7)))
        sl = Shortlist(live, keep=3)
        p = _pool(live, smooth=0.5, smooth_by="class", shortlist=sl, shortlist_hold=1)
        with pytest.raises(ValueError, match=r"open\(classes=\) on a pool with shortlist="):
            p.open(classes=[0, 1])
        h = p.open()
        clips = f(4)

        def push(i):
            pinned = [_cell_pins(p, h, 1)]
            S = Shortlist(live, keep=3).coarse_features(clips[i:i + 1]).cpu()
            want, bits, _ = reference_select_pinned(S, [1], 3, pinned)
            o = p.push_features({h: clips[i].reshape(T, E)})[h]
            ids = live.class_ids
            assert o.columns.tolist() == want[0] and o.pinned.tolist() == bits[0], i
            assert torch.equal(o.logits, live.classify_features(clips[i:i + 1], classes=[ids[c] for c in want[0]]))
            return o

        push(0)
        live.add_classes_features(f(4), [7, 8, 9, 10])            # growth past capacity: the planes grow with the store
        assert live.capacity > 8
        o = push(1)
        assert p._sl_cells.planes[0].shape[1] == live.capacity and HOLD in o.pinned.tolist()       # the held pairs survived the growth
        live.remove_classes([3])
        live.add_classes_features(f(1), [11])                     # "remove 3, add 11" into the freed slot between pushes
        assert live.slot_of(11) is not None
        push(2)
        push(3)


def test_nothing_crosses_between_host_and_device_once_a_shortlist_push_launches(world, monkeypatch):
    """The check of tests/test_gpu_shortlist.py, applied to a push of a pool with a shortlist: from its first launch (the ring write) to
    its return the push makes no torch.tensor(.., device=), no .to / .cuda of a host tensor, no .cpu / .tolist / .item of a device tensor
    and no torch.cuda.synchronize -- with smoothing, a baseline and a rule on, several rounds, and stale coarse rows to refresh."""
    from clip_fsar_amd import pool as pm
    from clip_fsar_amd.baseline import Baseline
    from clip_fsar_amd.events import EventRule
    from clip_fsar_amd.shortlist import Shortlist
    live = world.live
    with torch.no_grad():
        p = _pool(live, smooth=0.5, smooth_by="class", events=EventRule(0.5, -0.5, 1, 1), baseline=Baseline(warmup=2),
                  shortlist=Shortlist(live, keep=3), shortlist_hold=2)
        h = [p.open(), p.open()]
        pushes = [{h[i]: _frames(world, c) for i, c in push.items()} for push in SCHEDULE[:3]]
        state, seen = {"launched": False}, []
        ring_put, tensor, to, cuda = pm.php.ring_put, torch.tensor, torch.Tensor.to, torch.Tensor.cuda

        def watched_ring_put(*a):
            state["launched"] = True
            return ring_put(*a)

        def watched_tensor(*a, **kw):
            if state["launched"] and torch.device(kw.get("device") or "cpu").type != "cpu":
                seen.append("torch.tensor(.., device=)")
            return tensor(*a, **kw)

        def up(name, orig):
            def watched(self, *a, **kw):
                out = orig(self, *a, **kw)
                if state["launched"] and not self.is_cuda and out.is_cuda:
                    seen.append(name)
                return out
            return watched

        def down(name):
            orig = getattr(torch.Tensor, name)

            def watched(self, *a, **kw):
                if state["launched"] and self.is_cuda:
                    seen.append(name)
                return orig(self, *a, **kw)
            return watched

        monkeypatch.setattr(pm.php, "ring_put", watched_ring_put)
        monkeypatch.setattr(torch, "tensor", watched_tensor)
        monkeypatch.setattr(torch.Tensor, "to", up(".to", to))
        monkeypatch.setattr(torch.Tensor, "cuda", up(".cuda", cuda))
        for name in ("cpu", "tolist", "item"):
            monkeypatch.setattr(torch.Tensor, name, down(name))
        monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **kw: seen.append("torch.cuda.synchronize"))
        outs = []
        for push in pushes:
            outs.append(p.push_features(push))
            state["launched"] = False
        assert seen == []
        state["launched"] = True                                                  # the watch itself: it sees each kind of crossing
        torch.tensor([1], device=DEV).tolist()
        torch.zeros(1).to(DEV).cpu()
        assert seen == ["torch.tensor(.., device=)", "tolist", ".to", "cpu"]
        monkeypatch.undo()
        assert len(outs[1][h[1]].class_ids()) == 3 and p.take_events() is not None
