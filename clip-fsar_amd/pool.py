"""Stream pool: window streams that join, leave and push unevenly, classified together against a gallery.

    p = StreamPool(gallery, max_streams=64, stride=2, rate=1, max_push=64, smooth=0.0)   # gallery: SupportGallery or TextGallery
    a, b = p.open(), p.open()              # session handles: ints, never reused; a slot of the ring is reused after close()
    out = p.push({a: fa, b: fb})           # fa [na, 3, H, W], fb [nb, 3, H, W] fp32 on the device; any subset of the open sessions, n >= 1 each
    out[a].first_window, out[a].logits     # a StreamOutput per session: [nWa, C] fp32 (nWa may be 0); .smoothed or None
    po = p.push_packed(frames, sessions=[a, b], counts=[na, nb])    # frames [na + nb, 3, H, W]: the primitive the dict form calls
    po.sessions, po.first_window, po.offsets, po.logits             # logits [sum nW, C], session-major in the order given, windows ascending
    p.push_features({a: feats_a}); p.push_features_packed(feats, sessions, counts)          # [n, E] tower features computed elsewhere
    p.push_u8({a: ua, b: ub}); p.push_u8_packed([ua, ub], [a, b])     # decoded uint8 [n, H, W, 3] clips, each of its own H x W, on the host
                                                                      # or the device: clip_fsar_amd.ingest.FrameIngest, then push_packed
    values, index = p.topk(po, k=5)
    c = p.open(classes=[9, 2])             # a session with columns of its own (a tenant's classes); needs a LiveGallery, and smooth = 0
                                           # unless the pool smooths by class (below)
    out = p.push({a: fa, c: fc})           # out[c].logits [nWc, 2], out[a].logits [nWa, C]: still one tower call sequence, and one grouped
                                           # scoring launch per chunk of windows; the *_packed forms then return a GroupedPackedOutput
    p.enroll(a, class_id=7)                # the session's newest complete window becomes a shot of class 7 (a new class, or a further
                                           # shot of a registered one) out of the ring's tower rows: the tower does not run.  Needs a LiveGallery
    p.enrolable(a)                         # range of the window numbers still in the ring; p.enroll(a, 7, window=w, join=True)
    p.enroll_windows([(a, None, 7), (b, 3, 7), (b, 4, "kite")], text={"kite": "flying a kite"})     # -> {7: 2, "kite": 1}
    p.explain(a, classes=[7], window=None) # the OTAM soft alignment of one window still in the ring against class 7 (or k=3: against its own
                                           # top 3): clip_fsar_amd.align.Alignment; changes nothing of the session.  Needs a LiveGallery
    p.reset(a); p.close(a); p.stats(a); p.stats()
    q = StreamPool(live_gallery, smooth=0.5, smooth_by="class")      # smoothing state per (session, class) instead of per column: class
    c = q.open(classes=[9, 2]); q.enroll(c, "kite", join=True)        # lists, enrolment and removals while sessions run, no reset()
    r = StreamPool(live_gallery, smooth=0.5, smooth_by="class", events=EventRule(on=0.6, off=0.4, min_on=2, min_off=2))
    r.push_features({a: fa}); r.take_events()                         # [Event(session, class_id, kind, window, start, length, score, peak)]
    r.active(a)                                                       # [(class_id, length, peak)] of the session's running events
    z = StreamPool(live_gallery, baseline=Baseline(rate=1 / 32, warmup=16, gate=3.0), events=EventRule(on=4, off=2, min_on=2, min_off=2))
    z.push_features({a: fa})[a].deviation                             # [nW, C]: (score - the pair's mean) / its deviation; the rule judges it
    z.baseline(a)                                                     # [(class_id, mean, dev, n)] of the session's baselines
    t = StreamPool(live_gallery, stride=2, rates=(1, 2, 3))           # every window scored at three frame rates, the best one kept
    o = t.push_features({a: fa})[a]; o.logits, o.tempo, o.rates       # [nW, C] fp32, [nW, C] int32 (index into rates), (1, 2, 3)
    t.enroll(a, "kite", tempo=0); t.explain(a, [7], tempo=1)          # a window of the ring read at rates[0] / rates[1]
    v = StreamPool(live_gallery, events=EventRule(on=0.6, off=0.4), evidence=Evidence(capacity=256))     # clip_fsar_amd.evidence
    e = v.take_events()[0]; v.held(e); v.evidence_features(e)         # an EvidenceEvent; its window's [T, E] rows, long after the ring moved on
    v.explain_event(e); v.enroll_event(e, "kite")                     # explain / enroll on the kept rows, whatever became of the session
    w = StreamPool(gallery, still=StillGate())                        # clip_fsar_amd.still: frames that repeat their predecessor skip the tower
    w.push({a: frames}); w.last_kept()                                # {a: (True, False, ..)}: which frames went through the tower
    k = StreamPool(live_gallery, events=EventRule(on=0.6, off=0.4), contest=Contest(top=1))              # clip_fsar_amd.contest
    k.take_events(); k.leaders(out)                                   # events of a window's best class alone; (columns [nW, top], counts [nW])
    y = StreamPool(live_gallery, stride=2, history=History(frames=4096))                                  # clip_fsar_amd.history
    y.searchable(a); r = y.search([7, "kite"], top=16); r.hits[7]     # [Hit(session, class_id, window, score, tempo)], best first
    y.hit_features(hit); y.explain_hit(hit); y.enroll_hit(hit, "kite")                # on a hit whose window the history still holds
    d = StreamPool(live_gallery, timeline=Timeline(span=16, buckets=256, level=0.6))                      # clip_fsar_amd.timeline
    d.timeline(a).peak; d.recall([7, "kite"], top=16).hits[7]         # [buckets, C] per-bucket peaks; [Hit(..)] of the best buckets

clip_fsar_amd.stream.WindowStream serves a fixed set of streams that advance in lockstep.  Here every session numbers its own frames from 0
at open() or reset(): window k of a session holds its frames k * stride + j * rate, j = 0 .. T-1, and is emitted once, in order, by the push
that delivers its last frame (stream.window_plan per session).  The tower is per frame and a window's scores depend on its own T frames
alone, so the frames of unrelated sessions share one tower call sequence and their windows share context2 and the gallery launch: a
window's logits are what gallery.classify returns for its clip, in the gallery's own mode.

A push is described to the device by one descriptor table with a row per session (libclipfsar_pool.so, clip_fsar_amd.pool_hip): one ring
write per round, one gather plus one classify_features per chunk of windows, whatever the number of sessions.  A session's push beyond
max_push frames is split into rounds (round r takes up to max_push of what each session has left).  Sessions absent from a push are
untouched.  Smoothing state is per session: y_0 = x_0, y_k = fmaf(alpha, y_{k-1}, (1 - alpha) * x_k), the bits of WindowStream's.

smooth_by="class" (a LiveGallery or LiveTextGallery): the state is [max_streams, store capacity], a cell per (session slot, class store
slot), and beside every cell lies the generation the store slot had when the cell was written (LiveGallery.slot_generations).  A cell
continues the recurrence iff that mark is the slot's current generation, so a pair starts anew (y = x) at its first window after the
session's open() or reset() (the session's row of marks is zeroed), after the class's registration (the gallery bumps the generation of
a slot that was freed or changed owner), and after the class joined the session's list -- and at nothing else: other classes coming and
going, further shots, store growth and other sessions leave it alone.  One launch per push (libclipfsar_class_smooth.so,
clip_fsar_amd.class_smooth_hip), once the push's logits are in session-major order; the bits are the column mode's where both apply.

events=EventRule(...) (clip_fsar_amd.events; a LiveGallery or LiveTextGallery): every push that completes a window also runs a hysteresis
detector over each (session, class) pair's scores -- the smoothed ones when the pool smooths by class, the logits or probabilities
otherwise -- on the device (libclipfsar_events.so, clip_fsar_amd.events_hip: one call per push, on the session-major scores, over the
descriptor table and key lists of the class mode, which are then planned and uploaded once for both).  Its state is the pool's own, keyed
and guarded like the class mode's, so events run through class lists, enrolment, join=True, removals and slot reuse; a removed class and a
closed or reset session end their events silently.  The push returns what it returns without a rule and does not synchronise: it queues
the device's records with the metadata fixed at push time, and take_events() synchronises once and returns the Events push by push,
within a push in session order as pushed, then window, then column.  The queue holds EVENT_QUEUE pushes; a push onto a full queue
translates the oldest batch itself (one synchronisation) and keeps its events for the next take_events().  Records beyond the rule's
max_events per push are dropped with a RuntimeWarning and counted in stats()["events_dropped"].

baseline=Baseline(...) (clip_fsar_amd.baseline; a LiveGallery or LiveTextGallery): every push that completes a window also runs one
launch (libclipfsar_baseline.so, clip_fsar_amd.baseline_hip) over the same session-major scores a rule would judge, after smoothing and
before the detector, over the same table, keys and generations: each (session, class) pair keeps a running mean and mean absolute
deviation of its own scores in cells keyed and guarded like the class mode's, and the push's output carries `deviation`, z = (score -
mean) / deviation in the layout of logits, NaN through the pair's warm-up.  The outputs are then instances of subclasses of PackedOutput,
GroupedPackedOutput and StreamOutput with the same tuple contents and that one attribute more.  With events= as well the detector judges
z: the rule's thresholds are in units of the pair's own deviation and an Event's score and peak are deviations.  baseline(h) lists a
session's cells.

shortlist=Shortlist(gallery, keep=K) (clip_fsar_amd.shortlist; the pool's LiveGallery), shortlist_hold=H: every session's windows of a push
are one group of the shortlist's stages -- coarse scores over every class, then the exact kernel on K of them -- and smoothing, baselines
and the detector run over the selected slot lists.  The selection is libclipfsar_pool_select.so's (clip_fsar_amd.pool_select_hip): a
(session, class) pair that was scored at the session's previous scoring push stays listed ("pinned") while its event is running or its
onset streak is counting, and for H further pushes after it was selected on its score; a pair that was not scored at the previous
scoring push has its marks zeroed by the selection, so it starts anew in all three states, as a newly enrolled class does.  Outputs are
subclasses of PackedOutput / StreamOutput over the K listed classes with .columns (indices into gallery.class_ids, ascending, NONE = no
class), .pinned and .class_ids(); stats() gains "pins" and "pins_dropped"; active() and baseline() list the pairs scored at the session's
last scoring push.  keep >= len(gallery) is the pool without a shortlist, bit for bit.  open(classes=) and enroll(join=True) are refused.

rates=(r_0 < .. < r_{R-1}) (1 to 8 integers; a SupportGallery or a LiveGallery; `rate` stays at its default): the pool plans, sizes its
ring and numbers its windows exactly as a pool with rate = rmax = r_{R-1}.  Window k is completed by frame e_k = k * stride + (T - 1) *
rmax, and its TEMPO i is the T frames e_k - (T - 1 - j) * r_i, j < T: every tempo ends on the window's newest frame, so all complete in
the same push, and tempo R - 1 is the window of the rate = rmax pool.  The tower runs once per frame as before; per chunk of windows one
gather reads the R sequences of every window out of the ring (libclipfsar_tempo.so, clip_fsar_amd.tempo_hip, over the pool's own
descriptor table), classify_features scores them, and one launch reduces the R scores of every (window, class) cell to their maximum --
`logits` -- and the index of the tempo that gave it -- `tempo`, int32 in the layout of logits; ties go to the lowest index, and a NaN
among the R scores stays a NaN (reference_reduce restates the rule).  Smoothing, baselines, the detector, topk and stats() run on the
reduced scores unchanged.  The outputs are subclasses of PackedOutput / StreamOutput (and of their Deviation forms) with .tempo and
.rates.  enroll, enroll_windows and explain take tempo=, the index into rates at which a window of the ring is read (None: the last).
open(classes=) and shortlist= are refused, and so is a TextGallery or LiveTextGallery.

evidence=Evidence(capacity, kinds) (clip_fsar_amd.evidence; needs events=): the push that detects an event of one of `kinds` also copies
the T ring rows of the event's window into a slot of a device store (libclipfsar_evidence.so, clip_fsar_amd.evidence_hip: two launches
right behind the detector's, driven by its records on the device, no synchronisation; with rates= the window is read at the tempo that
won the event's cell).  take_events() then returns EvidenceEvents -- Event's fields, then `evidence` (the capture's serial, or None),
`missed` (None, "ring": a later round of the same push had overwritten the window, "capacity": more than `capacity` captures in one
push, "kind") and `tempo` -- and still synchronises once: the capture's answers come down with the records.  Serial s lives in slot
s mod capacity and is held until `capacity` later captures have overwritten it, through close(), reset() and any number of pushes;
held(e), evidence_features(e), explain_event(e) and enroll_event(e, class_id) work on it (each first translates the queued pushes, its
one synchronisation; take_events() still returns their events).  stats() gains "evidence" and "evidence_missed".

still=StillGate(pixel_tol, changed, max_run) (clip_fsar_amd.still, which states the measure, the predecessor and the rule): a pixel push
(push, push_packed, push_u8, push_u8_packed) first counts, per frame, the elements that differ from the frame before it by more than
pixel_tol (libclipfsar_still.so, clip_fsar_amd.still_hip); frames with at most changed * L such elements skip the tower and take the
tower row of their predecessor -- within the push, or the ring row of the session's newest frame before it.  The counts come to the host
(the gate's one synchronisation per push: the tower call is sized there), plan_still decides, the kept frames are packed, the tower runs
on them alone, their rows are expanded to a row per frame, and _run receives what push_features_packed would: rounds, rates=, shortlist=,
smoothing, baselines, events, evidence, enrolment and explain see no difference, and frame numbers stay.  open(), reset() and a feature
push leave a session without a predecessor: its next frame goes through the tower whatever it holds.  stats() gains "still_frames",
tower_frames counts the frames the tower really saw, last_kept() tells them apart.  One frame geometry per pool.

contest=Contest(top, margin) (clip_fsar_amd.contest, which states the rule; needs events=): between the judged scores of a push -- after
smoothing and the baseline -- and the detector, one launch (libclipfsar_contest.so, clip_fsar_amd.contest_hip, over the table and keys the
detector takes) ranks every window's row: the `top` highest candidates lead, ties to the lower column, and with `margin` none further than
that below the window's best; every other candidate reaches the detector as -inf.  An idle pair that is demoted loses its streak, a running
event counts a window below `off` and ends after min_off windows out of the leaders -- with an OFFSET whose score is -inf.  Nothing but the
detector sees that plane: the push returns the bits it returns without the option (a shortlist pool's pins follow the detector's cells, so an
outranked pair's pin lapses with its event).  leaders(out) recomputes a push's leading columns on the device.  The stage keeps no state.

history=History(frames=F) (clip_fsar_amd.history, which states the store, the plane and the peak rule; a LiveGallery): a store
[max_streams, F, E] that outlives the ring, F >= cap, made by the first push; every round of every push writes its rows there right beside
the ring write, with the ring's own kernel (cfsp_ring_put, the store as its ring: frame f at [slot, f mod F]).  The push returns the bits it
returns without the option.  searchable(h) is enrolable_windows over F; search(classes, ...) gathers the held windows of the open sessions
asked for (cfsp_window_sequences over one table, the store as its ring), scores them with classify_features(classes=) chunk by chunk into
a plane [NW, K] and runs libclipfsar_history.so (clip_fsar_amd.history_hip, two launches over the gather's table) on it: per class the
local maxima within `separation` windows of one session -- a local-maximum filter, not greedy suppression; a plateau yields its first
window -- and of those the `top` highest across sessions.  It synchronises once, to read the hit records.  hit_features, explain_hit and
enroll_hit read a hit's window out of the store the way enroll and explain read the ring.  The option adds nothing to stats().

timeline=Timeline(span, buckets, level, of) (clip_fsar_amd.timeline, which states the buckets, the cells and the fold; a LiveGallery or
LiveTextGallery): every push that completes a window also runs one launch (libclipfsar_timeline.so, clip_fsar_amd.timeline_hip) over
the judged scores -- after smoothing and the baseline, before the contest; or the plane `of` names -- over the table, keys and
generations every keyed launch of the push takes, the sessions' first window numbers riding in the same upload: per (session, bucket of
`span` windows, class) the peak score, the peak's window and the count of windows at or above `level`, in cells [max_streams, buckets,
store capacity] keyed and guarded like the class mode's, a ring of `buckets` buckets per pair.  The push returns the bits it returns
without the option.  timeline(h) reads a session's held buckets (one launch, no synchronisation); recall(classes, ...) reads the held
buckets of the sessions asked for into a plane of bucket peaks and runs the history's peak search on it: hours of scores in three
launches and no scoring, its hits' windows the pool's own.  shortlist= is refused.  The option adds nothing to stats().

Enrolment: a session's ring holds the tower rows of its last cap frames, and a support sequence is T tower rows plus the class's text row.
enroll / enroll_windows turn windows that are still in the ring into shots (libclipfsar_enroll.so, clip_fsar_amd.enroll_hip: one copy
launch per kind, new classes and further shots) and hand the sequences to the LiveGallery's registration from sequences.  Nothing of the
sessions changes: counters, ring, stats and smoothing state stay.
"""
from __future__ import annotations

import collections
import heapq
import warnings

import torch

from . import baseline_hip as blhip
from . import class_smooth_hip as cship
from . import contest_hip as cthip
from . import enroll_hip as enhip
from . import evidence_hip as edhip
from . import events_hip as evhip
from . import gallery_hip as ghip
from . import groups_hip as grhip
from . import history_hip as hship
from . import pool_hip as php
from . import pool_select_hip as pship
from . import still_hip as skhip
from . import tempo_hip as tphip
from . import timeline_hip as tlhip
from .baseline import Baseline
from .contest import Contest
from .events import EventRule, translate
from .evidence import MISSED, Evidence, EvidenceEvent, keep0
from .gallery import _GalleryBase
from .history import (History, Hit, SearchResult, check_min_score, check_separation, check_top, device_separation, largest_frames,
                      plan_search)
from .ingest import FrameIngest
from .still import StillGate, plan_still
from .stream import StreamOutput, window_plan
from .timeline import RecallHit, RecallResult, Timeline, TimelineView, held_buckets, read_rows

PackedOutput = collections.namedtuple("PackedOutput", "sessions first_window offsets logits smoothed")
# Of a push in which a session has a class list of its own: logits is flat, session i owning [logit_offsets[i], logit_offsets[i + 1]) as
# a row-major [offsets[i + 1] - offsets[i], widths[i]] block (windows ascending).
# smoothed: of a pool with smooth_by="class", flat in the layout of logits; None otherwise.
GroupedPackedOutput = collections.namedtuple("GroupedPackedOutput", "sessions first_window offsets logits logit_offsets widths smoothed",
                                             defaults=(None,))


def _class_ids(self):
    """the class ids behind `columns` (None where a place holds no class), per session of a packed output.  Synchronises."""
    rows = self.columns.cpu().tolist()
    name = lambda row: [self._ids[c] if c != pship.NONE else None for c in row]
    return name(rows) if self.columns.dim() == 1 else [name(row) for row in rows]


# What an option adds to a push's output: a prefix of the type's name, the keyword-only extras its constructor takes and the instance
# holds beside the tuple (`ids` as ._ids), the type's docstring and its methods.
#   Shortlist: logits, smoothed (and deviation) are [nW, K]; columns and pinned are int32 on the device, [K] of a session's output and
#     [sessions of the push, K] of a packed one; columns: indices into gallery.class_ids as of the push, ascending, NONE where the list
#     is shorter (every place of a session without windows); pinned: the place's PIN_* bits, 0: selected on its score
#   Tempo: tempo is int32 on the device in the layout of .logits, per cell the index into `rates`, the pool's tuple, of the tempo
#     whose score .logits holds
_EXTRAS = {
    "Shortlist": (("columns", "pinned", "ids"), "%s of a pool with a shortlist: the same tuple over the K listed classes, .columns, "
                  ".pinned and .class_ids()", {"class_ids": _class_ids}),
    "Tempo": (("tempo", "rates"), "%s of a pool with rates=: the same tuple, .tempo in the layout of .logits and .rates", {}),
    "Deviation": (("deviation",), "%s of a pool with a baseline: the same tuple, and .deviation in the layout of .logits (NaN through "
                  "warm-up)", {}),
}
_OUTPUT_TYPES = {t.__name__: t for t in (PackedOutput, GroupedPackedOutput, StreamOutput)}


def _extended(prefix, base):
    """the output type `prefix` + `base`'s name: a subclass of `base` with the same tuple whose constructor takes the option's extras by
    keyword and hands every other keyword on to `base`"""
    extras, doc, methods = _EXTRAS[prefix]

    def __new__(cls, *fields, **more):
        missing = [k for k in extras if k not in more]
        if missing:
            raise TypeError("%s() needs the keyword-only arguments %s" % (cls.__name__, ", ".join(missing)))
        mine = [more.pop(k) for k in extras]
        self = base.__new__(cls, *fields, **more)
        for k, v in zip(extras, mine):
            setattr(self, "_ids" if k == "ids" else k, v)
        return self
    t = type(prefix + base.__name__, (base,), dict(methods, __new__=__new__, __doc__=doc % base.__name__, __module__=__name__))
    _OUTPUT_TYPES[t.__name__] = t
    return t


DeviationPackedOutput = _extended("Deviation", PackedOutput)
DeviationGroupedPackedOutput = _extended("Deviation", GroupedPackedOutput)
DeviationStreamOutput = _extended("Deviation", StreamOutput)
ShortlistPackedOutput = _extended("Shortlist", PackedOutput)
ShortlistStreamOutput = _extended("Shortlist", StreamOutput)
DeviationShortlistPackedOutput = _extended("Deviation", ShortlistPackedOutput)
DeviationShortlistStreamOutput = _extended("Deviation", ShortlistStreamOutput)
TempoPackedOutput = _extended("Tempo", PackedOutput)
TempoStreamOutput = _extended("Tempo", StreamOutput)
DeviationTempoPackedOutput = _extended("Deviation", TempoPackedOutput)
DeviationTempoStreamOutput = _extended("Deviation", TempoStreamOutput)


def _output(base, *fields, deviation=None, tempo=None, rates=None, columns=None, pinned=None, ids=None):
    """the output of a push or of one of its sessions: `base` (PackedOutput, GroupedPackedOutput or StreamOutput) over `fields` when no
    extra is given, else the subclass the extras present name, holding them"""
    name, more = base.__name__, {}
    if columns is not None:
        name, more = "Shortlist" + name, dict(columns=columns, pinned=pinned, ids=ids)
    if tempo is not None:
        name, more = "Tempo" + name, dict(tempo=tempo, rates=rates)
    if deviation is not None:
        name, more = "Deviation" + name, dict(more, deviation=deviation)
    return _OUTPUT_TYPES[name](*fields, **more)


# One round of a push.  rows: the descriptor table, a row per session that still has frames (pool_hip's column order); members: the
# position of each row's session in the push; src: (first row, n) of each row's frames in the push's packed frames.
Round = collections.namedtuple("Round", "rows members src")
Plan = collections.namedtuple("Plan", "rounds first_window n_windows order")
# What a push with an event rule queues: buf, the device's int32 answer (n_events, then the events and values of events_hip.detect), and
# the metadata fixed at push time, per table row: the session's handle, its first window of the push and its columns' class ids.
# columns: of a pool with a shortlist, the push's sel_cols [rows, K] on the device -- a record's column is a place of that list, and
# class_ids then holds per row the gallery's class ids of that push, which the place's column indexes; None otherwise.
EventBatch = collections.namedtuple("EventBatch", "buf sessions first_window class_ids columns", defaults=(None,))
EVENT_QUEUE = 64                                  # pushes whose records may wait for take_events()


def plan_push(sessions, counts, T, stride, rate, max_push, smoothing=False):
    """The host plan of one push.  sessions: (ring slot, frames pushed so far) per session, counts: frames each pushes now.
    -> Plan(rounds, first_window and n_windows per session, order).  The windows come off the device round-major (every round
    session-major); order[i] is the position there of row i of the session-major result, or None when the two orders agree."""
    cap = (T - 1) * rate + max_push
    first_window = [window_plan(t, 0, T, stride, rate)[0] for _, t in sessions]
    starts = [0]
    for n in counts:
        starts.append(starts[-1] + n)
    rounds, done, where = [], [0] * len(sessions), [[] for _ in sessions]
    emitted = 0
    while any(d < n for d, n in zip(done, counts)):
        rows, members, src = [], [], []
        feat_off = win_off = 0
        for i, ((slot, t0), total) in enumerate(zip(sessions, counts)):
            n = min(max_push, total - done[i])
            if n <= 0:
                continue
            t = t0 + done[i]
            first, nW = window_plan(t, n, T, stride, rate)
            rows.append([slot, t % cap, n, feat_off, (first * stride) % cap, nW, win_off, int(bool(smoothing) and first > 0)])
            members.append(i)
            src.append((starts[i] + done[i], n))
            where[i].extend(range(emitted + win_off, emitted + win_off + nW))
            feat_off, win_off = feat_off + n, win_off + nW
            done[i] += n
        emitted += win_off
        rounds.append(Round(rows, members, src))
    order = [g for w in where for g in w]
    return Plan(rounds, first_window, [len(w) for w in where], None if order == list(range(len(order))) else order)


def enrolable_windows(t, T, stride, rate, cap):
    """The windows of a session with t frames since open() / reset() that can still be enrolled, as a range.  The ring holds the frames
    [max(0, t - cap), t); window w is the frames w * stride + j * rate, j = 0 .. T-1.  Enrolable: complete (w below the windows t frames
    complete) and its first frame retained (w * stride >= t - cap).  With stride <= max_push the newest complete window always is."""
    nW = window_plan(0, t, T, stride, rate)[1]
    lo = -(-max(0, t - cap) // stride)
    return range(lo, nW) if lo < nW else range(0)


EnrollPlan = collections.namedtuple("EnrollPlan", "windows slots positions")


def plan_enroll(sessions, requests, T, stride, rate, cap, names=None):
    """The host plan of an enrolment.  sessions: (ring slot, frames pushed so far) per session; requests: (index into sessions, window
    number or None: the session's newest complete window) -> EnrollPlan: per request the window number, the ring slot and the ring
    position (w * stride) mod cap of the window's first frame.  Raises ValueError on a window that is not enrolable (names: what to call
    each session in the message); changes nothing."""
    windows, slots, positions = [], [], []
    for i, w in requests:
        slot, t = sessions[i]
        ok = enrolable_windows(t, T, stride, rate, cap)
        asked = w
        if w is None:
            w = window_plan(0, t, T, stride, rate)[1] - 1
        if isinstance(w, bool) or not isinstance(w, int) or w not in ok:
            w = "None (the newest complete one)" if asked is None else repr(w)
            raise ValueError("%s: window %s is not enrolable -- the ring holds its windows %r (%d frames since open() / reset(), cap = %d)"
                             % (names[i] if names else "session %d" % i, w, ok, t, cap))
        windows.append(w)
        slots.append(slot)
        positions.append((w * stride) % cap)
    return EnrollPlan(windows, slots, positions)


def tempo_positions(win_pos, w, stride, T, rates, cap):
    """The ring rows of every tempo of window w of a table row whose WIN_POS is win_pos (the first frame of the row's first window in its
    rmax = rates[-1] form): [[row of frame j, j < T] per tempo i].  Tempo i holds the frames e - (T - 1 - j) * rates[i] with e the frame
    that completes the window, so its first frame lies (T - 1) * (rmax - rates[i]) behind the rmax form's first."""
    rmax = rates[-1]
    return [[(win_pos + w * stride + (T - 1) * (rmax - r) + j * r) % cap for j in range(T)] for r in rates]


def reference_reduce(scores, R):
    """cftp_reduce in torch (CPU tensors too): scores [NW * R, C], rows ordered (window, tempo) -> (out [NW, C], tempo [NW, C] int32).
    Per cell the largest of the R scores and the lowest index that holds it; when one of them is NaN, the first NaN and its index.  out
    is one of the inputs bit for bit."""
    scores = torch.as_tensor(scores, dtype=torch.float32)
    if scores.dim() != 2 or R < 1 or scores.shape[0] % R:
        raise ValueError("reference_reduce: scores must be [NW * R, C] with R = %d >= 1, got %s" % (R, tuple(scores.shape)))
    s = scores.view(scores.shape[0] // R, R, scores.shape[1])
    best = s[:, 0].clone()
    at = torch.zeros(best.shape, dtype=torch.int32, device=scores.device)
    for i in range(1, R):
        v = s[:, i]
        better = ~torch.isnan(best) & ((v > best) | torch.isnan(v))
        best = torch.where(better, v, best)
        at = torch.where(better, torch.full_like(at, i), at)
    return best, at


class _Session:
    __slots__ = ("slot", "t", "tower_frames", "state_gen", "state_layout", "classes", "tick")

    def __init__(self, slot, classes=None):
        self.slot = slot
        self.classes = classes                   # the session's own class list (open(classes=)), or None: every class; reset() keeps it
        self.clear()

    def clear(self):
        self.t = 0                               # frames pushed since open() / reset()
        self.tick = 0                            # scoring pushes (pushes that completed a window) since then: a shortlist pool's clock
        self.tower_frames = 0
        self.state_gen = None                    # generation of the pool's smoothing buffer this session's state row was written in
        self.state_layout = None                 # the gallery's layout_version then (None: a gallery whose columns never change meaning)


class _Cells:
    """A keyed cell store: planes [max_streams, store capacity], a cell per (session slot, class store slot), made by the first push
    that needs them.  dtypes: a plane each; guard: the indices of the planes that say whether a cell holds anything -- the generation
    marks, or a shortlist's two clocks -- which are made zero-filled and whose rows of the slots in `forgotten` (sessions opened or
    reset since the last push) are zeroed by the next push; the other planes are read behind a guard alone and are made uninitialised."""

    def __init__(self, dev, max_streams, dtypes, guard, limit, what):
        self.dev, self.max_streams, self.dtypes, self.guard, self.limit, self.what = dev, max_streams, dtypes, guard, limit, what
        self.planes = None
        self.forgotten = set()

    @staticmethod
    def too_many(max_streams, cap, what):
        return ("StreamPool: %s keeps a state cell per (session slot, store slot): max_streams = %d x store capacity = %d "
                "is 2^31 or more -- build the pool with fewer streams or the gallery with fewer slots" % (what, max_streams, cap))

    def at(self, cap):
        """the planes at store capacity `cap`; a grown store: reallocated with their columns copied, the guards' new columns 0.  The
        forgotten slots' rows of the guards are zeroed here, on the push's stream."""
        if self.max_streams * cap > self.limit:
            raise ValueError(self.too_many(self.max_streams, cap, self.what))
        old = None if self.planes is None else self.planes[0].shape[1]
        if old != cap:
            new = tuple((torch.zeros if i in self.guard else torch.empty)(self.max_streams, cap, device=self.dev, dtype=dtype)
                        for i, dtype in enumerate(self.dtypes))
            if old is not None:
                for t, was in zip(new, self.planes):
                    t[:, :old].copy_(was)
            self.planes = new
        for slot in sorted(self.forgotten):
            for i in self.guard:
                self.planes[i][slot].zero_()
        self.forgotten.clear()
        return self.planes


class _Buckets:
    """_Cells' sibling with a ring of B buckets between the two keys: the timeline's planes [max_streams, B, store capacity] -- peak
    fp32, at, above and marks int32 --, made by the first push that folds.  The marks are the guard: made zero-filled, a grown store's
    new columns zero, and the planes [slot] of the slots in `forgotten` zeroed by the next use; the others are read behind it alone."""

    def __init__(self, dev, max_streams, B):
        self.dev, self.max_streams, self.B = dev, max_streams, B
        self.planes = None
        self.forgotten = set()

    @staticmethod
    def too_many(max_streams, B, cap):
        return ("StreamPool: timeline= keeps a state cell per (session slot, bucket, store slot): max_streams = %d x buckets = %d x "
                "store capacity = %d is 2^31 or more -- build the pool with fewer streams or buckets or the gallery with fewer slots"
                % (max_streams, B, cap))

    def at(self, cap):
        if self.max_streams * self.B * cap > tlhip.MAX_CELLS:
            raise ValueError(self.too_many(self.max_streams, self.B, cap))
        old = None if self.planes is None else self.planes[0].shape[2]
        if old != cap:
            f32, i32 = torch.float32, torch.int32
            new = tuple((torch.zeros if i == 3 else torch.empty)(self.max_streams, self.B, cap, device=self.dev, dtype=dtype)
                        for i, dtype in enumerate((f32, i32, i32, i32)))
            if old is not None:
                for t, was in zip(new, self.planes):
                    t[:, :, :old].copy_(was)
            self.planes = new
        for slot in sorted(self.forgotten):
            self.planes[3][slot].zero_()
        self.forgotten.clear()
        return self.planes


class StreamPool:
    def __init__(self, gallery, max_streams=64, stride=1, rate=1, max_push=64, smooth=0.0, ingest=None, smooth_by="column",
                 *positional, shortlist=None, shortlist_hold=None, rates=None, evidence=None, still=None, contest=None, history=None,
                 timeline=None, events=None, baseline=None):
        # shortlist=, shortlist_hold=, rates=, evidence=, still=, contest=, history= and timeline= are keyword-only.  events and baseline were the 9th and 10th positional parameters before the two
        # existed and still are: `positional` takes them, so no earlier call changes its meaning.
        if len(positional) > 2 or (positional and events is not None) or (len(positional) > 1 and baseline is not None):
            raise TypeError("StreamPool: at most 10 positional arguments (.., smooth_by, events, baseline), and neither of the last two "
                            "by keyword as well; got %d positional" % (8 + len(positional)))
        events = positional[0] if positional else events
        baseline = positional[1] if len(positional) > 1 else baseline
        if not isinstance(gallery, _GalleryBase):
            raise TypeError("StreamPool: gallery must be a SupportGallery or a TextGallery, got %s" % type(gallery).__name__)
        for name, v in (("max_streams", max_streams), ("stride", stride), ("rate", rate), ("max_push", max_push)):
            if isinstance(v, bool) or not isinstance(v, int) or v < 1:
                raise ValueError("StreamPool: %s must be an integer >= 1, got %r" % (name, v))
        if max_streams > php.MAX_STREAMS:
            raise ValueError("StreamPool: max_streams = %d, the pool library serves at most %d" % (max_streams, php.MAX_STREAMS))
        if rates is not None:
            rates, rate = self._check_rates(gallery, rates, rate, shortlist), rates[-1]
        smooth = float(smooth)
        if not 0.0 <= smooth < 1.0:
            raise ValueError("StreamPool: smooth must be in [0, 1), got %r" % smooth)
        if gallery.T > php.MAX_T:
            raise ValueError("StreamPool: T = %d frames per window, the pool library gathers at most %d" % (gallery.T, php.MAX_T))
        if smooth_by not in ("column", "class"):
            raise ValueError("StreamPool: smooth_by must be \"column\" or \"class\", got %r" % (smooth_by,))
        if smooth_by == "class" and not hasattr(gallery, "slot_generations"):
            raise ValueError("StreamPool: smooth_by=\"class\" needs a gallery with a slot store (a LiveGallery or a LiveTextGallery), not a %s"
                             % type(gallery).__name__)
        if smooth_by == "class" and smooth and max_streams * gallery.capacity > cship.MAX_CELLS:
            raise ValueError(_Cells.too_many(max_streams, gallery.capacity, "smooth_by=\"class\""))

        def keyed(what, why, limit, slot_store=True):
            """what an option that keeps a cell per (session slot, store slot) asks of the pool: `what` names the option, `why` says
            what its state is keyed by, `limit` is its library's MAX_CELLS"""
            if slot_store and not hasattr(gallery, "slot_generations"):
                raise ValueError("StreamPool: %s needs a gallery with a slot store (a LiveGallery or a LiveTextGallery), not a %s"
                                 % (what, type(gallery).__name__))
            if smooth and smooth_by == "column":
                raise ValueError("StreamPool: %s on a pool with smooth > 0 needs smooth_by=\"class\" -- the column mode's state is "
                                 "keyed by column, %s" % (what, why))
            if max_streams * gallery.capacity > limit:
                raise ValueError(_Cells.too_many(max_streams, gallery.capacity, what))
        if events is not None:
            if not isinstance(events, EventRule):
                raise TypeError("StreamPool: events must be an EventRule, got %s" % type(events).__name__)
            keyed("events=", "the detector's by class", evhip.MAX_CELLS)
        if evidence is not None:
            if not isinstance(evidence, Evidence):
                raise TypeError("StreamPool: evidence must be an Evidence, got %s" % type(evidence).__name__)
            if events is None:
                raise ValueError("StreamPool: evidence= is given without events= -- evidence is the window behind an event; build the "
                                 "pool with events=EventRule(...) as well")
        if still is not None and not isinstance(still, StillGate):
            raise TypeError("StreamPool: still must be a StillGate, got %s" % type(still).__name__)
        if contest is not None:
            if not isinstance(contest, Contest):
                raise TypeError("StreamPool: contest must be a Contest, got %s" % type(contest).__name__)
            if events is None:
                raise ValueError("StreamPool: contest= is given without events= -- the contest decides which classes of a window reach "
                                 "the detector; build the pool with events=EventRule(...) as well")
        if history is not None:
            self._check_history(gallery, history, (gallery.T - 1) * rate + max_push, max_streams)
        if timeline is not None:
            self._check_timeline(gallery, timeline, max_streams, shortlist, smooth_by == "class" and bool(smooth), baseline)
        if baseline is not None:
            if not isinstance(baseline, Baseline):
                raise TypeError("StreamPool: baseline must be a Baseline, got %s" % type(baseline).__name__)
            keyed("baseline=", "the baseline's by class", blhip.MAX_CELLS)
        if shortlist is None and shortlist_hold is not None:
            raise ValueError("StreamPool: shortlist_hold = %r is given without shortlist= -- there is no list to hold a class in"
                             % (shortlist_hold,))
        if shortlist is not None:
            from .shortlist import Shortlist
            if not isinstance(shortlist, Shortlist):
                raise TypeError("StreamPool: shortlist must be a Shortlist, got %s" % type(shortlist).__name__)
            if shortlist.gallery is not gallery:
                raise ValueError("StreamPool: shortlist= was built over another gallery -- shortlist.gallery must be the pool's gallery")
            keyed("shortlist=", "and a shortlist's columns change with every push", pship.MAX_CELLS, slot_store=False)
            hold = 0 if shortlist_hold is None else shortlist_hold
            if isinstance(hold, bool) or not isinstance(hold, int) or not 0 <= hold <= pship.MAX_HOLD:
                raise ValueError("StreamPool: shortlist_hold must be an integer in [0, 2^20], got %r" % (shortlist_hold,))
        self.smooth_by = smooth_by
        self._by_class = smooth_by == "class" and bool(smooth)     # with smooth = 0 the option is inert
        self.gallery = gallery
        self.dev = gallery.dev
        self.max_streams, self.stride, self.rate, self.max_push, self.alpha = max_streams, stride, rate, max_push, smooth
        self.rates = rates                       # the tempo pool's rates, ascending (self.rate is the largest of them), or None
        self.T, self.E = gallery.T, gallery.E
        self.cap = (self.T - 1) * rate + max_push
        self._ring = torch.empty(max_streams, self.cap, self.E, device=self.dev, dtype=torch.float32)
        self._X = None                           # gathered windows [rows, T, E], grown on demand
        self._state = None                       # the column mode's smoothing state [max_streams, C], indexed by slot
        self._state_gen = 0                      # bumped whenever _state is allocated anew (the class count changed)
        self._stores = []                        # the keyed cell stores of the options given; open() and reset() walk them
        i32, f32 = torch.int32, torch.float32

        def cells(dtypes, guard, limit, what):
            self._stores.append(_Cells(self.dev, max_streams, dtypes, guard, limit, what))
            return self._stores[-1]
        # smooth_by="class": (state, marks) by (slot, store slot), the marks the generations beside the state; None: nothing is kept
        self._smooth_cells = cells((f32, i32), (1,), cship.MAX_CELLS, "smooth_by=\"class\"") if self._by_class else None
        self._smooth_tables = None               # class_smooth_hip's descriptor tables, made by the first class-mode push
        self._smooth_keys = (None, None, None)   # the last push's own store-slot lists, the gallery's column list then, their device form
        self._tables = php.TableUploader(self.dev, max_streams)
        self._enroll_tables = None               # enrolment lists (enroll_hip's row layout), made by the first enroll
        self._sessions = {}                      # handle -> _Session
        self._free = list(range(max_streams))    # a heap: the lowest free slot is taken first
        self._next_handle = 0
        self._totals = {"frames": 0, "tower_frames": 0, "windows": 0}
        self._events = events                    # the EventRule, or None: nothing below is there
        if events is not None:
            self._totals.update(events=0, events_dropped=0)
            self._ev_cells = cells((i32, i32, f32, i32), (3,), evhip.MAX_CELLS, "events=")       # (streak, length, peak, marks)
            self._ev_work = None                 # events_hip.detect's workspace, grown on demand
            self._ev_queue = collections.deque() # EventBatch per push that ran the detector, oldest first
            self._ev_ready = []                  # Events of batches a push had to translate itself
            self._ev_ids = (None, None)          # (layout_version, class count) and the gallery's class ids then
        self._evidence = evidence                # the Evidence, or None: nothing below is there
        if evidence is not None:
            self._totals.update(evidence=0, evidence_missed=0)
            self._ed_store = None                # [capacity, T, E] fp32, with _ed_head [1] int32 and _ed_work: made by the first push that detects
            self._ed_head = self._ed_work = self._ed_tables = None
            self._ed_captured = 0                # captures translated so far: the next serial
            # the type of this pool's events: EvidenceEvent under its own name, so that an event says which pool's store holds its window
            self._event_type = type("EvidenceEvent", (EvidenceEvent,), {"__slots__": (), "__doc__": EvidenceEvent.__doc__})
        self._contest_rule = contest             # the Contest, or None: nothing below is there
        if contest is not None:
            self._ct_work = None                 # contest_hip.contest's workspace, grown on demand
            self._ct_tables = None               # the descriptor tables of leaders(), made by its first call
        self._shortlist = shortlist              # the Shortlist, or None: nothing below is there
        if shortlist is not None:
            self._hold = hold
            self._totals.update(pins=0, pins_dropped=0)
            self._sl_cells = cells((i32, i32), (0, 1), pship.MAX_CELLS, "shortlist=")            # (seen, merit), both their own guard
            self._sl_tables = None               # pool_select_hip's group tables, made by the first scoring push
            self._sl_pins = None                 # [2] int64 on the device: pins and dropped pins of the pushes not yet read
            self._ev_ids = (None, None)          # _every_class_ids' cache, with or without a rule: the ids behind a push's columns
        self._baseline = baseline                # the Baseline, or None: nothing below is there
        if baseline is not None:
            self._bl_cells = cells((f32, f32, i32, i32), (3,), blhip.MAX_CELLS, "baseline=")     # (mean, dev, count, marks)
        self._still = still                      # the StillGate, or None: nothing below is there
        if still is not None:
            self._totals.update(still_frames=0)
            self._sk_prev = None                 # [max_streams, L] fp32: every session's newest frame of its last pixel push; made by the first gated push
            self._sk_hw = None                   # the H x W the store was made for
            self._sk_state = {}                  # handle -> [has a predecessor in _sk_prev, run of skipped frames, still frames]
            self._sk_tables = php.TableUploader(self.dev, max_streams, cols=skhip.TABLE_COLS)
            self._sk_lists = skhip.ListUploader(self.dev)
            self._sk_work = None                 # still_hip.changed's workspace, grown on demand
            self._sk_last = {}                   # last_kept()'s answer
        self._history = history                  # the History, or None: nothing below is there
        if history is not None:
            self._hs_store = None                # [max_streams, F, E] fp32: frame f of a session at [slot, f mod F]; made by the first push
            self._hs_tables = php.TableUploader(self.dev, 2 * max_streams)   # a round's two tables in one upload; a search's one
            self._hs_X = None                    # a search's gathered windows [rows, T, E], grown on demand
            self._hs_work = None                 # history_hip.peaks' workspace, grown on demand
        self._timeline = timeline                # the Timeline, or None: nothing below is there
        if timeline is not None:
            self._tl_cells = _Buckets(self.dev, max_streams, timeline.buckets)      # (peak, at, above, marks), made by the first fold
            self._stores.append(self._tl_cells)  # open() and reset() queue the slot's marks for zeroing
            self._tl_first = None                # the push's first window numbers, behind its table in the one upload
            self._tl_tables = None               # timeline() and recall(): the read's table and the peak search's, made by the first call
            self._tl_work = None                 # history_hip.peaks' workspace of recall(), grown on demand
        if ingest is not None and not isinstance(ingest, FrameIngest):
            raise TypeError("StreamPool: ingest must be a FrameIngest, got %s" % type(ingest).__name__)
        if ingest is not None:
            ingest.serves(self.dev, who="StreamPool")
        self._ingest = ingest                    # push_u8's transform; None: built from gallery.head.args by the first push_u8

    @staticmethod
    def _check_rates(gallery, rates, rate, shortlist):
        """rates= of the constructor -> the tuple; every refusal of the option, before anything is allocated"""
        from .live_text_gallery import LiveTextGallery
        from .text_gallery import TextGallery
        if isinstance(rates, (str, bytes)) or not isinstance(rates, (tuple, list)):
            raise TypeError("StreamPool: rates must be a tuple of integers, got %s" % type(rates).__name__)
        if rate != 1:
            raise ValueError("StreamPool: rates= is given together with rate = %d -- leave rate at its default, the pool plans with the "
                             "largest of rates" % rate)
        if not 1 <= len(rates) <= tphip.MAX_RATES:
            raise ValueError("StreamPool: rates holds %d values -- give 1 to %d frame rates" % (len(rates), tphip.MAX_RATES))
        for r in rates:
            if isinstance(r, bool) or not isinstance(r, int) or r < 1:
                raise ValueError("StreamPool: rates must hold integers >= 1, got %r in %r" % (r, tuple(rates)))
        if any(b <= a for a, b in zip(rates, rates[1:])):
            raise ValueError("StreamPool: rates must be strictly ascending, got %r -- sort them and drop repeats" % (tuple(rates),))
        if isinstance(gallery, (TextGallery, LiveTextGallery)):
            raise ValueError("StreamPool: rates= on a %s is not supported -- a maximum over per-tempo softmax probabilities is another "
                             "quantity; use a SupportGallery or a LiveGallery" % type(gallery).__name__)
        if shortlist is not None:
            raise ValueError("StreamPool: rates= together with shortlist= is not supported -- tempo windows of a shortlisted pool are out "
                             "of scope; build the pool with one of the two")
        return tuple(rates)

    @staticmethod
    def _check_timeline(gallery, timeline, max_streams, shortlist, by_class, baseline):
        """every refusal of timeline= of the constructor, before anything is allocated"""
        if not isinstance(timeline, Timeline):
            raise TypeError("StreamPool: timeline must be a Timeline, got %s" % type(timeline).__name__)
        if not hasattr(gallery, "slot_generations"):
            raise ValueError("StreamPool: timeline= needs a gallery with a slot store (a LiveGallery or a LiveTextGallery), not a %s"
                             % type(gallery).__name__)
        if shortlist is not None:
            raise ValueError("StreamPool: timeline= together with shortlist= is not supported -- a shortlist's columns change with "
                             "every push, a timeline over them is out of scope; build the pool with one of the two")
        for of, made, how in (("smoothed", by_class, "smooth > 0 and smooth_by=\"class\""), ("deviation", baseline is not None, "baseline=")):
            if timeline.of == of and not made:
                raise ValueError("StreamPool: timeline.of = %r names a plane this pool does not make -- build it with %s, or leave of at "
                                 "None" % (of, how))
        if max_streams * timeline.buckets * gallery.capacity > tlhip.MAX_CELLS:
            raise ValueError(_Buckets.too_many(max_streams, timeline.buckets, gallery.capacity))

    @staticmethod
    def _check_history(gallery, history, cap, max_streams):
        """every refusal of history= of the constructor, before anything is allocated"""
        from .live_gallery import LiveGallery
        from .live_text_gallery import LiveTextGallery
        from .text_gallery import TextGallery
        if not isinstance(history, History):
            raise TypeError("StreamPool: history must be a History, got %s" % type(history).__name__)
        if isinstance(gallery, (TextGallery, LiveTextGallery)):
            raise ValueError("StreamPool: history= on a %s is not supported -- a softmax over the searched classes alone is another "
                             "quantity than the one over every class; use a LiveGallery" % type(gallery).__name__)
        if not isinstance(gallery, LiveGallery):
            raise ValueError("StreamPool: history= needs a gallery that scores class subsets and registers from features (a "
                             "LiveGallery), not a %s" % type(gallery).__name__)
        if history.frames < cap:
            raise ValueError("StreamPool: history.frames = %d is below the ring's cap = (T - 1) * rate + max_push = %d -- a history "
                             "shorter than the ring is the ring; give at least %d frames" % (history.frames, cap, cap))
        most = largest_frames(max_streams, gallery.E)
        if history.frames > most:
            raise ValueError("StreamPool: history.frames = %d x max_streams = %d rows of E = %d floats break the pool library's 32-bit "
                             "item limit -- the largest frames that fits is %d" % (history.frames, max_streams, gallery.E, most))

    # ------------------------------------------------------------------ sessions
    def open(self, classes=None):
        """a new session, its frames numbered from 0 -> its handle.  classes: registered class ids (any order, no repeats) -- the session
        is scored against these alone, its logits' columns in the order given; None: every class, in registration order."""
        if classes is not None and self.rates is not None:
            raise ValueError("StreamPool: open(classes=) on a pool with rates= is not supported -- per-session class lists with tempo "
                             "windows are out of scope; open the session without a list")
        if classes is not None and self._shortlist is not None:
            raise ValueError("StreamPool: open(classes=) on a pool with shortlist= is not supported -- per-session candidate lists are "
                             "out of scope; every session is shortlisted from every class")
        if classes is not None:
            classes = list(classes)
            if not hasattr(self.gallery, "classify_features_grouped"):
                raise ValueError("StreamPool: open(classes=) needs a gallery that scores groups (a LiveGallery), not a %s"
                                 % type(self.gallery).__name__)
            if self.alpha and not self._by_class:
                raise ValueError("StreamPool: open(classes=) on a pool with smooth > 0 is not supported -- smoothing with per-session "
                                 "class lists is out of scope; build the pool with smooth = 0")
            self._session_lists([self._next_handle], [classes])
        if not self._free:
            raise RuntimeError("StreamPool: all %d slots are in use -- close() a session or build the pool with a larger max_streams"
                               % self.max_streams)
        h = self._next_handle
        self._next_handle += 1
        self._sessions[h] = _Session(heapq.heappop(self._free), classes)
        self._forget(h, self._sessions[h])       # nothing of the slot's previous owner is read
        return h

    def _forget(self, h, s):
        """the session starts anew: no predecessor frame, and every store zeroes the slot's guards at the next push"""
        if self._still is not None:
            self._sk_state[h] = [False, 0, 0]    # the frame a previous owner of the slot left in the store is never read
        for store in self._stores:
            store.forgotten.add(s.slot)

    def _session_lists(self, handles, lists):
        """the sessions' class lists under the gallery's rules (registered, no repeats, not empty); an error names the session"""
        from .live_gallery import plan_columns
        for h, classes in zip(handles, lists):
            if classes is not None:
                plan_columns(self.gallery._book, classes, "StreamPool: session %d" % h)

    def _session(self, h):
        s = self._sessions.get(h) if isinstance(h, int) and not isinstance(h, bool) else None
        if s is None:
            raise ValueError("StreamPool: session %r is not open (closed, or never returned by open())" % (h,))
        return s

    def close(self, h):
        """the session's slot becomes free; its handle is never valid again"""
        heapq.heappush(self._free, self._session(h).slot)
        del self._sessions[h]
        if self._still is not None:
            del self._sk_state[h]

    def reset(self, h):
        """Frame counter 0; the session's ring contents and smoothing state are dropped."""
        s = self._session(h)
        s.clear()
        self._forget(h, s)

    @property
    def sessions(self):
        return sorted(self._sessions)

    def stats(self, h=None):
        """of a session: frames, tower_frames and windows since open() / reset(); of the pool: what all pushes added up to, and the open
        sessions -- with an event rule also "events" and "events_dropped", the records translated so far and those beyond max_events;
        with a shortlist also "pins" and "pins_dropped", the pinned (session, class) pairs the selections counted and those of them that
        more than K pins squeezed out (reading them synchronises); with evidence= also "evidence" and "evidence_missed", the windows
        captured and those that had left the ring or found no room, counted as "events" is, when the records are translated"""
        if h is not None and self._still is not None:
            s = self._session(h)
            return {"frames": s.t, "tower_frames": s.tower_frames, "windows": window_plan(0, s.t, self.T, self.stride, self.rate)[1],
                    "still_frames": self._sk_state[h][2]}
        if h is None:
            if self._shortlist is not None:
                self._read_pins()
            return dict(self._totals, open=len(self._sessions))
        s = self._session(h)
        return {"frames": s.t, "tower_frames": s.tower_frames, "windows": window_plan(0, s.t, self.T, self.stride, self.rate)[1]}

    # ------------------------------------------------------------------ pushes
    def _ready(self):
        g = self.gallery
        eng = g._fresh_engine()
        if not len(g):
            raise RuntimeError("%s: no classes registered" % g._name)
        return eng

    def _check(self, t, tail, what, layout, sessions, counts):
        """-> (the packed tensor as fp32, the sessions' records, counts as ints); every error of a push is raised here, before any launch"""
        recs, counts = self._check_members(sessions, counts)
        if isinstance(t, torch.Tensor) and t.dim() and sum(counts) != t.shape[0]:
            raise ValueError("StreamPool: counts sum to %d, %s holds %d frames" % (sum(counts), what, t.shape[0]))
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError("StreamPool: %s must be a HIP device tensor (no CPU path exists)" % what)
        if t.dim() != 1 + len(tail) or any(want is not None and got != want for got, want in zip(t.shape[1:], tail)):
            raise ValueError("StreamPool: %s must be %s, got %s" % (what, layout, tuple(t.shape)))
        self._check_state(sessions, recs)
        return t.to(dtype=torch.float32).contiguous(), recs, counts

    def _check_members(self, sessions, counts):
        """-> (the sessions' records, counts as ints): open sessions, each once, a count >= 1 for each"""
        sessions = list(sessions)
        counts = [int(c) for c in counts]
        recs = [self._session(h) for h in sessions]
        if len(set(sessions)) != len(sessions):
            raise ValueError("StreamPool: a session appears twice in one push: %r" % (sessions,))
        if not sessions or len(counts) != len(sessions) or min(counts) < 1:
            raise ValueError("StreamPool: a push needs sessions and one count >= 1 for each, got %d sessions, counts %r" % (
                len(sessions), counts))
        return recs, counts

    def _check_state(self, sessions, recs):
        self._session_lists(sessions, [s.classes for s in recs])         # a class removed since open(): raised here, before any launch
        if self.alpha and not self._by_class:
            C = len(self.gallery)
            fresh = self._state is None or self._state.shape[1] != C
            for h, s in zip(sessions, recs):
                if s.state_gen is not None and (fresh or s.state_gen != self._state_gen):
                    raise RuntimeError("StreamPool: the gallery has %d classes, the smoothing state of session %d was made with another "
                                       "count -- reset() the session after adding classes when smoothing is on" % (C, h))
                if s.state_gen is not None and s.state_layout != getattr(self.gallery, "layout_version", None):
                    raise RuntimeError("StreamPool: classes were removed from the gallery since the smoothing state of session %d was "
                                       "made, its columns mean other classes now -- reset() the session after removing classes when "
                                       "smoothing is on" % h)

    def push_packed(self, frames, sessions, counts):
        """frames [N, 3, H, W] fp32 (device): counts[i] next frames of sessions[i], one session after the other -> PackedOutput of the
        windows they complete.  The tower runs once per frame, in one call sequence over all of them."""
        eng = self._ready()
        frames, recs, counts = self._check(frames, (3, None, None), "frames", "[N, 3, H, W]", sessions, counts)
        if self._still is not None:
            return self._push_still(eng, frames, list(sessions), recs, counts)
        feats = torch.empty(frames.shape[0], self.E, device=self.dev, dtype=torch.float32)
        for f0 in range(0, frames.shape[0], eng.max_frames):
            f1 = min(frames.shape[0], f0 + eng.max_frames)
            eng.vit.forward(frames[f0:f1], feats[f0:f1])
        for s, n in zip(recs, counts):
            s.tower_frames += n
        self._totals["tower_frames"] += frames.shape[0]
        return self._run(eng, feats, list(sessions), recs, counts)

    def _push_still(self, eng, frames, handles, recs, counts):
        """push_packed of a pool with still= (clip_fsar_amd.still): the change count of every frame against its predecessor on the
        device, plan_still on the host -- counts.cpu() is the gate's ONE synchronisation per push: the tower call has to be sized on the
        host --, the kept frames packed and the store of newest frames updated in one launch, the tower over the kept frames alone,
        their rows expanded to a row per frame (a skipped frame before the push's first kept one reads the ring row of the session's
        newest frame, before _run writes the ring), and _run on the full [N, E] features, as push_features_packed would receive them."""
        gate = self._still
        N, (H, W) = frames.shape[0], frames.shape[2:]
        L = 3 * H * W
        if L > skhip.MAX_L:
            raise ValueError("StreamPool: still= keeps a frame of 3 x %d x %d = %d elements per session, 2^31 or more" % (H, W, L))
        if self._sk_prev is None:
            self._sk_prev = torch.empty(self.max_streams, L, device=self.dev, dtype=torch.float32)
            self._sk_hw = (H, W)
        if (H, W) != self._sk_hw:
            raise ValueError("StreamPool: frames of %d x %d pushed into a pool whose still= store was made for %d x %d -- a gated pool "
                             "takes one geometry" % (H, W, self._sk_hw[0], self._sk_hw[1]))
        states = [self._sk_state[h] for h in handles]
        rows, f0 = [], 0
        for s, st, n in zip(recs, states, counts):
            rows.append([s.slot, f0, n, (s.t - 1) % self.cap if st[0] else -1])
            f0 += n
        table = self._sk_tables.upload(rows)
        flat = frames.view(N, L)
        work = self._work("_sk_work", skhip.workspace_ints(N, L))
        changed = torch.empty(N, device=self.dev, dtype=torch.int32)
        skhip.changed(flat, self._sk_prev, changed, work, table, gate.tol)
        kept, src, runs = plan_still(changed.cpu().tolist(), rows, [st[1] for st in states], gate.limit(L), gate.max_run)
        NK = len(kept)
        packing = 0 < NK < N                     # every frame kept: the tower reads `frames`; none kept: there is no tower call
        packed = torch.empty(NK, L, device=self.dev, dtype=torch.float32) if packing else None
        skhip.pack(flat, packed, self._sk_prev, self._sk_lists.upload(kept) if packing else skhip.List(None, None, NK), table)
        for st in states:                        # the store holds this push's frames from here on, the ring their rows once _run is through
            st[0] = False
        tower_in = packed.view(NK, 3, H, W) if packing else frames
        kept_feats = torch.empty(NK, self.E, device=self.dev, dtype=torch.float32) if NK else None
        for k0 in range(0, NK, eng.max_frames):
            k1 = min(NK, k0 + eng.max_frames)
            eng.vit.forward(tower_in[k0:k1], kept_feats[k0:k1])
        if NK == N:                              # src is 0 .. N - 1: the kept rows are the push's
            feats = kept_feats
        else:
            feats = torch.empty(N, self.E, device=self.dev, dtype=torch.float32)
            skhip.expand(kept_feats, self._ring, feats, self._sk_lists.upload(src), table)
        out = self._run(eng, feats, handles, recs, counts)
        flags = [False] * N
        for i in kept:
            flags[i] = True
        self._sk_last = {}
        for h, s, st, row, run in zip(handles, recs, states, rows, runs):
            mine = tuple(flags[row[skhip.F0]:row[skhip.F0] + row[skhip.N]])
            self._sk_last[h] = mine
            s.tower_frames += sum(mine)
            st[0], st[1], st[2] = True, run, st[2] + len(mine) - sum(mine)
        self._totals["tower_frames"] += NK
        self._totals["still_frames"] += N - NK
        return out

    def last_kept(self):
        """of a pool with still=: {session: a bool per frame of its part of the most recent pixel push -- True: the frame went through
        the tower}"""
        if self._still is None:
            raise ValueError("StreamPool.last_kept: the pool was built without still=")
        return dict(self._sk_last)

    def push_features_packed(self, feats, sessions, counts):
        """feats [N, E] fp32 (device): the tower features of the frames -> as push_packed"""
        eng = self._ready()
        feats, recs, counts = self._check(feats, (self.E,), "feats", "[N, E=%d]" % self.E, sessions, counts)
        if self._still is not None:              # the sessions' newest frames are no longer the ones in the store
            for h in sessions:
                self._sk_state[h][:2] = [False, 0]
        return self._run(eng, feats, list(sessions), recs, counts)

    def _by_session(self, packed_call, per_session, what, dims):
        self._ready()
        if not isinstance(per_session, dict) or not per_session:
            raise ValueError("StreamPool: a push takes a non-empty dict {session: %s}" % what)
        for h, t in per_session.items():
            self._session(h)
            if not isinstance(t, torch.Tensor) or not t.is_cuda:
                raise RuntimeError("StreamPool: %s of session %r must be a HIP device tensor (no CPU path exists)" % (what, h))
            if t.dim() != dims or t.shape[0] < 1:
                raise ValueError("StreamPool: %s of session %r must have %d dimensions and n >= 1 rows, got %s" % (
                    what, h, dims, tuple(t.shape)))
        ts = list(per_session.values())
        return self._split(packed_call(ts[0] if len(ts) == 1 else torch.cat(ts, 0), list(per_session), [t.shape[0] for t in ts]))

    @staticmethod
    def _split(po):
        """PackedOutput or GroupedPackedOutput -> {session: StreamOutput}"""
        out = {}
        planes = [(k, getattr(po, k, None)) for k in ("smoothed", "deviation", "tempo")]     # each session carries its block of them
        rows = [(k, getattr(po, k, None)) for k in ("columns", "pinned")]                    # and its row of a shortlist's lists
        for i, h in enumerate(po.sessions):
            w0, w1 = po.offsets[i], po.offsets[i + 1]
            if isinstance(po, GroupedPackedOutput):
                block = lambda t: t[po.logit_offsets[i]:po.logit_offsets[i + 1]].view(w1 - w0, po.widths[i])
            else:
                block = lambda t: t[w0:w1]
            mine = {k: None if t is None else block(t) for k, t in planes}
            mine.update((k, None if t is None else t[i]) for k, t in rows)
            out[h] = _output(StreamOutput, po.first_window[i], block(po.logits), mine.pop("smoothed"), rates=getattr(po, "rates", None),
                             ids=getattr(po, "_ids", None), **mine)
        return out

    def push(self, frames):
        """{session: frames [n, 3, H, W]} -> {session: StreamOutput}; one push_packed over all of them"""
        return self._by_session(self.push_packed, frames, "frames", 4)

    def push_features(self, feats):
        """{session: feats [n, E]} -> {session: StreamOutput}; one push_features_packed over all of them"""
        return self._by_session(self.push_features_packed, feats, "feats", 2)

    # ------------------------------------------------------------------ pushes of decoded uint8 clips
    @property
    def ingest(self):
        """the FrameIngest of push_u8: the constructor's, or one built here from gallery.head.args (DATA.TEST_SCALE, TEST_CROP_SIZE, MEAN, STD)"""
        if self._ingest is None:
            self._ingest = FrameIngest.from_cfg(self.gallery.head.args, self.dev)
        return self._ingest

    def push_u8_packed(self, clips, sessions):
        """clips: a list of uint8 [n_i, H_i, W_i, 3], the next frames of sessions[i], each clip of its own geometry and on the device, in
        pinned or in pageable host memory -> PackedOutput.  FrameIngest.transform (one upload on its copy stream, one launch), then
        push_packed on its result: the same rounds, tables and stats.  Every error is raised before the upload starts."""
        eng = self._ready()
        ingest = self.ingest
        ingest.serves(self.dev, getattr(eng, "arch", {}).get("res"), "StreamPool")
        if not isinstance(clips, (list, tuple)) or not clips:
            raise ValueError("StreamPool: push_u8_packed takes a non-empty list of uint8 [n, H, W, 3] clips")
        sessions = list(sessions)
        if len(sessions) != len(clips):
            raise ValueError("StreamPool: %d clips for %d sessions" % (len(clips), len(sessions)))
        counts = [n for n, _, _ in ingest.check(clips)]
        recs, counts = self._check_members(sessions, counts)
        self._check_state(sessions, recs)
        return self.push_packed(ingest.transform(clips), sessions, counts)

    def push_u8(self, clips):
        """{session: uint8 [n, H, W, 3]} -> {session: StreamOutput}; one push_u8_packed over all of them"""
        self._ready()
        if not isinstance(clips, dict) or not clips:
            raise ValueError("StreamPool: a push takes a non-empty dict {session: uint8 [n, H, W, 3] frames}")
        return self._split(self.push_u8_packed(list(clips.values()), list(clips)))

    def _gathered(self, eng, plan, feats, recs=None):
        """The device side of a push up to scoring: per round one table and one ring write, then per chunk of its windows one gather.
        Yields (round, its table, its windows nW, chunk w0, w1, the chunk's windows X [w1 - w0, T, E]); a round without windows yields
        nothing.  Of a pool with rates=: X is [(w1 - w0) * R, T, E], the R tempos of every window, rows ordered (window, tempo), and a
        chunk holds as many windows as their R sequences each fit classify_features.  recs: the push's session records -- a pool
        with history= writes every round's rows into its store as well."""
        T = self.T
        done = [0] * len(plan.first_window)      # frames of each session the rounds so far have written
        R = 1 if self.rates is None else len(self.rates)
        per = max(1, eng.max_frames // (T * R))  # classify_features scores that many clips per chunk: gather no more at a time
        for rnd in plan.rounds:
            if len(plan.rounds) == 1:
                piece = feats
            else:                                # a later round's frames lie apart in the packed features: pack them for the ring write
                piece = torch.cat([feats[f0:f0 + n] for f0, n in rnd.src], 0)
            if self._history is None:
                table = self._tables.upload(rnd.rows)
                php.ring_put(piece, self._ring, table)
            else:                                # the store's table rides behind the ring's: one upload, two ring writes
                table, held = self._history_tables(rnd, recs, done)
                php.ring_put(piece, self._ring, table)
                php.ring_put(piece, self._hs_store, held)
            nW = sum(r[php.NW] for r in rnd.rows)
            if nW == 0:
                continue
            if self._X is None or self._X.shape[0] < min(nW, per) * R:
                self._X = torch.empty(min(nW, per) * R, T, self.E, device=self.dev, dtype=torch.float32)
            for w0 in range(0, nW, per):
                w1 = min(nW, w0 + per)
                X = self._X[:(w1 - w0) * R]
                if self.rates is None:
                    php.window_sequences(self._ring, X, table, nW, w0, w1, T, self.stride, self.rate)
                else:
                    tphip.window_sequences(self._ring, X, table, nW, w0, w1, T, self.stride, self.rates)
                yield rnd, table, nW, w0, w1, X

    def _run_grouped(self, eng, feats, handles, recs, counts):
        """_run of a push in which a session has a class list: every chunk of windows is scored by one grouped launch, each session's
        windows against its own list (None: every class) -> GroupedPackedOutput"""
        g, T = self.gallery, self.T
        plan = plan_push([(s.slot, s.t) for s in recs], counts, T, self.stride, self.rate, self.max_push)
        lists = [s.classes for s in recs]
        widths = [len(g) if c is None else len(c) for c in lists]
        offsets, logit_offsets = [0], [0]
        for nW, C in zip(plan.n_windows, widths):
            offsets.append(offsets[-1] + nW)
            logit_offsets.append(logit_offsets[-1] + nW * C)
        logits = torch.empty(logit_offsets[-1], device=self.dev, dtype=torch.float32)
        done = [0] * len(recs)                   # windows of each session scored so far: its block fills in window order
        for rnd, table, nW, w0, w1, X in self._gathered(eng, plan, feats, recs):
            # the chunk's windows session by session: row j of the round holds windows WIN_OFF .. WIN_OFF + NW - 1 of the round's list
            part = [(i, max(0, min(w1, r[php.WIN_OFF] + r[php.NW]) - max(w0, r[php.WIN_OFF]))) for i, r in zip(rnd.members, rnd.rows)]
            part = [(i, n) for i, n in part if n]
            res = g.classify_features_grouped(X, [n for _, n in part], [lists[i] for i, _ in part])
            if w1 - w0 == offsets[-1]:           # one chunk holds every window of the push: its flat logits are the push's
                logits = res.logits
                continue
            for j, (i, n) in enumerate(part):
                at = logit_offsets[i] + done[i] * widths[i]
                logits[at:at + n * widths[i]].copy_(res.logits[res.offsets[j]:res.offsets[j + 1]])
                done[i] += n
        cp = self._class_push(recs, plan.n_windows) if self._keyed and logits.numel() else None
        smoothed, deviation = self._judge(logits, cp, handles, recs, counts, plan.first_window)
        self._advance(recs, counts, offsets[-1])
        return _output(GroupedPackedOutput, handles, plan.first_window, offsets, logits, logit_offsets, widths, smoothed, deviation=deviation)

    def _judge(self, logits, cp, handles, recs, counts, first_window, columns=None, tempo=None):
        """what follows scoring in every push, over its session-major logits (dense [NW, C], [NW, K] of a shortlist push, or the grouped
        layout): per-class smoothing, the baseline, the contest and the detector, one after the other over the same table and keys ->
        (smoothed, deviation), each None without its option.  cp: _class_push's, None when the push completed no window or no option
        keeps cells; handles, recs, counts, first_window: of the table's rows -- the sessions of the push, of a shortlist push (which
        passes its `columns`) those with windows; their frame counters have not moved yet.  tempo: the push's tempo plane."""
        smoothed = self._smooth_classes(cp, logits) if self._by_class else None       # one launch, on the session-major logits: a
        judged = smoothed if self._by_class else logits                               # session's rounds stay in sequence
        deviation = None
        if self._baseline is not None:
            judged = deviation = self._normalize(cp, judged)
        if cp is not None and self._timeline is not None:                             # before the contest: its plane is the detector's alone
            self._fold(cp, {None: judged, "logits": logits, "smoothed": smoothed, "deviation": deviation}[self._timeline.of])
        if cp is not None and self._events is not None:
            seen = judged if self._contest_rule is None else self._contest(cp, judged)     # the detector alone sees the demoted plane
            self._detect(handles, recs, first_window, seen, cp, columns, [s.t + n for s, n in zip(recs, counts)], tempo)
        return smoothed, deviation

    def _advance(self, recs, counts, NW):
        """the push is enqueued: its sessions' frame counters and the pool's totals move"""
        for s, n in zip(recs, counts):
            s.t += n
        self._totals["frames"] += sum(counts)
        self._totals["windows"] += NW

    def _class_push(self, recs, n_windows):
        """what the launches over (session slot, store slot) cells share in one push -- per-class smoothing and the event detector: the
        host plan, the store slots' generations, the device keys and the uploaded descriptor table"""
        g = self.gallery
        book = g._book
        plan = cship.plan_rows([s.slot for s in recs], n_windows, [None if s.classes is None else [book.slot_of[c] for c in s.classes]
                                                                   for s in recs], len(book.order))
        gens = g.slot_generations()
        # the device keys: the gallery's own column list (every class's store slot, cached there until the classes change) for the sessions
        # without a list, the own lists behind it -- a push without lists uploads nothing
        every = g._columns(None) if plan.every else None
        key = tuple(plan.keys)
        if self._smooth_keys[0] != key or self._smooth_keys[1] is not every:
            own = torch.tensor(plan.keys, device=self.dev, dtype=torch.int32) if key else None
            self._smooth_keys = (key, every, own if every is None else every if own is None else torch.cat([every, own]))
        if self._timeline is not None:
            return plan, gens, self._smooth_keys[2], self._timeline_tables(plan.rows, recs)
        if self._smooth_tables is None:
            self._smooth_tables = cship.table_uploader(self.dev, self.max_streams)
        return plan, gens, self._smooth_keys[2], self._smooth_tables.upload(plan.rows)

    def _smooth_classes(self, cp, logits):
        """smooth_by="class": the push's logits, session-major (dense [NW, C] or the grouped layout), -> their smoothed values in the same
        layout; one launch over every session of the push.  cp: _class_push's, None when the push completed no window"""
        smoothed = torch.empty_like(logits)
        if cp is None:
            return smoothed
        _, gens, keys, table = cp
        state, marks = self._smooth_cells.at(gens.shape[0])
        cship.smooth_classes(logits.view(-1), state, marks, gens, keys, smoothed.view(-1), table, self.alpha)
        return smoothed

    # ------------------------------------------------------------------ baselines
    @property
    def _keyed(self):
        """whether a push runs a launch over (session slot, store slot) cells, i.e. needs _class_push's plan and upload"""
        return self._by_class or self._events is not None or self._baseline is not None or self._timeline is not None

    def _normalize(self, cp, scores):
        """the push's session-major scores (dense [NW, C] or the grouped layout) -> their deviations in the same layout; one
        cfbl_normalize over every session of the push.  cp: _class_push's, None when the push completed no window"""
        deviation = torch.empty_like(scores)
        if cp is None:
            return deviation
        b = self._baseline
        _, gens, keys, table = cp
        cells = self._bl_cells.at(gens.shape[0])
        blhip.normalize(scores.view(-1), *cells, gens, keys, deviation.view(-1), table, b.rate, b.warm_rate, b.warmup, b.gate, b.floor)
        return deviation

    def baseline(self, h):
        """[(class_id, mean, dev, n)]: the session's baselines -- its cells whose mark is the store slot's current generation -- in the
        order of the session's columns.  Synchronises."""
        if self._baseline is None:
            raise ValueError("StreamPool.baseline: this pool keeps no baselines (build it with baseline=Baseline(...))")
        s = self._session(h)
        ids, at, valid = self._live_cells(s, self._bl_cells)
        if not ids:
            return []
        cols = [t[s.slot].index_select(0, at).tolist() for t in self._bl_cells.planes[:3]]
        return [(c, m, d, n) for c, live, m, d, n in zip(ids, valid.tolist(), *cols) if live]

    def _live_cells(self, s, store):
        """of a store whose last plane holds the generation marks: (the session's class ids that have a cell, in the order of its
        columns; their store slots `at`, a device index; whether each cell's mark is the slot's current generation and, of a pool with a
        shortlist, the pair was scored at the session's last scoring push) -- ([], None, None) when there is none"""
        if store.planes is None or s.slot in store.forgotten:
            return [], None, None
        marks = store.planes[-1]
        book = self.gallery._book
        ids = [c for c in (book.order if s.classes is None else s.classes) if c in book.slot_of and book.slot_of[c] < marks.shape[1]]
        if not ids:
            return [], None, None
        at = torch.tensor([book.slot_of[c] for c in ids], device=self.dev)
        gens = self.gallery.slot_generations().index_select(0, at)
        return ids, at, (marks[s.slot].index_select(0, at) == gens) & self._listed(s, at)

    # ------------------------------------------------------------------ events
    def _every_class_ids(self):
        g = self.gallery
        key = (g.layout_version, len(g))          # columns change their meaning with a removal and are appended by an addition
        if self._ev_ids[0] != key:
            self._ev_ids = (key, tuple(g.class_ids))
        return self._ev_ids[1]

    def _work(self, name, need):
        """the int32 workspace kept under the attribute `name`, grown on demand to `need` elements"""
        work = getattr(self, name)
        if work is None or work.numel() < need:
            work = torch.empty(need, device=self.dev, dtype=torch.int32)
            setattr(self, name, work)
        return work

    def _contest(self, cp, judged):
        """the push's judged plane (dense [NW, C], [NW, K] of a shortlist push, or the grouped layout) -> the plane the detector sees, in
        the same layout: every window's leaders keep their bits, every other candidate is -inf; one cfct_contest over the table and keys
        of the push.  Nothing but the detector reads it."""
        c = self._contest_rule
        _, gens, keys, table = cp
        demoted = torch.empty_like(judged)
        work = self._work("_ct_work", cthip.workspace_words(judged.numel()))
        cthip.contest(judged.view(-1), keys, demoted.view(-1), None, None, work, table, gens.shape[0], c.top, c.margin)
        return demoted

    def leaders(self, out):
        """(columns [NW, top] int32, counts [NW] int32) of every window of a push's output, packed or per session: the window's leading
        classes as the detector saw them, ascending and padded with contest.NONE, and their number.  On the device, no synchronisation.
        Recomputed from the output's judged plane -- deviation with a baseline, else smoothed with per-class smoothing, else logits --
        through the pool's own cfct_contest.  A column is an index into gallery.class_ids; of a session with a class list of its own,
        and of a GroupedPackedOutput, it counts within that session's list; of a shortlist pool's output it is mapped through the
        session's `columns`, and a place without a class does not compete."""
        c = self._contest_rule
        if c is None:
            raise ValueError("StreamPool.leaders: this pool holds no contest (build it with events=EventRule(...), contest=Contest(...))")
        judged = getattr(out, "deviation", None)
        if judged is None:
            judged = out.logits if out.smoothed is None else out.smoothed
        keys, cap, lists = None, 1, None
        if isinstance(out, GroupedPackedOutput):
            n_windows, widths = [w1 - w0 for w0, w1 in zip(out.offsets, out.offsets[1:])], list(out.widths)
        elif hasattr(out, "columns"):              # of a pool with a shortlist: a place competes iff it holds a class
            n_windows, lists = self._shortlist_groups(out)
            widths, keys, cap = [judged.shape[1]] * len(n_windows), lists.contiguous().view(-1), pship.NONE
        else:
            n_windows, widths = [judged.shape[0]], [judged.shape[1]]
        NW = sum(n_windows)
        columns = torch.empty(NW, c.top, device=self.dev, dtype=torch.int32)
        counts = torch.empty(NW, device=self.dev, dtype=torch.int32)
        if not NW:
            return columns, counts
        if not judged.is_cuda:
            raise RuntimeError("StreamPool.leaders: the output's scores must be a HIP device tensor (no CPU path exists)")
        rows, n_out = [], 0
        for i, (nW, NC) in enumerate(zip(n_windows, widths)):
            rows.append([0, nW, n_out, NC, i * NC if keys is not None else 0, 0])
            n_out += nW * NC
        if self._ct_tables is None:
            self._ct_tables = cship.table_uploader(self.dev, self.max_streams)
        flat = judged.contiguous().view(-1)
        work = self._work("_ct_work", cthip.workspace_words(n_out))
        cthip.contest(flat, keys, torch.empty_like(flat), columns, counts, work, self._ct_tables.upload(rows), cap, c.top, c.margin)
        return columns if lists is None else self._listed_classes(columns, cthip.NONE, n_windows, lists), counts

    @staticmethod
    def _shortlist_groups(out):
        """a shortlist pool's output -> (the windows of each of its groups, their lists [groups, K]): a session's output is one group,
        a packed output holds one per session"""
        if out.columns.dim() == 1:
            return [out.logits.shape[0]], out.columns[None]
        return [w1 - w0 for w0, w1 in zip(out.offsets, out.offsets[1:])], out.columns

    def _listed_classes(self, places, none, n_windows, lists):
        """places [NW, k] int32 into the K places of each window's group (`none`: no place) -> the indices into gallery.class_ids that
        the group's list holds there; `none` stays"""
        group = torch.tensor([i for i, n in enumerate(n_windows) for _ in range(n)], device=self.dev, dtype=torch.int64)
        found = places != none
        place = torch.where(found, places, torch.zeros_like(places)).long()
        return torch.where(found, lists[group].gather(1, place), places)

    def _detect(self, handles, recs, first_window, scores, cp, columns=None, after=None, tempo=None):
        """one cfev_detect over the push's session-major scores (three launches, no synchronisation); the records stay on the device and
        are queued with the push's metadata.  columns: of a shortlist push, its sel_cols -- handles, recs and first_window then hold
        the sessions with windows alone, the table's rows.  after, tempo (a pool with evidence=): the frames each session will have
        after this push and the push's tempo plane -- the capture follows the detector on the same stream."""
        rule = self._events
        cplan, gens, keys, table = cp
        cells = self._ev_cells.at(gens.shape[0])
        M = rule.max_events
        n_where = 0 if self._evidence is None else 2 * M      # the capture's `where` rides behind the records: one copy brings both down
        buf = torch.empty(1 + (evhip.EVENT_COLS + evhip.VALUE_COLS) * M + n_where, device=self.dev, dtype=torch.int32)
        events, values = self._records(buf, M)
        work = self._work("_ev_work", evhip.workspace_ints(cplan.n_chunks))
        evhip.detect(scores.view(-1), *cells, gens, keys, events, values, buf[:1], work, table, rule.on, rule.off, rule.min_on, rule.min_off)
        if self._evidence is not None:
            self._capture(first_window, cplan.rows, after, events, buf[:1], self._where(buf, M), tempo)
        if len(self._ev_queue) >= EVENT_QUEUE:     # a full queue: the oldest batch is translated here and kept for take_events()
            self._ev_ready.extend(self._translate([self._ev_queue.popleft()]))
        every = None
        ids = []
        for s in recs:
            if s.classes is None:
                every = self._every_class_ids() if every is None else every
            ids.append(every if s.classes is None else s.classes)       # a session's list is replaced (enroll's join), never changed
        self._ev_queue.append(EventBatch(buf, handles, first_window, ids, columns))

    @staticmethod
    def _records(buf, M):
        """the events [M, 5] int32 and values [M, 2] fp32 inside an EventBatch's buffer (buf[0] is n_events)"""
        split = 1 + evhip.EVENT_COLS * M
        return buf[1:split].view(M, evhip.EVENT_COLS), buf[split:split + evhip.VALUE_COLS * M].view(torch.float32).view(M, evhip.VALUE_COLS)

    @staticmethod
    def _where(buf, M):
        """of a pool with evidence=: the capture's where [M, 2] int32 behind the records of an EventBatch's buffer"""
        return buf[1 + (evhip.EVENT_COLS + evhip.VALUE_COLS) * M:].view(M, 2)

    def _capture(self, first_window, rows, after, events, n_events, where, tempo):
        """one cfed_capture behind the detector (two launches, no synchronisation): the windows of the push's records of the Evidence's
        kinds go into the store.  rows: the detector's table rows; first_window, after: per row the session's first window of the push
        and its frames once the push is done, which say where the row's windows lie in the ring and which of them a later round of the
        same push has overwritten."""
        ev = self._evidence
        if self._ed_store is None:
            self._ed_store = torch.empty(ev.capacity, self.T, self.E, device=self.dev, dtype=torch.float32)
            self._ed_head = torch.zeros(1, device=self.dev, dtype=torch.int32)
            self._ed_work = torch.empty(edhip.workspace_ints(ev.capacity), device=self.dev, dtype=torch.int32)
            self._ed_tables = edhip.table_uploader(self.dev, self.max_streams)
        table = [[r[evhip.SLOT], (first * self.stride) % self.cap, r[evhip.NW], keep0(first, r[evhip.NW], self.stride, t, self.cap),
                  r[evhip.OUT0], r[evhip.NC]] for r, first, t in zip(rows, first_window, after)]
        more = {} if self.rates is None else dict(rates=self.rates)
        edhip.capture(self._ring, events, n_events, None if self.rates is None else tempo.view(-1), self._ed_store, self._ed_head, where,
                      self._ed_work, self._ed_tables.upload(table), ev.mask, self.stride, self.rate, **more)

    def _translate(self, batches):
        """EventBatches -> their Events, batch by batch; one synchronising copy"""
        if not batches:
            return []
        M = self._events.max_events
        if self._shortlist is None:
            host = (batches[0].buf[None] if len(batches) == 1 else torch.stack([b.buf for b in batches])).cpu()
            lists = [None] * len(batches)
        else:                                      # the pushes' columns ride behind their records, and the pin counters (two int64 as
            pieces = [t.reshape(-1) for b in batches for t in (b.buf, b.columns)]       # four int32) behind them: still one copy
            counted, self._sl_pins = self._sl_pins, None
            if counted is not None:
                pieces.append(counted.view(torch.int32))
            parts = torch.cat(pieces).cpu().split([t.numel() for t in pieces])
            if counted is not None:
                self._count_pins(*parts[-1].clone().view(torch.int64).tolist())
            host, lists = parts[0:2 * len(batches):2], [c.view(len(b.sessions), -1).tolist() for b, c in zip(batches, parts[1::2])]
        out, dropped = [], 0
        for b, h, columns in zip(batches, host, lists):
            n = int(h[0])
            kept = min(n, M)
            events, values = self._records(h, M)
            ids = b.class_ids
            if columns is not None:                # a record's column is a place of the push's list: the class behind it then
                ids = [[every[c] if c != pship.NONE else None for c in row] for every, row in zip(ids, columns)]
            found = translate(events[:kept], values[:kept], kept, b.sessions, b.first_window, ids, self._events)
            out.extend(found if self._evidence is None else self._with_evidence(found, events[:kept].tolist(), self._where(h, M)[:kept].tolist()))
            self._totals["events"] += kept
            dropped += n - kept
        if dropped:
            self._totals["events_dropped"] += dropped
            warnings.warn("StreamPool: %d event records beyond max_events = %d per push were dropped (the detector's state advanced all "
                          "the same) -- build the rule with a larger max_events" % (dropped, M), RuntimeWarning, stacklevel=3)
        return out

    def _need_rule(self, what):
        if self._events is None:
            raise ValueError("StreamPool.%s: this pool has no event rule (build it with events=EventRule(...))" % what)

    def take_events(self):
        """the Events of every push since the last call, push by push; within a push in session order as pushed, then window, then
        column.  Synchronises once; clears the queue.  (Of a pool with a shortlist the pin counters come down in the same copy.)"""
        self._need_rule("take_events")
        batches = list(self._ev_queue)
        self._ev_queue.clear()
        out, self._ev_ready = self._ev_ready, []
        out.extend(self._translate(batches))
        return out

    def active(self, h):
        """[(class_id, length, peak)]: the session's pairs whose event is running -- active cells whose mark is the store slot's current
        generation -- in the order of the session's columns.  Synchronises."""
        self._need_rule("active")
        s = self._session(h)
        ids, at, valid = self._live_cells(s, self._ev_cells)
        if not ids:
            return []
        streak, length, peak, _ = self._ev_cells.planes
        on = (valid & (streak[s.slot].index_select(0, at) < 0)).tolist()
        lens, peaks = length[s.slot].index_select(0, at).tolist(), peak[s.slot].index_select(0, at).tolist()
        return [(c, n, p) for c, live, n, p in zip(ids, on, lens, peaks) if live]

    # ------------------------------------------------------------------ event evidence
    def _with_evidence(self, found, records, where):
        """the Events of one batch (translate's order) -> this pool's EvidenceEvents.  records, where: the batch's kept records and the
        capture's answers, in the device's record order -- the order in which the captures took their slots, so the order of the serials"""
        serial = {}
        for i, (slot, _) in enumerate(where):
            if slot >= 0:
                if slot != self._ed_captured % self._evidence.capacity:
                    raise RuntimeError("StreamPool: capture %d took slot %d of the evidence store, the host counted it into slot %d -- "
                                       "the device's head and the host's count have parted" % (
                                           self._ed_captured, slot, self._ed_captured % self._evidence.capacity))
                serial[i] = self._ed_captured
                self._ed_captured += 1
            elif slot in (edhip.LEFT_RING, edhip.NO_ROOM):
                self._totals["evidence_missed"] += 1
        self._totals["evidence"] += len(serial)
        # translate sorts the records by (row, window, column) with a stable sort: the same sort over their indices pairs them up
        order = sorted(range(len(records)), key=lambda i: (records[i][0], records[i][2], records[i][1]))
        tempo = self.rates is not None
        return [self._event_type(*e, serial.get(i), None if i in serial else MISSED[where[i][0]], where[i][1] if tempo and i in serial else None)
                for e, i in zip(found, order)]

    def _held_event(self, e, what):
        """every refusal of an event method; drains the queued batches (one synchronisation) so that the host's count of captures is the
        device's -> the event's store slot"""
        if self._evidence is None:
            raise ValueError("StreamPool.%s: this pool keeps no evidence (build it with events=EventRule(...), evidence=Evidence(...))" % what)
        if type(e) is not self._event_type:
            raise TypeError("StreamPool.%s: takes an EvidenceEvent that this pool's take_events() returned, got %s%s" % (
                what, type(e).__name__, " of another pool" if isinstance(e, EvidenceEvent) else ""))
        if e.evidence is None:
            why = {"ring": "its window had left the ring when the push that detected it ended (a push of several rounds)",
                   "capacity": "the push that detected it captured more than capacity = %d windows" % self._evidence.capacity,
                   "kind": "evidence is kept for %s events, this one is an %s" % (" and ".join(self._evidence.kinds), e.kind)}[e.missed]
            raise ValueError("StreamPool.%s: the event has no evidence (missed = %r): %s" % (what, e.missed, why))
        batches = list(self._ev_queue)
        self._ev_queue.clear()
        self._ev_ready.extend(self._translate(batches))         # take_events() returns them later
        cap = self._evidence.capacity
        if isinstance(e.evidence, bool) or not isinstance(e.evidence, int) or not 0 <= e.evidence < self._ed_captured:
            raise ValueError("StreamPool.%s: evidence %r is not a serial this pool has handed out (%d so far)" % (
                what, e.evidence, self._ed_captured))
        if self._ed_captured - e.evidence > cap:
            raise ValueError("StreamPool.%s: evidence %d is no longer held -- %d windows were captured since, the store keeps the newest "
                             "capacity = %d; build the pool with a larger Evidence(capacity=)" % (
                                 what, e.evidence, self._ed_captured - 1 - e.evidence, cap))
        return e.evidence % cap

    def held(self, e):
        """whether the event's window is in the store: it was captured, and fewer than `capacity` windows were captured since.
        Synchronises once when pushes are queued (their events stay for take_events())."""
        try:
            self._held_event(e, "held")
        except ValueError:
            if self._evidence is None:
                raise
            return False
        return True

    def evidence_features(self, e):
        """[T, E] fp32, a copy: the tower rows of the event's window as they were in the ring when the event was detected"""
        slot = self._held_event(e, "evidence_features")
        return self._ed_store[slot].clone()

    def explain_event(self, e, classes=None, k=None):
        """explain() of an event's evidence: the OTAM soft alignment of its window against `classes` (default: the event's own class) or
        against its top-k classes -> clip_fsar_amd.align.Alignment of one clip, through Aligner.align_features.  Changes nothing."""
        slot = self._held_event(e, "explain_event")
        al = self._the_aligner()
        if classes is None and k is None:
            classes = [e.class_id]
        return al.align_features(self._ed_store[slot].clone().unsqueeze(0), classes, k)

    def enroll_event(self, e, class_id, text=None):
        """enroll() of an event's evidence: its window becomes a shot of class_id -- of a registered class a further one, of an unknown id
        the first of a new class (its text from TEST.CLASS_NAME or from `text`, {class id: name or [E] row}) -> the class's shot count.
        Through the gallery's add_shots_features / add_classes_features; nothing of any session changes."""
        slot = self._held_event(e, "enroll_event")
        g = self._enrolling_gallery()
        cid = g._shot_ids([class_id])[0]
        feats = self._ed_store[slot].clone().unsqueeze(0)
        if cid in g._book.slot_of:
            return list(g.add_shots_features(feats, [cid]))[0]
        g.add_classes_features(feats, [cid], text)
        return 1

    def _run(self, eng, feats, handles, recs, counts):
        if self._shortlist is not None:
            return self._run_shortlist(eng, feats, handles, recs, counts)
        if any(s.classes is not None for s in recs):
            return self._run_grouped(eng, feats, handles, recs, counts)
        g, T, C = self.gallery, self.T, len(self.gallery)
        by_column = bool(self.alpha) and not self._by_class
        plan = plan_push([(s.slot, s.t) for s in recs], counts, T, self.stride, self.rate, self.max_push, smoothing=by_column)
        NW = sum(plan.n_windows)
        logits = torch.empty(NW, C, device=self.dev, dtype=torch.float32)
        smoothed = torch.empty_like(logits) if by_column else None
        tempo = torch.empty(NW, C, device=self.dev, dtype=torch.int32) if self.rates is not None else None
        if by_column and NW and (self._state is None or self._state.shape[1] != C):
            self._state = torch.empty(self.max_streams, C, device=self.dev, dtype=torch.float32)
            self._state_gen += 1
        g0 = 0
        for rnd, table, nW, w0, w1, X in self._gathered(eng, plan, feats, recs):
            out = logits[g0:g0 + nW]
            if tempo is None:
                out[w0:w1].copy_(g.classify_features(X))
            else:                                # the R scores of every (window, class) cell -> their maximum and the tempo that gave it
                tphip.reduce(g.classify_features(X), out[w0:w1], tempo[g0 + w0:g0 + w1], len(self.rates))
            if w1 == nW:                         # the round's last chunk
                if by_column:
                    php.smooth_logits(out, self._state, smoothed[g0:g0 + nW], table, self.alpha)
                g0 += nW
        if plan.order is not None and NW:        # several rounds: round-major -> session-major
            index = torch.tensor(plan.order, device=self.dev)
            logits = logits.index_select(0, index)
            smoothed = smoothed.index_select(0, index) if by_column else None
            tempo = tempo.index_select(0, index) if tempo is not None else None
        cp = self._class_push(recs, plan.n_windows) if self._keyed and NW else None
        by_class, deviation = self._judge(logits, cp, handles, recs, counts, plan.first_window, tempo=tempo)
        self._advance(recs, counts, NW)
        offsets = [0]
        for s, nW in zip(recs, plan.n_windows):
            if by_column and nW:
                s.state_gen = self._state_gen
                s.state_layout = getattr(g, "layout_version", None)
            offsets.append(offsets[-1] + nW)
        return _output(PackedOutput, handles, plan.first_window, offsets, logits, smoothed if by_column else by_class, deviation=deviation,
                       tempo=tempo, rates=self.rates)

    # ------------------------------------------------------------------ the pool with a shortlist
    def _listed(self, s, at):
        """of a pool with a shortlist: which of the session's cells at the store slots `at` (a device index) were scored at its last
        scoring push -- active() and baseline() list those alone; without a shortlist: all of them"""
        if self._shortlist is None:
            return torch.ones(at.shape[0], device=self.dev, dtype=torch.bool)
        if self._sl_cells.planes is None or s.slot in self._sl_cells.forgotten or not s.tick:
            return torch.zeros(at.shape[0], device=self.dev, dtype=torch.bool)
        seen = self._sl_cells.planes[0]
        inside = at < seen.shape[1]
        return inside & (seen[s.slot].index_select(0, at.clamp(max=seen.shape[1] - 1)) == s.tick)

    def _read_pins(self):
        """the device's pin counts of the pushes since the last reading -> the totals.  Synchronises."""
        if self._sl_pins is not None:
            counted, self._sl_pins = self._sl_pins, None
            self._count_pins(*counted.tolist())

    def _count_pins(self, pins, dropped):
        self._totals["pins"] += pins
        self._totals["pins_dropped"] += dropped

    def _run_shortlist(self, eng, feats, handles, recs, counts):
        """_run of a pool with a shortlist: every window of the push is gathered into one session-major buffer, each session's windows
        are one group of the Shortlist's stages with cfps_select_pinned in the place of cfsh_select, and smoothing, baselines and the
        detector run over the selected slot lists [G, K] as their keys -> ShortlistPackedOutput"""
        g, T, sl = self.gallery, self.T, self._shortlist
        plan = plan_push([(s.slot, s.t) for s in recs], counts, T, self.stride, self.rate, self.max_push)
        NW = sum(plan.n_windows)
        live = [i for i, nW in enumerate(plan.n_windows) if nW]               # the sessions with a group, in the order pushed
        # ---- what the host decides and sends up before the first launch
        K = min(sl.keep, len(g))
        if NW:
            prep = sl._pool_prepare()
            gens = g.slot_generations()
            order = None if plan.order is None else torch.tensor(plan.order, device=self.dev)
            n_live = [plan.n_windows[i] for i in live]
            sel_rows, _ = pship.table_rows(n_live, [recs[i].slot for i in live], [recs[i].tick + 1 for i in live])
            chunks = -(-K // cship.CHUNK)
            key_rows = [[recs[i].slot, nW, q * K, K, j * K, j * chunks] for j, (i, nW, q) in enumerate(zip(live, n_live, (
                r[pship.Q0] for r in sel_rows)))]                             # plan_rows' shape: NC = K, KEY0 = j * K
            cplan = cship.SmoothPlan(key_rows, [], False, NW * K, len(live) * chunks)
        every = self._every_class_ids()          # cached until the classes change: no O(classes) work per tick
        # ---- the device: ring writes and gathers, round by round
        W = torch.empty(NW, T, self.E, device=self.dev, dtype=torch.float32)
        g0 = 0
        for rnd, table, nW, w0, w1, X in self._gathered(eng, plan, feats, recs):
            W[g0 + w0:g0 + w1].copy_(X)
            if w1 == nW:
                g0 += nW
        offsets = [0]
        for nW in plan.n_windows:
            offsets.append(offsets[-1] + nW)
        S_push = len(recs)
        columns = torch.full((S_push, K), pship.NONE, device=self.dev, dtype=torch.int32)
        pinned = torch.zeros(S_push, K, device=self.dev, dtype=torch.int32)
        logits = torch.empty(NW, K, device=self.dev, dtype=torch.float32)
        smoothed = torch.empty_like(logits) if self._by_class else None
        deviation = torch.empty_like(logits) if self._baseline is not None else None
        if NW:
            if order is not None:                  # several rounds: round-major -> session-major, a group must be consecutive
                W = W.index_select(0, order)
            cap = gens.shape[0]
            seen, merit = self._sl_cells.at(cap)
            smooth_marks = self._smooth_cells.at(cap)[1] if self._by_class else None
            base_marks = self._bl_cells.at(cap)[3] if self._baseline is not None else None
            ev_streak, _, _, ev_marks = self._ev_cells.at(cap) if self._events is not None else [None] * 4
            G = len(live)
            if self._sl_tables is None:
                self._sl_tables = pship.table_uploader(self.dev, self.max_streams)
            sel_pin = torch.empty(G, K, device=self.dev, dtype=torch.int32)
            n_pins = torch.empty(G, device=self.dev, dtype=torch.int32)

            def select(S, cols, K):
                sel_cols = torch.empty(G, K, device=self.dev, dtype=torch.int32)
                sel_slots = torch.empty(G, K, device=self.dev, dtype=torch.int32)
                work = torch.empty(pship.workspace_floats(G, S.shape[1]), device=self.dev, dtype=torch.float32)
                pship.select_pinned(S, cols, gens, ev_streak, ev_marks, seen, merit, smooth_marks, base_marks,
                                    self._sl_tables.upload(sel_rows), sl.keep, self._hold, sel_cols, sel_slots, sel_pin, n_pins, work)
                return sel_cols, sel_slots

            sel_cols, sel_slots, flat, _ = sl._pool_score(prep, W, n_live, select)
            logits = flat.view(NW, K)
            for s in (recs[i] for i in live):
                s.tick += 1
            if self._smooth_tables is None:
                self._smooth_tables = cship.table_uploader(self.dev, self.max_streams)
            cp = (cplan, gens, sel_slots.view(-1), self._smooth_tables.upload(key_rows))
            # (the padded places of a list carry no store slot: they are no candidates of the contest)
            rows = lambda per_session: [per_session[i] for i in live]         # the table's rows: the sessions with windows
            smoothed, deviation = self._judge(logits, cp, rows(handles), rows(recs), rows(counts), rows(plan.first_window), columns=sel_cols)
            if G == S_push:
                columns, pinned = sel_cols, sel_pin
            else:
                for j, i in enumerate(live):     # no index goes up inside a push: the rows are copied one by one
                    columns[i].copy_(sel_cols[j])
                    pinned[i].copy_(sel_pin[j])
            counted = torch.stack([n_pins.sum(), (n_pins - K).clamp_(min=0).sum()])
            self._sl_pins = counted if self._sl_pins is None else self._sl_pins + counted
        self._advance(recs, counts, NW)
        return _output(PackedOutput, handles, plan.first_window, offsets, logits, smoothed, deviation=deviation, columns=columns,
                       pinned=pinned, ids=every)

    def _topk_shortlist(self, out, k, smoothed):
        """topk of a shortlist pool's output: the top-k places of every window's row (a place without a class is never taken), mapped
        to class indices through the session's columns"""
        src = out.smoothed if smoothed else out.logits
        if src is None:
            raise ValueError("StreamPool.topk: this output has no smoothed scores (smooth = 0)")
        nW, K = src.shape
        if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= min(grhip.TOPK_MAX, K):
            raise ValueError("StreamPool.topk: k must be in [1, min(16, K = %d = min(keep, number of classes))], got %r" % (K, k))
        if not nW:
            return (torch.empty(0, k, device=self.dev, dtype=torch.float32), torch.empty(0, k, device=self.dev, dtype=torch.int32))
        n_windows, lists = self._shortlist_groups(out)
        rows, _ = grhip.table_rows(n_windows, [K] * len(n_windows), self.T)
        values, index = self.gallery.topk_of_groups(src.contiguous().view(-1), rows, k)
        return values, self._listed_classes(index, pship.NONE, n_windows, lists)

    # ------------------------------------------------------------------ enrolment
    def _enrolling_gallery(self):
        g = self.gallery
        if not hasattr(g, "add_shots_features"):
            raise ValueError("StreamPool: enrolment needs a gallery that registers from features (a LiveGallery), not a %s"
                             % type(g).__name__)
        return g

    def enrolable(self, h):
        """range of the session's window numbers that enroll() accepts: complete, and their first frame still in the ring"""
        self._enrolling_gallery()
        return enrolable_windows(self._session(h).t, self.T, self.stride, self.rate, self.cap)

    def _tempo(self, tempo, what):
        """tempo= of enroll / enroll_windows / explain -> (the rate the window is read at, how far its first frame lies behind the first
        frame of the window as enrolable(h) numbers it)"""
        if self.rates is None:
            if tempo is not None:
                raise ValueError("StreamPool.%s: tempo = %r on a pool without rates= -- build the pool with rates=(...) or leave tempo "
                                 "at None" % (what, tempo))
            return self.rate, 0
        R = len(self.rates)
        if tempo is None:
            tempo = R - 1
        if isinstance(tempo, bool) or not isinstance(tempo, int) or not 0 <= tempo < R:
            raise ValueError("StreamPool.%s: tempo must be an index into rates = %r, 0 .. %d, or None (the last one), got %r"
                             % (what, self.rates, R - 1, tempo))
        return self.rates[tempo], (self.T - 1) * (self.rate - self.rates[tempo])

    def _ring_sequences(self, trows, slots, positions, classes, rate=None, ring=None):
        """one launch: the support sequences X0 [n, T+1, E] of the ring windows (slot, position), each closed by trows[classes[i]];
        rate: the frames' distance in the ring (None: the pool's); ring: what is read, [max_streams, its cap, E], the positions
        counting modulo that cap (None: the pool's ring; the history store of a pool with history=)"""
        n = len(slots)
        if self._enroll_tables is None or self._enroll_tables.max_rows < n:
            self._enroll_tables = enhip.table_uploader(self.dev, max(1024, n))
        X0 = torch.empty(n, self.T + 1, self.E, device=self.dev, dtype=torch.float32)
        enhip.ring_sequences(self._ring if ring is None else ring, trows, self._enroll_tables.upload(enhip.table_rows(slots, positions, classes)), X0,
                             self.rate if rate is None else rate)
        return X0

    def enroll_windows(self, items, text=None, tempo=None):
        """items: [(session, window number or None: the session's newest complete window, class id), ...] -> {class id: its shot count}.
        Every window becomes a shot of its class: of a registered class a further one (LiveGallery.add_shots' rules), of an unknown id
        the first of a new class (add_classes' rules; its text from TEST.CLASS_NAME or from `text`).  Several windows of one class are its
        shots in the order given.  tempo (a pool with rates=): the index into rates at which every window of the call is read; None:
        the last one, the window as enrolable(h) numbers it.  The windows' tower rows are read out of the ring -- one launch for the new classes, one for the further
        shots -- and the tower does not run.  Every error is raised before any launch and leaves the gallery as it was."""
        g = self._enrolling_gallery()
        rate, shift = self._tempo(tempo, "enroll_windows")
        eng = g._fresh_engine()
        items = list(items) if isinstance(items, (list, tuple)) else None
        if not items or any(not isinstance(it, (list, tuple)) or len(it) != 3 for it in items):
            raise ValueError("StreamPool: enroll_windows takes a non-empty list of (session, window or None, class id)")
        if text is not None and not isinstance(text, dict):
            raise TypeError("StreamPool: `text` must map class id -> class name or [E] text row")
        for h, _, _ in items:
            self._session(h)
        handles = list(dict.fromkeys(h for h, _, _ in items))
        at = {h: i for i, h in enumerate(handles)}
        plan = plan_enroll([(self._sessions[h].slot, self._sessions[h].t) for h in handles], [(at[h], w) for h, w, _ in items], self.T,
                           self.stride, self.rate, self.cap, names=["StreamPool: session %d" % h for h in handles])
        ids = g._shot_ids([c for _, _, c in items])
        book = g._book
        known = [i for i, c in enumerate(ids) if c in book.slot_of]
        new = [i for i, c in enumerate(ids) if c not in book.slot_of]
        shot_plan = add = None
        if known:
            shot_plan = g._plan_shots([ids[i] for i in known], book)
            book = shot_plan.book
        if new:
            new_ids = list(dict.fromkeys(ids[i] for i in new))
            add = g._plan_classes(eng, [ids[i] for i in new], new_ids, text, book)
        # ---- the device work: nothing below raises on the call's arguments
        def sequences(members, classes):
            """trows -> (X0, offs): the windows of the items `members` grouped by class in the order of `classes`, the caller's order
            inside a class, each closed by its class's row of trows; one launch"""
            local = {c: j for j, c in enumerate(classes)}
            order = sorted(members, key=lambda i: (local[ids[i]], i))
            offs = [0]
            for c in classes:
                offs.append(offs[-1] + sum(1 for i in members if ids[i] == c))
            at_tempo = () if self.rates is None else (rate,)                  # a pool without rates= calls it as it always did
            return lambda trows: (self._ring_sequences(trows, [plan.slots[i] for i in order],
                                                       [(plan.positions[i] + shift) % self.cap for i in order],
                                                       [local[ids[i]] for i in order], *at_tempo), offs)

        result, serial_of = {}, {}

        def made(members, classes):
            """a gallery with a shot ledger: the serials its call just made, class-grouped as the sequences were, by item"""
            if getattr(g, "_ledger", None) is not None:
                local = {c: j for j, c in enumerate(classes)}
                serial_of.update(zip(sorted(members, key=lambda i: (local[ids[i]], i)), g._last_shots))

        if known:
            result.update(zip(shot_plan.classes, g._shots_sequences(eng, shot_plan, sequences(known, shot_plan.classes))))
            made(known, shot_plan.classes)
        if new:
            trows, counts, add_plan = add
            g._register_sequences(eng, trows, counts, add_plan, sequences(new, new_ids))
            result.update(zip(new_ids, counts))
            made(new, new_ids)
        if serial_of:                                         # last_shots: of the whole call, in the order of its items
            g._last_shots = [serial_of[i] for i in range(len(items))]
            result.update((c, g.shots(c)) for c in result)    # per_class: the counts the call leaves behind
        return {c: result[c] for c in dict.fromkeys(ids)}

    def enroll(self, h, class_id, window=None, text=None, join=False, tempo=None):
        """enroll_windows([(h, window, class_id)], text, tempo) -> the class's shot count.  join=True: a session opened with classes=[...] gets
        the class appended to its list when it is not there (a session without a list sees every class anyway)."""
        if join and self._shortlist is not None:
            raise ValueError("StreamPool: enroll(join=True) on a pool with shortlist= is not supported -- per-session candidate lists are "
                             "out of scope; every session is shortlisted from every class, an enrolled one included")
        shots = self.enroll_windows([(h, window, class_id)], text, tempo)
        cid = next(iter(shots))
        s = self._sessions[h]
        if join and s.classes is not None and cid not in s.classes:
            s.classes = s.classes + [cid]
        return shots[cid]

    # ------------------------------------------------------------------ explanation
    def _the_aligner(self):
        """the pool's Aligner over its gallery, made by the first explanation"""
        from .align import Aligner
        al = getattr(self, "_aligner", None)
        if al is None or al.gallery is not self.gallery:
            al = self._aligner = Aligner(self.gallery)
        return al

    def explain(self, h, classes=None, k=None, window=None, tempo=None):
        """The OTAM soft alignment of one window of the session (window: a number of enrolable(h); None: the newest complete one) against
        `classes` (registered ids) or against its own top-k classes -> clip_fsar_amd.align.Alignment of one clip: per class the T x T plan,
        the cosine distances and the logit.  The window's T tower rows are read out of the ring, as enroll() reads them, and go through
        Aligner.align_features; nothing of the session changes -- ring, counters, smoothing, baselines, detector and shortlist planes stay
        as they are.  Of an event e: explain(e.session, [e.class_id], window=e.window), as long as the window is in the ring (explain_event(e) of a pool
        with evidence= has no such limit).  tempo (a
        pool with rates=): the index into rates at which the window is read; None: the last one."""
        s = self._session(h)
        rate, shift = self._tempo(tempo, "explain")
        al = self._the_aligner()
        ap = al._plan(1, classes, k)                                          # every error before the device is touched
        plan = plan_enroll([(s.slot, s.t)], [(0, window)], self.T, self.stride, self.rate, self.cap, names=["StreamPool: session %d" % h])
        rows = torch.tensor([(plan.positions[0] + shift + j * rate) % self.cap for j in range(self.T)], device=self.dev)
        return al._run(ap, self.gallery._check_feats(self._ring[s.slot].index_select(0, rows).unsqueeze(0)), False)

    # ------------------------------------------------------------------ top-k
    def _topk_grouped(self, out, k, smoothed):
        if smoothed and out.smoothed is None:
            raise ValueError("StreamPool.topk: this output has no smoothed scores (smooth = 0)")
        n_windows = [w1 - w0 for w0, w1 in zip(out.offsets, out.offsets[1:])]
        widths = [C for nW, C in zip(n_windows, out.widths) if nW]
        if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= min([grhip.TOPK_MAX] + widths):
            raise ValueError("StreamPool.topk: k must be in [1, min(16, the shortest class list of a session with windows)], got %r" % (k,))
        if not out.offsets[-1]:
            return (torch.empty(0, k, device=self.dev, dtype=torch.float32), torch.empty(0, k, device=self.dev, dtype=torch.int32))
        rows, _ = grhip.table_rows(n_windows, out.widths, self.T)
        return self.gallery.topk_of_groups(out.smoothed if smoothed else out.logits, rows, k)

    def topk(self, out, k=5, smoothed=False):
        """(values [nW, k] fp32 descending, class index [nW, k] int32 into gallery.class_ids) of every window of a PackedOutput or a
        StreamOutput (of out.smoothed with smoothed=True); ties go to the lower index.  Of a session with a class list of its own, and of
        a GroupedPackedOutput, the index counts within that session's list, and k is at most the shortest list of a session with windows."""
        if isinstance(out, GroupedPackedOutput):
            return self._topk_grouped(out, k, smoothed)
        if hasattr(out, "columns"):                # of a pool with a shortlist: the index counts in gallery.class_ids, NONE where the
            return self._topk_shortlist(out, k, smoothed)                     # session's list is shorter than k
        src = out.smoothed if smoothed else out.logits
        if src is None:
            raise ValueError("StreamPool.topk: this output has no smoothed scores (smooth = 0)")
        nW, C = src.shape
        if not 1 <= k <= min(ghip.TOPK_MAX, max(1, C)):
            raise ValueError("StreamPool.topk: k must be in [1, min(16, number of classes)], got %d" % k)
        values = torch.empty(nW, k, device=src.device, dtype=torch.float32)
        index = torch.empty(nW, k, device=src.device, dtype=torch.int32)
        if nW:
            ghip.topk(src.contiguous(), k, values, index)
        return values, index

    # ------------------------------------------------------------------ history search
    def _history_tables(self, rnd, recs, done):
        """the two tables of one round in one upload -> (the ring's, as _tables.upload(rnd.rows) gives it; the history store's: the same
        rows with PUT_POS counting modulo F and no windows, for the ring's own kernel to write the round's rows right beside the ring
        write).  done: the frames of each session the push's earlier rounds wrote, advanced here."""
        F = self._history.frames
        if self._hs_store is None:
            self._hs_store = torch.empty(self.max_streams, F, self.E, device=self.dev, dtype=torch.float32)
        rows = []
        for i, r in zip(rnd.members, rnd.rows):
            rows.append([r[php.SLOT], (recs[i].t + done[i]) % F, r[php.N], r[php.FEAT_OFF], 0, 0, 0, 0])
            done[i] += r[php.N]
        both, S = self._hs_tables.upload(rnd.rows + rows), len(rows)
        return php.Table(both.host[:S], both.dev[:S], S), php.Table(both.host[S:], both.dev[S:], S)

    def _need_history(self, what):
        if self._history is None:
            raise ValueError("StreamPool.%s: this pool keeps no history (build it with history=History(frames=...))" % what)

    def searchable(self, h):
        """range of the session's window numbers that search() scans and the *_hit methods accept: complete, and their first frame
        still in the history store"""
        self._need_history("searchable")
        return enrolable_windows(self._session(h).t, self.T, self.stride, self.rate, self._history.frames)

    def search(self, classes, sessions=None, top=16, min_score=None, separation=None, last=None, tempo=None):
        """Where did `classes` (1 to 64 registered ids, no repeats) happen in the windows the history still holds?  -> SearchResult
        (clip_fsar_amd.history, which states the plane and the rule): hits {class id: [Hit(session, class_id, window, score, tempo)],
        best first}, at most `top` per class and no two of one session and class within `separation` windows of each other (default:
        the largest distance at which two windows share a frame); peaks {class id: the count before top cut it}; windows scanned; the
        plane scores [NW, K] on the device with its sessions, first_window and offsets.  sessions: None -- every open session in handle
        order -- or a list, in that order; min_score: only scores >= it (as fp32) count; last=n: only windows completed by one of a
        session's newest n frames; tempo (a pool with rates=): the index into rates at which every window is read, None: the last.
        One gather and one classify_features per chunk of windows, two launches for the peaks, one synchronisation.  Changes nothing."""
        self._need_history("search")
        what = "StreamPool.search"
        g = self.gallery
        from .live_gallery import plan_columns
        ids = list(classes) if isinstance(classes, (list, tuple)) else None
        if ids is None:
            raise TypeError("%s: classes must be a list of registered class ids, got %s" % (what, type(classes).__name__))
        plan_columns(g._book, ids, what)
        if len(ids) > hship.MAX_CLASSES:
            raise ValueError("%s: %d classes -- one search takes 1 to %d; split the list" % (what, len(ids), hship.MAX_CLASSES))
        if sessions is None:
            handles = self.sessions
        else:
            handles = list(sessions) if isinstance(sessions, (list, tuple)) else None
            if handles is None:
                raise TypeError("%s: sessions must be None or a list of open sessions, got %s" % (what, type(sessions).__name__))
            if len(set(handles)) != len(handles):
                raise ValueError("%s: a session appears twice in sessions=: %r" % (what, handles))
        recs = [self._session(h) for h in handles]
        check_top(top, what)
        floor = check_min_score(min_score, what)
        sep = check_separation(((self.T - 1) * self.rate) // self.stride if separation is None else separation, what)
        if last is not None and (isinstance(last, bool) or not isinstance(last, int) or last < 1):
            raise ValueError("%s: last must be None or an integer >= 1 (frames), got %r" % (what, last))
        rate, shift = self._tempo(tempo, "search")
        at_tempo = None if self.rates is None else (len(self.rates) - 1 if tempo is None else tempo)
        T, K, F = self.T, len(ids), self._history.frames
        plan = plan_search([(s.slot, s.t) for s in recs], T, self.stride, self.rate, F, last, shift)
        NW = plan.offsets[-1]
        sep = device_separation(sep, plan.n_windows, what)
        if NW * K > hship.MAX_PLANE:
            raise ValueError("%s: %d windows x %d classes -- a plane holds at most 2^30 scores; search fewer sessions or classes, or "
                             "give last=" % (what, NW, K))
        scores = torch.empty(NW, K, device=self.dev, dtype=torch.float32)
        result = lambda hits, peaks: SearchResult(dict(zip(ids, hits)), dict(zip(ids, peaks)), NW, scores, handles, plan.first_window,
                                                  plan.offsets)
        if not NW:                                 # nothing is held (or no session is open): nothing is launched
            return result([[] for _ in ids], [0] * K)
        eng = self._ready()
        table = self._hs_tables.upload(plan.rows)
        per = max(1, eng.max_frames // T)          # classify_features scores that many clips per chunk: gather no more at a time
        if self._hs_X is None or self._hs_X.shape[0] < min(NW, per):
            self._hs_X = torch.empty(min(NW, per), T, self.E, device=self.dev, dtype=torch.float32)
        for w0 in range(0, NW, per):
            w1 = min(NW, w0 + per)
            X = self._hs_X[:w1 - w0]
            php.window_sequences(self._hs_store, X, table, NW, w0, w1, T, self.stride, rate)
            scores[w0:w1].copy_(g.classify_features(X, classes=ids))
        # the records in one buffer, so that one copy brings them down: n_hits [K], n_peaks [K], hit_rows [K, top], hit_scores [K, top]
        buf = torch.empty(2 * K + 2 * K * top, device=self.dev, dtype=torch.int32)
        n_hits, n_peaks = buf[:K], buf[K:2 * K]
        hit_rows = buf[2 * K:2 * K + K * top].view(K, top)
        hit_scores = buf[2 * K + K * top:].view(torch.float32).view(K, top)
        work = self._work("_hs_work", hship.workspace_words(NW, K))
        hship.peaks(scores, work, hit_rows, hit_scores, n_hits, n_peaks, table, sep, floor, top)
        host = buf.cpu()                           # the search's one synchronisation
        counts, peaks = host[:K].tolist(), host[K:2 * K].tolist()
        rows = host[2 * K:2 * K + K * top].view(K, top).tolist()
        values = host[2 * K + K * top:].view(torch.float32).view(K, top).tolist()
        owner = [i for i, n in enumerate(plan.n_windows) for _ in range(n)]          # plane row -> its session's place in the search
        hits = []
        for c, n, rr, vv in zip(ids, counts, rows, values):
            order = sorted(range(n), key=lambda j: (-vv[j], rr[j]))                  # descending score, then plane row
            hits.append([Hit(handles[owner[rr[j]]], c, plan.first_window[owner[rr[j]]] + rr[j] - plan.offsets[owner[rr[j]]], vv[j], at_tempo)
                         for j in order])
        return result(hits, peaks)

    def _held_hit(self, h, what):
        """every refusal of a *_hit method -> (the session's record, the store position of the first frame of the hit's window read
        at the hit's tempo, the rate it is read at)"""
        self._need_history(what)
        if not isinstance(h, Hit):
            raise TypeError("StreamPool.%s: takes a Hit that search() returned, got %s" % (what, type(h).__name__))
        s = self._session(h.session)
        rate, shift = self._tempo(h.tempo, what)
        F = self._history.frames
        plan = plan_enroll([(s.slot, s.t)], [(0, h.window)], self.T, self.stride, self.rate, F, names=["StreamPool: session %d" % h.session])
        return s, (plan.positions[0] + shift) % F, rate

    def hit_features(self, h):
        """[T, E] fp32, a copy: the tower rows of a hit's window (read at the hit's tempo) out of the history store, as long as
        h.window is in searchable(h.session).  One launch, the one enroll reads the ring with."""
        s, pos, rate = self._held_hit(h, "hit_features")
        zero = torch.zeros(1, self.E, device=self.dev, dtype=torch.float32)           # the closing row of a support sequence: dropped
        return self._ring_sequences(zero, [s.slot], [pos], [0], rate, ring=self._hs_store)[0, :self.T].clone()

    def explain_hit(self, h, classes=None, k=None):
        """explain() of a hit: the OTAM soft alignment of its window against `classes` (default: the hit's own class) or against its
        top-k classes -> clip_fsar_amd.align.Alignment of one clip, through Aligner.align_features.  Changes nothing."""
        self._held_hit(h, "explain_hit")
        al = self._the_aligner()
        if classes is None and k is None:
            classes = [h.class_id]
        return al.align_features(self.hit_features(h).unsqueeze(0), classes, k)

    def enroll_hit(self, h, class_id, text=None):
        """enroll() of a hit: its window becomes a shot of class_id -- of a registered class a further one, of an unknown id the first
        of a new class (its text from TEST.CLASS_NAME or from `text`, {class id: name or [E] row}) -> the class's shot count.
        Through the gallery's add_shots_features / add_classes_features; nothing of any session changes."""
        self._held_hit(h, "enroll_hit")
        g = self._enrolling_gallery()
        cid = g._shot_ids([class_id])[0]
        feats = self.hit_features(h).unsqueeze(0)
        if cid in g._book.slot_of:
            return list(g.add_shots_features(feats, [cid]))[0]
        g.add_classes_features(feats, [cid], text)
        return 1

    # ------------------------------------------------------------------ timeline
    def _timeline_tables(self, rows, recs):
        """_class_push's upload of a pool with timeline=: the push's table, and behind it -- in the same upload, six to a row -- the
        first window number of every row's session (its frame counter has not moved yet) -> the table as upload(rows) gives it; the
        first numbers wait in _tl_first for _fold"""
        S, cols = len(rows), cship.TABLE_COLS
        if self._smooth_tables is None:
            self._smooth_tables = cship.table_uploader(self.dev, self.max_streams + -(-self.max_streams // cols))
        first = [window_plan(s.t, 0, self.T, self.stride, self.rate)[0] for s in recs]
        first += [0] * (-len(first) % cols)
        both = self._smooth_tables.upload(rows + [first[i:i + cols] for i in range(0, len(first), cols)])
        self._tl_first = cship.Table(both.host[S:].view(-1)[:S], both.dev[S:].view(-1)[:S], S)
        return cship.Table(both.host[:S], both.dev[:S], S)

    def _fold(self, cp, scores):
        """one cftl_fold over the push's session-major plane `scores` (dense [NW, C] or the grouped layout), on the table and keys
        every keyed launch of the push takes: no synchronisation, nothing returned"""
        tl = self._timeline
        _, gens, keys, table = cp
        tlhip.fold(scores.view(-1), *self._tl_cells.at(gens.shape[0]), gens, keys, table, self._tl_first, tl.span, tl.level)

    def _need_timeline(self, what):
        if self._timeline is None:
            raise ValueError("StreamPool.%s: this pool keeps no timeline (build it with timeline=Timeline(...))" % what)

    def _held_buckets(self, s, last, what):
        """the buckets the timeline still holds of a session, from the host's counters"""
        if last is not None and (isinstance(last, bool) or not isinstance(last, int) or last < 1):
            raise ValueError("StreamPool.%s: last must be None or an integer >= 1 (buckets), got %r" % (what, last))
        tl = self._timeline
        return held_buckets(window_plan(0, s.t, self.T, self.stride, self.rate)[1], tl.span, tl.buckets, last)

    def _read_buckets(self, slots, buckets, K, keys):
        """one cftl_read: the buckets `buckets[i]` (a range) of slot slots[i] over the K store slots `keys` (a device list, shared by
        every row) -> (peak, at, above), each [sum of the ranges' lengths, K] on the device, the rows one after the other"""
        rows, n_out = read_rows(slots, buckets, [K] * len(slots), [0] * len(slots))
        peak = torch.empty(n_out // K, K, device=self.dev, dtype=torch.float32)
        at = torch.empty(n_out // K, K, device=self.dev, dtype=torch.int32)
        above = torch.empty_like(at)
        if n_out:
            if self._tl_tables is None:
                self._tl_tables = (tlhip.read_uploader(self.dev, self.max_streams), php.TableUploader(self.dev, self.max_streams))
            gens = self.gallery.slot_generations()
            tlhip.read(*self._tl_cells.at(gens.shape[0]), gens, keys, peak.view(-1), at.view(-1), above.view(-1),
                       self._tl_tables[0].upload(rows), self._timeline.span)
        return peak, at, above

    def timeline(self, h, classes=None, last=None):
        """What the session saw, bucket by bucket -> TimelineView(first_bucket, span, class_ids, peak, at, above): row i of the planes
        [nb, K] (on the device; fp32, int32, int32) is bucket first_bucket + i, the windows (first_bucket + i) * span + 0 .. span - 1,
        and holds per class the bucket's highest score, the window it belongs to and the count of windows at or above the timeline's
        level -- (-inf, -1, 0) where the pair has no live cell (clip_fsar_amd.timeline states the rule).  The buckets are those still
        held, max(0, bn - B + 1) .. bn with bn the bucket of the session's newest window; last=n: the newest n of them; a session
        without a window gives empty planes.  classes: ids of the session's columns, in the order given; None: all of them, in their
        order.  One cftl_read, no synchronisation; changes nothing."""
        self._need_timeline("timeline")
        what = "StreamPool.timeline"
        s = self._session(h)
        g = self.gallery
        from .live_gallery import plan_columns
        if classes is None:
            ids = list(g._book.order if s.classes is None else s.classes)
            plan_columns(g._book, ids or None, what)
        else:
            ids = list(classes) if isinstance(classes, (list, tuple)) else None
            if ids is None:
                raise TypeError("%s: classes must be None or a list of registered class ids, got %s" % (what, type(classes).__name__))
            plan_columns(g._book, ids, what)
            for c in ids:
                if s.classes is not None and c not in s.classes:
                    raise ValueError("%s: class %r is not registered (classes= of session %d)" % (what, c, h))
        buckets = self._held_buckets(s, last, "timeline")
        K = len(ids)
        if not len(buckets) or not K:
            empty = lambda dtype: torch.empty(0, K, device=self.dev, dtype=dtype)
            return TimelineView(buckets.start, self._timeline.span, tuple(ids), empty(torch.float32), empty(torch.int32), empty(torch.int32))
        keys = g._columns(None) if classes is None and s.classes is None else \
            torch.tensor([g._book.slot_of[c] for c in ids], device=self.dev, dtype=torch.int32)
        return TimelineView(buckets.start, self._timeline.span, tuple(ids), *self._read_buckets([s.slot], [buckets], K, keys))

    def recall(self, classes, sessions=None, top=16, min_score=None, separation=1, last=None):
        """When were `classes` (1 to 64 registered ids, no repeats) strongest, in the buckets the timeline still holds?  -> RecallResult:
        hits {class id: [Hit(session, class_id, window, score, tempo=None)], best first} -- window the peak's own window, so a hit goes
        into explain / enroll while the ring holds it and, on a pool with history=, into hit_features / explain_hit / enroll_hit; each
        hit also carries .bucket and .above --, peaks {class id: the count before top cut it}, buckets scanned.  The rule is
        clip_fsar_amd.history.reference_search on the plane of bucket peaks, session-major in the order of `sessions` (None: every open
        session in handle order), buckets ascending: `separation` counts buckets, min_score and top are search()'s.  last=n: the newest
        n buckets of every session.  One cftl_read, the two launches of the history's peak search, a gather; one synchronisation.
        Nothing is scored, and nothing changes."""
        self._need_timeline("recall")
        what = "StreamPool.recall"
        g = self.gallery
        from .live_gallery import plan_columns
        ids = list(classes) if isinstance(classes, (list, tuple)) else None
        if ids is None:
            raise TypeError("%s: classes must be a list of registered class ids, got %s" % (what, type(classes).__name__))
        slots = plan_columns(g._book, ids, what)
        if len(ids) > hship.MAX_CLASSES:
            raise ValueError("%s: %d classes -- one recall takes 1 to %d; split the list" % (what, len(ids), hship.MAX_CLASSES))
        if sessions is None:
            handles = self.sessions
        else:
            handles = list(sessions) if isinstance(sessions, (list, tuple)) else None
            if handles is None:
                raise TypeError("%s: sessions must be None or a list of open sessions, got %s" % (what, type(sessions).__name__))
            if len(set(handles)) != len(handles):
                raise ValueError("%s: a session appears twice in sessions=: %r" % (what, handles))
        recs = [self._session(h) for h in handles]
        check_top(top, what)
        floor = check_min_score(min_score, what)
        sep = check_separation(separation, what)
        buckets = [self._held_buckets(s, last, "recall") for s in recs]
        counts = [len(b) for b in buckets]
        NB, K = sum(counts), len(ids)
        sep = device_separation(sep, counts, what)
        if NB * K > hship.MAX_PLANE:
            raise ValueError("%s: %d buckets x %d classes -- a plane holds at most 2^30 scores; recall fewer sessions or classes, or "
                             "give last=" % (what, NB, K))
        if not NB:                                 # nothing is held (or no session is open): nothing is launched
            return RecallResult({c: [] for c in ids}, {c: 0 for c in ids}, 0)
        keys = torch.tensor(slots, device=self.dev, dtype=torch.int32)
        peak, at, above = self._read_buckets([s.slot for s in recs], buckets, K, keys)
        offsets = [0]
        for n in counts:
            offsets.append(offsets[-1] + n)
        table = self._tl_tables[1].upload([[s.slot, 0, 0, 0, 0, n, off, 0] for s, n, off in zip(recs, counts, offsets)])
        # the records in one buffer, so that one copy brings them down: n_hits [K], n_peaks [K], then [K, top] each of hit_rows,
        # hit_scores, the hits' windows and their counts
        buf = torch.empty(2 * K + 4 * K * top, device=self.dev, dtype=torch.int32)
        n_hits, n_peaks = buf[:K], buf[K:2 * K]
        part = lambda i: buf[2 * K + i * K * top:2 * K + (i + 1) * K * top].view(K, top)
        hit_rows, hit_scores = part(0), part(1).view(torch.float32)
        work = self._work("_tl_work", hship.workspace_words(NB, K))
        hship.peaks(peak, work, hit_rows, hit_scores, n_hits, n_peaks, table, sep, floor, top)
        where = hit_rows.clamp(max=NB - 1).long().t()                                # [top, K]: an unused place reads the last row
        part(2).copy_(at.gather(0, where).t())
        part(3).copy_(above.gather(0, where).t())
        host = buf.cpu()                           # the recall's one synchronisation
        n, peaks = host[:K].tolist(), host[K:2 * K].tolist()
        hpart = lambda i: host[2 * K + i * K * top:2 * K + (i + 1) * K * top].view(K, top)
        rows, values = hpart(0).tolist(), hpart(1).view(torch.float32).tolist()
        windows, aboves = hpart(2).tolist(), hpart(3).tolist()
        owner = [i for i, m in enumerate(counts) for _ in range(m)]                  # plane row -> its session's place in the recall
        hits = {}
        for k, c in enumerate(ids):
            order = sorted(range(n[k]), key=lambda j: (-values[k][j], rows[k][j]))   # descending score, then plane row
            hits[c] = [RecallHit(handles[owner[rows[k][j]]], c, windows[k][j], values[k][j], None,
                                 bucket=buckets[owner[rows[k][j]]].start + rows[k][j] - offsets[owner[rows[k][j]]], above=aboves[k][j])
                       for j in order]
        return RecallResult(hits, dict(zip(ids, peaks)), NB)
