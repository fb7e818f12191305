"""Timeline: what did a session see, class by class, long after its ring moved on?

    p = StreamPool(live_gallery, timeline=Timeline(span=16, buckets=256, level=0.6))        # keyword-only; a gallery with a slot store
    a = p.open(); p.push({a: frames})                        # pushes return what they return without the option, bit for bit
    v = p.timeline(a)                                        # classes=None, last=None -> TimelineView
    v.first_bucket, v.span, v.class_ids                      # bucket i of the view holds the windows (first_bucket + i) * span + 0 .. span-1
    v.peak, v.at, v.above                                    # [nb, K] on the device: fp32, int32, int32
    r = p.recall([7, "kite"], top=16)                        # sessions=None, min_score=None, separation=1 (buckets), last=None
    r.hits[7]                                                # [Hit(session, class_id, window, score, tempo=None)], best first; .bucket, .above
    p.explain(h.session, [h.class_id], window=h.window)      # while the ring holds the window; hit_features(h) with history=

THE RULE.  The pool scores every (session, window, class) at every push.  The timeline folds the plane `of` -- None: the judged plane,
as leaders() defines it, deviation with a baseline, else smoothed with per-class smoothing, else logits; or one of those three by
name -- into BUCKETS of `span` windows in the push that made the scores.  Window w of a session (its own number, the one
out.first_window counts) lies in bucket b = w // span, and bucket b lives at position b % B of a ring of B = `buckets` buckets.  The
state planes are [max_streams, B, cap], cap the gallery's store capacity: peak fp32, at int32, above int32, marks int32.  With gens
[cap] the store slots' generations (LiveGallery.slot_generations), the cell of (session slot, bucket b, store slot key) is LIVE FOR b
iff marks == gens[key] and at >= 0 and at // span == b; any other cell stands for the empty one, peak = -inf, at = -1, above = 0.  The
peak's own window number says which lap of the ring a cell belongs to, so a cell carries no bucket tag, and open(), reset(), a
removal, a slot's reuse and a class joining a list start a pair's cells anew exactly as they restart its smoothing state.

A CANDIDATE is a score that is neither NaN nor -inf (the contest's and the history's definition: +inf is one).  The fold runs over a
row's windows in ascending order.  A candidate s at window w replaces the peak when the cell is empty or s > peak -- strictly, so a tie
keeps the earlier window, and since -0.0 == +0.0 the peak keeps the bits of the first; above += 1 when level is None, or s >= level as
fp32.  When the fold leaves a cell -- at a bucket change or at the row's end -- it writes the cell iff at >= 0: the three values and
marks = gens[key].  A cell that saw no candidate is not touched.  The state therefore does not depend on how a session's windows were
cut into pushes.

This module is the host half and is pure Python / numpy: the option's type and reference_fold / reference_read, the two kernels of
libclipfsar_timeline.so (include/ext/clipfsar_timeline.h) restated on the CPU, which they are compared against bit for bit.  recall()'s
rule is clip_fsar_amd.history.reference_search on the plane of bucket peaks.
"""
from __future__ import annotations

import collections
import math

import numpy as np

from .history import Hit

MAX_SPAN = 1 << 20                       # CFTL_MAX_SPAN
MAX_BUCKETS = 1 << 16                    # CFTL_MAX_BUCKETS
PLANES = ("logits", "smoothed", "deviation")
# the fold's table (class_smooth's) and the read's, column by column
SLOT, NW, OUT0, NC, KEY0, CHUNK0 = range(6)
R_SLOT, R_B0, R_NB, R_NC, R_KEY0, R_OUT0, R_CHUNK0 = range(7)
CHUNK = 256                              # CFTL_CHUNK


class Timeline(collections.namedtuple("Timeline", "span buckets level of")):
    """span: windows per bucket, 1 .. 2^20; buckets: the length B of the bucket ring, 1 .. 65536; level: None -- `above` counts every
    candidate -- or a number that is finite as fp32, held as that fp32 value; of: None (the judged plane), "logits", "smoothed" or
    "deviation" """
    __slots__ = ()

    def __new__(cls, span=16, buckets=256, level=None, of=None):
        for name, v, hi in (("span", span, MAX_SPAN), ("buckets", buckets, MAX_BUCKETS)):
            if isinstance(v, bool) or not isinstance(v, int) or not 1 <= v <= hi:
                raise ValueError("Timeline: %s must be an integer in [1, %d], got %r" % (name, hi, v))
        if level is not None:
            if isinstance(level, bool) or not isinstance(level, (int, float)) or not math.isfinite(level):
                raise ValueError("Timeline: level must be None or a finite number, got %r" % (level,))
            with np.errstate(over="ignore"):
                as32 = float(np.float32(level))
            if not math.isfinite(as32):
                raise ValueError("Timeline: level must be finite as fp32, got %r" % (level,))
            level = as32
        if of is not None and of not in PLANES:
            raise ValueError("Timeline: of must be None, \"logits\", \"smoothed\" or \"deviation\", got %r" % (of,))
        return super().__new__(cls, span, buckets, level, of)


# first_bucket: the bucket of the planes' row 0; class_ids: of their columns; peak / at / above [nb, K] on the device
TimelineView = collections.namedtuple("TimelineView", "first_bucket span class_ids peak at above")
# hits, peaks: {class id: ...} in the order of the recall's classes; buckets: the buckets scanned
RecallResult = collections.namedtuple("RecallResult", "hits peaks buckets")


class RecallHit(Hit):
    """history.Hit of a recall -- the same tuple, `window` the peak's own window and tempo None -- and .bucket, the bucket the peak
    lies in, and .above, the bucket's count of windows at or above the timeline's level"""

    def __new__(cls, *fields, bucket, above):
        self = super().__new__(cls, *fields)
        self.bucket, self.above = bucket, above
        return self


def held_buckets(n_windows, span, B, last=None):
    """the buckets a session with n_windows completed windows still holds, as a range: max(0, bn - B + 1) .. bn with
    bn = (n_windows - 1) // span; last=n: the newest n of them"""
    if n_windows < 1:
        return range(0)
    bn = (n_windows - 1) // span
    lo = max(0, bn - B + 1)
    if last is not None:
        lo = max(lo, bn - last + 1)
    return range(lo, bn + 1)


def read_rows(slots, buckets, widths, key0s):
    """cftl_read's table: per row its slot, its range of buckets, its width and where its list starts in keys -> (rows, NOUT)"""
    rows, n_out, chunks = [], 0, 0
    for slot, bs, nc, key0 in zip(slots, buckets, widths, key0s):
        rows.append([int(slot), bs.start if len(bs) else 0, len(bs), int(nc), int(key0), n_out, chunks])
        n_out += len(bs) * int(nc)
        chunks += -(-int(nc) // CHUNK)
    return rows, n_out


def new_state(max_streams, B, cap):
    """(peak, at, above, marks) as numpy planes [max_streams, B, cap] of a pool that has folded nothing: marks 0, the rest arbitrary"""
    return (np.zeros((max_streams, B, cap), np.float32), np.zeros((max_streams, B, cap), np.int32),
            np.zeros((max_streams, B, cap), np.int32), np.zeros((max_streams, B, cap), np.int32))


def _cell(state, gens, slot, pos, key, b, span):
    """the cell as the fold and the read see it for bucket b -> (peak, at, above, what it was: "live", "lap" -- this generation's cell
    of another lap --, "empty" -- this generation's mark over at < 0 --, "stale" -- written under another generation --, "never")"""
    peak, at, above, marks = state
    m, a = int(marks[slot, pos, key]), int(at[slot, pos, key])
    if m == int(gens[key]):
        if a >= 0 and a // span == b:
            return peak[slot, pos, key], a, int(above[slot, pos, key]), "live"
        return np.float32(-np.inf), -1, 0, ("lap" if a >= 0 else "empty")      # (the fold never writes at < 0: a hand-made cell)
    return np.float32(-np.inf), -1, 0, ("never" if m == 0 else "stale")


def reference_fold(state, gens, rows, keys, scores, first, span, B, level):
    """cftl_fold on the host.  state: (peak, at, above, marks), numpy planes [max_streams, B, cap], CHANGED IN PLACE; gens [cap]; rows:
    the 6-column table; keys: the flat key lists; scores: the flat fp32 scores; first: each row's first window number; level: None or
    a number, compared as fp32 -> {"ties": candidates equal to a standing peak, which kept its window; "replaced": candidates that
    took a standing peak's place; "laps": cells of an earlier lap overwritten; "restarted": cells written under another generation
    overwritten} of this call."""
    peak, at, above, marks = state
    cap = peak.shape[2]
    scores = np.asarray(scores, dtype=np.float32).reshape(-1)
    lvl = None if level is None else np.float32(level)
    counts = dict(ties=0, replaced=0, laps=0, restarted=0)
    for row, w0 in zip(rows, first):
        slot, nW, out0, nc, key0 = (int(row[c]) for c in (SLOT, NW, OUT0, NC, KEY0))
        for j in range(nc):
            key = int(keys[key0 + j])
            if nW == 0 or not 0 <= key < cap:
                continue
            k = 0
            while k < nW:
                w = int(w0) + k
                b = w // span
                pos = b % B
                p, a, n, was = _cell(state, gens, slot, pos, key, b, span)
                while k < nW and (int(w0) + k) // span == b:
                    s = scores[out0 + k * nc + j]
                    if not np.isnan(s) and s != -np.inf:
                        if a < 0 or s > p:
                            counts["replaced"] += a >= 0
                            p, a = s, int(w0) + k
                        elif s == p:
                            counts["ties"] += 1
                        if lvl is None or s >= lvl:
                            n += 1
                    k += 1
                if a >= 0:
                    counts["laps"] += was == "lap"
                    counts["restarted"] += was == "stale"
                    peak[slot, pos, key], at[slot, pos, key], above[slot, pos, key] = p, a, n
                    marks[slot, pos, key] = gens[key]
    return counts


def reference_read(state, gens, rows, keys, span, B):
    """cftl_read on the host.  rows: the 7-column table -> (out_peak fp32, out_at int32, out_above int32), flat, each row's row-major
    [NB, NC] block at its OUT0"""
    cap = state[0].shape[2]
    n_out = sum(int(r[R_NB]) * int(r[R_NC]) for r in rows)
    out_peak, out_at, out_above = np.empty(n_out, np.float32), np.empty(n_out, np.int32), np.empty(n_out, np.int32)
    for row in rows:
        slot, b0, nb, nc, key0, out0 = (int(row[c]) for c in (R_SLOT, R_B0, R_NB, R_NC, R_KEY0, R_OUT0))
        for i in range(nb):
            for j in range(nc):
                key = int(keys[key0 + j])
                if 0 <= key < cap:
                    p, a, n, _ = _cell(state, gens, slot, (b0 + i) % B, key, b0 + i, span)
                else:
                    p, a, n = np.float32(np.nan), -1, 0
                o = out0 + i * nc + j
                out_peak[o], out_at[o], out_above[o] = p, a, n
    return out_peak, out_at, out_above
