"""Stream events: onsets and offsets per (session, class) of a stream pool, detected on the device.

    rule = EventRule(on=0.6, off=0.4, min_on=2, min_off=2)       # hysteresis: on >= off, both finite; min_on, min_off >= 1
    p = StreamPool(live_gallery, smooth=0.5, smooth_by="class", events=rule)
    p.push_features({a: fa, b: fb})                               # returns what it returns without a rule; does not synchronise
    for e in p.take_events():                                     # synchronises once
        e.session, e.class_id, e.kind, e.window, e.start, e.length, e.score, e.peak
    p.active(a)                                                   # [(class_id, length, peak)] of the session's running events

The rule is one state machine per (session, class) pair over the pair's scores s_k in window order -- the pair's smoothed score when the
pool smooths by class, else its logit or probability:

  idle     s >= on extends a streak (peak: its maximum); the min_on-th consecutive such window is the ONSET (length min_on, start = that
           window - min_on + 1).  s < on, or NaN, ends the streak.
  active   every window extends the event (length + 1, peak = max); s < off extends a run below off, anything else (NaN included) ends
           that run; its min_off-th consecutive window is the OFFSET (length: the event's windows up to the run, start = where the
           onset's streak began).

The window that confirms one transition never counts towards the other.  A pair starts idle at its first window after the session's
open() or reset(), after the class's registration and after the class joined the session's list, exactly where per-class smoothing starts
anew; nothing else disturbs it.  A class that is removed, and a session that is closed or reset, end their events silently: no offset is
reported for them.

This module is the host half and is pure: the rule, the event type, reference_events (the machine restated in Python, what the kernels of
libclipfsar_events.so are tested against bit for bit) and the translator from the device's records to Event tuples.  The thresholds are
compared as fp32, which is how the C ABI takes them.
"""
from __future__ import annotations

import collections
import math
import struct

ONSET, OFFSET = 1, 2                     # a record's kind (CFEV_ONSET, CFEV_OFFSET)
KINDS = {ONSET: "onset", OFFSET: "offset"}
INT32_MAX = (1 << 31) - 1

Event = collections.namedtuple("Event", "session class_id kind window start length score peak")
# One record of the device: window k within the windows of its call, kind, len, the score at k and the peak.
Record = collections.namedtuple("Record", "k kind len score peak")
Cell = collections.namedtuple("Cell", "streak length peak")
IDLE = Cell(0, 0, 0.0)                   # how a cell without a valid mark starts


def _fp32(v):
    """v rounded to fp32, as the C ABI receives it (beyond fp32's range: an infinity)"""
    try:
        return struct.unpack("f", struct.pack("f", v))[0]
    except OverflowError:
        return math.copysign(math.inf, v)


class EventRule(collections.namedtuple("EventRule", "on off min_on min_off max_events")):
    """on, off: thresholds, off <= on, finite; min_on, min_off: windows that confirm a transition, >= 1; max_events: records a push
    can hand over, >= 1 (more are counted as dropped)"""
    __slots__ = ()

    def __new__(cls, on, off, min_on=1, min_off=1, max_events=4096):
        for name, v in (("on", on), ("off", off)):
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(_fp32(v)):
                raise ValueError("EventRule: %s must be a finite number (as fp32), got %r" % (name, v))
        if _fp32(off) > _fp32(on):
            raise ValueError("EventRule: off = %r must not exceed on = %r" % (off, on))
        for name, v in (("min_on", min_on), ("min_off", min_off), ("max_events", max_events)):
            if isinstance(v, bool) or not isinstance(v, int) or not 1 <= v <= INT32_MAX:
                raise ValueError("EventRule: %s must be an integer in [1, 2^31), got %r" % (name, v))
        return super().__new__(cls, float(on), float(off), min_on, min_off, max_events)


def _fmax(a, b):
    """fmaxf: the other operand when one is NaN"""
    if b != b:
        return a
    if a != a:
        return b
    return a if a >= b else b


def reference_events(scores, rule, cell=None):
    """The machine of one (session, class) pair over its consecutive scores (floats holding fp32 values), from `cell` (a Cell, or None:
    idle) -> ([Record], the Cell it leaves).  Running it over a series in pieces, each from the cell the piece before left, gives the
    records of one run with k counted from each piece's start."""
    on, off = _fp32(rule.on), _fp32(rule.off)
    streak, length, peak = IDLE if cell is None else cell
    records = []
    for k, s in enumerate(scores):
        if streak >= 0:
            if s >= on:
                peak = s if streak == 0 else _fmax(peak, s)
                streak += 1
                if streak == rule.min_on:
                    records.append(Record(k, ONSET, rule.min_on, s, peak))
                    streak, length = -1, rule.min_on
            else:
                streak = 0
        else:
            length = min(length + 1, INT32_MAX)
            peak = _fmax(peak, s)
            below = -streak if s < off else 0
            if below == rule.min_off:
                records.append(Record(k, OFFSET, length - rule.min_off, s, peak))
                streak = 0
            else:
                streak = -1 - below
    return records, Cell(streak, length, peak)


def translate(events, values, n, sessions, first_window, class_ids, rule):
    """The records of one push -> [Event].  events: rows (table row, column, window k, kind, len), values: rows (score, peak) -- lists, or
    tensors on the host -- of which the first min(n, len(events)) count; sessions, first_window, class_ids: per table row the session's
    handle, the number of its first window of the push and its columns' class ids, as they were when the push was made.  Order: the
    sessions as pushed, then window, then column.  window = first_window[row] + k; an onset starts at window - min_on + 1, an offset's
    event at window - min_off - length + 1."""
    if hasattr(events, "tolist"):
        events = events.tolist()
    if hasattr(values, "tolist"):
        values = values.tolist()
    kept = min(int(n), len(events))
    out = []
    for (row, j, k, kind, ln), (score, peak) in sorted(zip(events[:kept], values[:kept]), key=lambda r: (r[0][0], r[0][2], r[0][1])):
        window = first_window[row] + k
        start = window - rule.min_on + 1 if kind == ONSET else window - rule.min_off - ln + 1
        out.append(Event(sessions[row], class_ids[row][j], KINDS[kind], window, start, ln, score, peak))
    return out
