"""Event evidence: an event's window kept after the session's ring has moved on.

    p = StreamPool(live_gallery, events=EventRule(on=0.6, off=0.4, min_on=2), evidence=Evidence(capacity=256, kinds=("onset",)))
    p.push_features({a: fa}); ...                 # any number of pushes, close() and reset() included
    for e in p.take_events():                     # EvidenceEvent: Event's eight fields, then evidence, missed, tempo
        if p.held(e):
            p.evidence_features(e)                # [T, E]: the tower rows of the window e.window, a copy
            p.explain_event(e)                    # clip_fsar_amd.align.Alignment of those rows against e.class_id
            p.enroll_event(e, "kite")             # "that one was actually kite": the rows become a shot

In the push that detects an event the T ring rows of its window are copied into a slot of a store on the device
(libclipfsar_evidence.so, clip_fsar_amd.evidence_hip: a placement pass and a row copy, driven by the detector's records while they are
still on the device -- no synchronisation).  The store is a ring of `capacity` slots: capture number s (its SERIAL, counted by the host
in the device's record order) lives in slot s mod capacity and is HELD until `capacity` later captures have overwritten it.  An event
whose window could not be captured says why in `missed`: "ring" (a push of several rounds had already overwritten the window), "capacity"
(more than `capacity` captures in one push) or "kind" (its kind is not among the Evidence's kinds).

This module is the host half and is pure: the option, the event type, and reference_capture, cfed_capture restated on CPU tensors, which
the kernels are tested against bit for bit.
"""
from __future__ import annotations

import collections

import torch

from .events import OFFSET, ONSET, Event

KIND_BITS = {"onset": 1, "offset": 2}            # CFED_KIND_ONSET, CFED_KIND_OFFSET
NOT_CAPTURED, LEFT_RING, NO_ROOM = -1, -2, -3    # where[i, 0] of a record without a slot
MISSED = {NOT_CAPTURED: "kind", LEFT_RING: "ring", NO_ROOM: "capacity"}
MAX_CAPACITY = 1 << 20
TABLE_COLS = 6
SLOT, POS0, NW, KEEP0, OUT0, NC = range(TABLE_COLS)

# evidence: the capture's serial, or None; missed: None, "ring", "capacity" or "kind"; tempo: the index into the pool's rates at which
# the window was read (the tempo that won the event's cell), None on a pool without rates= and for an event without evidence
EvidenceEvent = collections.namedtuple("EvidenceEvent", Event._fields + ("evidence", "missed", "tempo"))


class Evidence(collections.namedtuple("Evidence", "capacity kinds")):
    """capacity: slots of the store, an integer in [1, 2^20] -- a capture is held until `capacity` later ones have overwritten it;
    kinds: the events whose windows are captured, a non-empty subset of ("onset", "offset")"""
    __slots__ = ()

    def __new__(cls, capacity=256, kinds=("onset",)):
        if isinstance(capacity, bool) or not isinstance(capacity, int) or not 1 <= capacity <= MAX_CAPACITY:
            raise ValueError("Evidence: capacity must be an integer in [1, 2^20], got %r" % (capacity,))
        if isinstance(kinds, (str, bytes)) or not isinstance(kinds, (tuple, list)):
            raise TypeError("Evidence: kinds must be a tuple of \"onset\" and / or \"offset\", got %r" % (kinds,))
        kinds = tuple(kinds)
        if not kinds or len(set(kinds)) != len(kinds) or any(k not in KIND_BITS for k in kinds):
            raise ValueError("Evidence: kinds must be a non-empty subset of (\"onset\", \"offset\") without repeats, got %r" % (kinds,))
        return super().__new__(cls, capacity, tuple(k for k in KIND_BITS if k in kinds))

    @property
    def mask(self):
        """`kinds` as cfed_capture takes it: bit 0 onsets, bit 1 offsets"""
        return sum(KIND_BITS[k] for k in self.kinds)


def keep0(first_window, n_windows, stride, frames_after, cap):
    """KEEP0 of a table row: the smallest k in [0, n_windows] whose window first_window + k still has its first frame in a ring of cap
    frames that holds frames_after frames (the session's count after the push) -- the ring keeps the frames [frames_after - cap,
    frames_after); later frames of a window are newer still"""
    lost = max(0, frames_after - cap)            # frames below this one are overwritten
    first_kept = -(-lost // stride)              # the first window number whose first frame is kept
    return min(max(0, first_kept - first_window), n_windows)


def reference_capture(ring, events, n, tempo, table, head, store, kinds, T, stride, rate, rates=None):
    """cfed_capture on CPU tensors.  ring [max_streams, cap, E]; events [max_events, 5] int rows (row, j, k, kind, len); n: n_events;
    tempo: the flat tempo plane or None (with rates: the ascending rates, rates[-1] == rate); table: rows of TABLE_COLS ints; head: int
    in [0, capacity); store [capacity, T, E]; kinds: the bit mask -> (where [max_events, 2] int32, the new head, the new store -- a
    clone, `store` itself is left alone)."""
    ring = torch.as_tensor(ring)
    cap = ring.shape[1]
    rows = events.tolist() if hasattr(events, "tolist") else [list(r) for r in events]
    table = table.tolist() if hasattr(table, "tolist") else [list(r) for r in table]
    flat = None if tempo is None else torch.as_tensor(tempo).reshape(-1).tolist()
    if (flat is None) != (rates is None):
        raise ValueError("reference_capture: tempo and rates go together")
    store = store.clone()
    capacity, M = store.shape[0], len(rows)
    where = torch.full((M, 2), 0, dtype=torch.int32)
    where[:, 0] = NOT_CAPTURED
    rank = 0
    for i in range(min(max(int(n), 0), M)):
        row, j, k, kind, _ = rows[i]
        wanted = (kind == ONSET and kinds & 1) or (kind == OFFSET and kinds & 2)
        if not wanted or not 0 <= row < len(table):
            continue
        d = table[row]
        if not (0 <= k < d[NW] and 0 <= j < d[NC]):
            continue
        if k < d[KEEP0]:
            where[i, 0] = LEFT_RING
            continue
        if rank >= capacity:
            where[i, 0] = NO_ROOM
            rank += 1
            continue
        slot = (head + rank) % capacity
        rank += 1
        t, r, shift = 0, rate, 0
        if flat is not None:
            t = flat[d[OUT0] + k * d[NC] + j]
            t = len(rates) - 1 if not 0 <= t < len(rates) else t
            r = rates[t]
            shift = (T - 1) * (rates[-1] - r)
        for f in range(T):
            store[slot, f] = ring[d[SLOT], (d[POS0] + k * stride + shift + f * r) % cap]
        where[i, 0], where[i, 1] = slot, t
    return where, (head + min(rank, capacity)) % capacity, store
