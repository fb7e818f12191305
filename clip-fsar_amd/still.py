"""Still frames: the semantics of StreamPool(still=StillGate(...)) -- which frames of a pixel push skip the tower.  Pure Python and torch
on the CPU; the device side is libclipfsar_still.so (clip_fsar_amd.still_hip), which computes reference_changed's counts.

    pool = StreamPool(gallery, still=StillGate())                    # exact repeats skip the tower
    pool = StreamPool(gallery, still=StillGate(pixel_tol=0.02, changed=0.001, max_run=30))
    pool.push({a: frames}); pool.last_kept()                          # {a: (True, False, False, True, ..)}: which frames the tower saw
    pool.stats(a)["tower_frames"], pool.stats(a)["still_frames"]

THE MEASURE.  A frame is L = 3 * H * W fp32 values, as handed to the tower.  The change count of a frame x against its predecessor y is
the number of elements e with  not (|x[e] - y[e]| <= tol): the subtraction is ONE rounded fp32 operation, and tol is pixel_tol rounded
to fp32 once, on the host.  A NaN in either frame counts as changed, and so does inf - inf (a NaN); -0.0 against +0.0 does not.  The
count is an integer, so it is a bit-for-bit function of the inputs whatever the order of the reduction.  pixel_tol is in the units of
the tower's input, AFTER mean and std: one step of a uint8 pixel is 1 / (255 * std) there -- with DATA.STD = [0.229, 0.224, 0.225] that
is 0.0171, 0.0175 and 0.0174 in the three channels, so pixel_tol = 0.02 forgives one step of sensor noise and 0.04 two.

THE PREDECESSOR.  Within a push, frame j of a session has the push's frame j - 1 as predecessor; frame 0 has the newest frame of the
session's last pixel push, which the pool keeps in a store prev [max_streams, L].  A session has NO predecessor after open() (a reused
slot included: the previous owner's frame is never read), after reset(), and after any push_features* that included it -- its newest
frame is then not the one in prev.  The count of a frame without a predecessor is -1.

THE RULE (plan_still).  limit = floor(changed * L).  Each session's frames are walked in order; a frame is KEPT -- it goes through the
tower -- when its count is -1, when its count is above limit, or when the session's run of consecutive skipped frames has reached
max_run.  Otherwise it is SKIPPED: it receives the tower row of the frame before it (which may itself have been skipped: in the end the
row of the session's newest kept frame), and the run grows by one.  A kept frame sets the run to 0.  Runs carry over between pushes.

THE DRIFT BOUND.  With changed = 0 a skipped frame differs from its predecessor by at most pixel_tol in every element, so after a run of
r skipped frames every element of the r-th lies within r * pixel_tol of the frame whose tower row it received -- at most max_run *
pixel_tol.  With changed > 0 up to limit elements per step are not bounded at all.  With both tolerances 0 only exact repeats are
skipped, the row a frame receives is the row the tower would have computed for it up to the tower's own batch dependence, and
max_run=None (unlimited) is safe.
"""
from __future__ import annotations

import math

import torch


class StillGate:
    """pixel_tol: an element changed when it differs from the predecessor's by more than this (finite, >= 0; tower-input units);
    changed: a frame is still when at most floor(changed * L) of its L elements changed (0 <= changed < 1);
    max_run: after this many consecutive skipped frames of a session the next one is kept whatever its count (an integer >= 1), or
    None: no limit."""
    __slots__ = ("pixel_tol", "changed", "max_run")

    def __init__(self, pixel_tol=0.0, changed=0.0, max_run=None):
        for name, v in (("pixel_tol", pixel_tol), ("changed", changed)):
            if isinstance(v, bool) or not isinstance(v, (int, float)):
                raise TypeError("StillGate: %s must be a number, got %s" % (name, type(v).__name__))
        pixel_tol, changed = float(pixel_tol), float(changed)
        if not math.isfinite(pixel_tol) or pixel_tol < 0:
            raise ValueError("StillGate: pixel_tol must be finite and >= 0, got %r" % pixel_tol)
        if not 0.0 <= changed < 1.0:                 # a NaN fails this too
            raise ValueError("StillGate: changed must be in [0, 1), got %r" % changed)
        if max_run is not None and (isinstance(max_run, bool) or not isinstance(max_run, int)):
            raise TypeError("StillGate: max_run must be None or an integer, got %s" % type(max_run).__name__)
        if max_run is not None and max_run < 1:
            raise ValueError("StillGate: max_run must be None or an integer >= 1, got %r" % max_run)
        object.__setattr__(self, "pixel_tol", pixel_tol)
        object.__setattr__(self, "changed", changed)
        object.__setattr__(self, "max_run", max_run)

    def __setattr__(self, name, value):
        raise AttributeError("StillGate is immutable")

    def __repr__(self):
        return "StillGate(pixel_tol=%r, changed=%r, max_run=%r)" % (self.pixel_tol, self.changed, self.max_run)

    @property
    def tol(self):
        """pixel_tol rounded to fp32, once: what both the kernel and reference_changed compare against"""
        return float(torch.tensor(self.pixel_tol, dtype=torch.float32))

    def limit(self, L):
        """floor(changed * L): the largest change count of a still frame of L elements"""
        return int(math.floor(self.changed * L))


def reference_changed(frames, prev, rows, tol):
    """cfsk_changed in torch on the CPU.  frames [N, ...] and prev [max_streams, ...] fp32 (trailing dimensions are flattened to L);
    rows: the table, (slot, f0, n, last_pos) per session; tol: a float, rounded to fp32 here -> counts [N] int32: per frame the number
    of elements e with not (|x[e] - y[e]| <= tol) against its predecessor -- the frame before it in its row, prev[slot] for a row's
    first frame when last_pos >= 0 -- and -1 for a first frame when last_pos < 0 (prev[slot] is not read then)."""
    frames = torch.as_tensor(frames, dtype=torch.float32).cpu()
    frames = frames.reshape(frames.shape[0], -1)
    prev = torch.as_tensor(prev, dtype=torch.float32).cpu()
    prev = prev.reshape(prev.shape[0], -1)
    t = torch.tensor(tol, dtype=torch.float32)
    counts = torch.empty(frames.shape[0], dtype=torch.int32)
    for slot, f0, n, last_pos in rows:
        for i in range(f0, f0 + n):
            if i == f0 and last_pos < 0:
                counts[i] = -1
                continue
            y = prev[slot] if i == f0 else frames[i - 1]
            counts[i] = int((~((frames[i] - y).abs() <= t)).sum())
    return counts


def plan_still(counts, rows, runs, limit, max_run):
    """THE RULE (module docstring).  counts: the change count per frame of the push (-1: no predecessor); rows: the table, (slot, f0, n,
    last_pos) per session; runs: each session's run of skipped frames before the push, in the order of rows; limit: floor(changed * L);
    max_run: an integer >= 1 or None -> (kept, src, runs after the push).  kept: the indices of the frames that go through the tower,
    ascending; src[i]: the index, among kept, of the newest kept frame of frame i's session at or before i, or -1 when there is none in
    this push -- the frame then takes the row of the session's newest frame before the push."""
    kept, src, after = [], [-1] * len(counts), []
    for (slot, f0, n, last_pos), run in zip(rows, runs):
        at = -1
        for i in range(f0, f0 + n):
            c = int(counts[i])
            if c < 0 or c > limit or (max_run is not None and run >= max_run):
                at = len(kept)
                kept.append(i)
                run = 0
            else:
                run += 1
            src[i] = at
        after.append(run)
    return kept, src, after
