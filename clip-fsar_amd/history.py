"""History search: where else did a class happen, in the frames a pool still holds?

    p = StreamPool(live_gallery, stride=2, max_push=64, history=History(frames=4096))       # keyword-only; a LiveGallery
    a, b = p.open(), p.open(); p.push({a: fa, b: fb})        # pushes return what they return without the option, bit for bit
    p.searchable(a)                                          # range of a's window numbers whose T frames the history still holds
    r = p.search([7, "kite"], top=16)                        # sessions=None, min_score=None, separation=None, last=None, tempo=None
    r.hits[7]                                                # [Hit(session, class_id, window, score, tempo), ...], best first
    r.peaks[7], r.windows                                    # the peaks class 7 had before `top` cut them; the windows scanned
    r.scores, r.sessions, r.first_window, r.offsets          # the [NW, K] plane on the device, session-major
    p.hit_features(h); p.explain_hit(h); p.enroll_hit(h, "kite")     # while h.window is in p.searchable(h.session)

A session's ring holds cap = (T - 1) * rate + max_push frames, enough for the windows a push completes.  THE STORE of a pool with
history= holds [max_streams, F, E] fp32 tower rows, F = History.frames >= cap (a history shorter than the ring is the ring), and is
made by the first push.  Frame f of a session lives at [slot, f mod F]; every round of every push -- pixels, features, uint8, still=
-- writes the round's rows into it right beside the ring write, with the ring's own kernel (cfsp_ring_put, the store as its ring).
open() and reset() start a session at frame 0, so nothing of a slot's previous owner or of an earlier life is searchable, and only
open sessions are searched.  searchable(h) is pool.enrolable_windows(t, T, stride, rate, F): the complete windows whose first frame
the store still holds.

SEARCH.  classes: 1 to 64 registered ids, no repeats.  sessions: None -- every open session in handle order -- or a list, searched in
that order.  last=n: only windows completed by one of the session's newest n frames.  tempo (a pool with rates=): the index into rates
at which every window is read, as explain(tempo=) reads it; None: the last.  The windows are gathered out of the store
(cfsp_window_sequences) and scored by gallery.classify_features(X, classes=ids), a chunk of engine.max_frames // T windows at a time,
into the PLANE scores [NW, K]: session-major in the search's order, windows ascending, session i owning the plane rows
offsets[i] .. offsets[i + 1] - 1, its first one window first_window[i].  Then, on the device (libclipfsar_history.so), per class k:

  candidate   a score that is neither NaN nor -inf and, with min_score, score >= min_score as fp32
  beats       v beats j with a higher score, or with an equal score (==, so -0.0 == +0.0) and v < j
  peak        candidate j of session row r is a peak when no candidate v of the same row and class with 0 < |v - j| <= separation
              beats it.  Rows never see each other's windows.  This is a LOCAL-MAXIMUM FILTER, not greedy suppression: a window is
              judged against its neighbours' scores whether or not those neighbours are peaks themselves, so a rising run of
              windows suppresses all but its top even where greedy suppression would have kept a second one further down, and a
              plateau of equal scores yields its first window only
  separation  default ((T - 1) * rate) // stride, the largest distance at which two windows can share a frame; >= 0.  The device
              is given min(separation, longest row - 1), at most MAX_SEPARATION
  hits        per class the `top` highest peaks over all rows, 1 <= top <= MAX_TOP; a tie at the last place goes to the lower plane
              row -- an earlier session in the search's order, then a lower window.  The device returns them in ascending plane-row
              order; the host sorts them by descending score, then plane row.  A Hit's score carries the plane's bits.

search synchronises once, when it reads the hit records; with no searchable window it launches nothing and returns empty lists.
This module is the host half and is pure: the option's type, the plan of a search and reference_search, the rule restated on the CPU,
which the kernels are compared against bit for bit.
"""
from __future__ import annotations

import collections

import numpy as np

from .contest import score_keys
from .stream import window_plan

NONE = 0x7FFFFFFF                        # an unused place of hit_rows (CFHS_NONE)
MAX_CLASSES = 64                         # CFHS_MAX_CLASSES
MAX_TOP = 4096                           # CFHS_MAX_TOP
MAX_SEPARATION = 4096                    # CFHS_MAX_SEPARATION
MAX_ITEMS = 0x7FFFFFFF                   # the pool library indexes the rows and row pieces of a ring with 32 bits (csrc/ring_rows.h)


class History(collections.namedtuple("History", "frames")):
    """frames: the tower rows the store keeps per session, an integer >= 1 -- and, in a pool, at least the ring's cap and at most
    largest_frames(max_streams, E)"""
    __slots__ = ()

    def __new__(cls, frames):
        if isinstance(frames, bool) or not isinstance(frames, int) or frames < 1:
            raise ValueError("History: frames must be an integer >= 1, got %r" % (frames,))
        return super().__new__(cls, frames)


def largest_frames(max_streams, E):
    """the largest History.frames a pool of max_streams slots and rows of E floats can hold: the pool library's kernels index the
    store's max_streams * frames rows, 4-byte piece by piece at worst, with 32 bits"""
    return MAX_ITEMS // (int(max_streams) * int(E))


Hit = collections.namedtuple("Hit", "session class_id window score tempo")
# hits, peaks: {class id: ...} in the order of the search's classes; sessions, first_window, offsets: of the plane's session rows
SearchResult = collections.namedtuple("SearchResult", "hits peaks windows scores sessions first_window offsets")
# rows: the pool's 8-column table, a row per session; first_window, n_windows per session; offsets: their running sum, one longer
SearchPlan = collections.namedtuple("SearchPlan", "rows first_window n_windows offsets")


def held_windows(t, T, stride, rate, frames, last=None):
    """The windows of a session with t frames that a search scans, as a range: pool.enrolable_windows(t, T, stride, rate, frames) --
    complete, and the first frame still in the store -- and, with last=n, completed by one of the newest n frames: window w is
    completed by frame w * stride + (T - 1) * rate, which must be at least t - n."""
    from .pool import enrolable_windows          # the one statement of what a ring -- here the store -- of `frames` rows still holds
    ws = enrolable_windows(t, T, stride, rate, frames)
    if last is None or not len(ws):
        return ws
    lo = max(ws.start, -(-max(0, t - last - (T - 1) * rate) // stride))
    return range(lo, ws.stop) if lo < ws.stop else range(0)


def plan_search(sessions, T, stride, rate, frames, last=None, shift=0):
    """The host plan of a search.  sessions: (store slot, frames pushed so far) per session, in the search's order -> SearchPlan.  A
    table row follows the pool's layout (pool_hip): SLOT, PUT_POS = t mod frames, N = 0, FEAT_OFF = 0, WIN_POS = (lo * stride + shift)
    mod frames with lo the session's first held window, NW, WIN_OFF the running sum of NW, HAS_STATE = 0.  shift: how far the first
    frame of a window read at another tempo lies behind the first frame of the window as it is numbered (0 without rates=).  A
    session without a held window has NW = 0 and first_window = the number its next window will have."""
    rows, first_window, n_windows, offsets = [], [], [], [0]
    for slot, t in sessions:
        ws = held_windows(t, T, stride, rate, frames, last)
        lo = ws.start if len(ws) else window_plan(0, t, T, stride, rate)[1]
        rows.append([int(slot), t % frames, 0, 0, (lo * stride + shift) % frames, len(ws), offsets[-1], 0])
        first_window.append(lo)
        n_windows.append(len(ws))
        offsets.append(offsets[-1] + len(ws))
    return SearchPlan(rows, first_window, n_windows, offsets)


def check_top(top, what="History"):
    if isinstance(top, bool) or not isinstance(top, int) or not 1 <= top <= MAX_TOP:
        raise ValueError("%s: top must be an integer in [1, %d], got %r" % (what, MAX_TOP, top))
    return top


def check_separation(separation, what="History"):
    if isinstance(separation, bool) or not isinstance(separation, int) or separation < 0:
        raise ValueError("%s: separation must be an integer >= 0, got %r" % (what, separation))
    return separation


def check_min_score(min_score, what="History"):
    """-> None, or min_score as an fp32 value (a Python float); NaN is refused: no score is at least NaN"""
    if min_score is None:
        return None
    if isinstance(min_score, bool) or not isinstance(min_score, (int, float)) or min_score != min_score:
        raise ValueError("%s: min_score must be None or a number that is not NaN, got %r" % (what, min_score))
    with np.errstate(over="ignore"):
        return float(np.float32(min_score))


def device_separation(separation, n_windows, what="History"):
    """what the device is given for `separation` over rows of n_windows windows each: min(separation, longest row - 1) -- a larger
    distance reaches no further -- which must not exceed MAX_SEPARATION"""
    sep = max(0, min(separation, max(list(n_windows) + [0]) - 1))
    if sep > MAX_SEPARATION:
        raise ValueError("%s: separation = %d over a longest row of %d windows -- the search stages at most %d windows of halo; "
                         "give a smaller separation, or last= to shorten the rows" % (what, separation, max(n_windows), MAX_SEPARATION))
    return sep


def reference_search(scores, n_windows_per_row, separation, min_score, top):
    """The rule on the CPU.  scores: the plane [NW, K] fp32 (numpy, a host tensor or nested lists); n_windows_per_row: the windows of
    each session row, which tile the plane's rows in order; separation >= 0 (any size); min_score: None or a number that is not NaN;
    top >= 1 -> (hits, peaks): per class the kept plane rows in the device's order, ascending, and the class's number of peaks."""
    s = np.array(scores.numpy() if hasattr(scores, "numpy") else scores, dtype=np.float32)
    if s.ndim != 2 or s.shape[1] < 1:
        raise ValueError("reference_search: scores must be [NW, K] with K >= 1, got shape %s" % (s.shape,))
    counts = [int(n) for n in n_windows_per_row]
    if any(n < 0 for n in counts) or sum(counts) != s.shape[0]:
        raise ValueError("reference_search: the rows hold %r windows, the plane has %d" % (counts, s.shape[0]))
    check_separation(separation, "reference_search")
    if isinstance(top, bool) or not isinstance(top, int) or top < 1:
        raise ValueError("reference_search: top must be an integer >= 1, got %r" % (top,))
    floor = check_min_score(min_score, "reference_search")
    valid = None
    if floor is not None:
        with np.errstate(invalid="ignore"):
            valid = s >= np.float32(floor)
    key = score_keys(s, valid).astype(np.int64)          # 0: no candidate; equal scores (both zeros too) have equal keys
    peak, at = np.zeros(key.shape, dtype=bool), 0
    for n in counts:                                     # a session row at a time, every class and window of it at once
        blk = key[at:at + n]
        beaten = np.zeros(blk.shape, dtype=bool)
        for d in range(1, min(separation, n - 1) + 1):
            beaten[d:] |= blk[:-d] >= blk[d:]            # the neighbour d windows earlier beats it with an equal score too
            beaten[:-d] |= blk[d:] > blk[:-d]            # the one d windows later only with a higher one
        peak[at:at + n] = (blk != 0) & ~beaten           # (a key of 0, no candidate, beats nobody: every candidate's key is above it)
        at += n
    hits, peaks = [], []
    for k in range(s.shape[1]):
        found = np.flatnonzero(peak[:, k]).tolist()
        peaks.append(len(found))
        best = sorted(found, key=lambda row: (-key[row, k], row))[:top]      # a tie at the last place: the lower plane row
        hits.append(sorted(best))
    return hits, peaks
