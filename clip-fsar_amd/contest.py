"""Contest: only a window's leading classes may fire events.

    p = StreamPool(live_gallery, events=EventRule(on=0.6, off=0.4), contest=Contest(top=1))                  # the best class of a window
    p = StreamPool(live_gallery, events=EventRule(on=0.6, off=0.4), contest=Contest(top=3, margin=0.05))     # the best three, and none
                                                                                                              # further than 0.05 below the best
    out = p.push_features({a: fa}); p.take_events()
    columns, counts = p.leaders(out[a])          # [nW, top] int32 (ascending columns, NONE-padded), [nW] int32: what the detector saw

The event detector judges every (session, class) pair on its own.  The contest is one stage between "judged" and "detector" that makes a
window's classes compete: it ranks the row -- one window of one session, its NC judged scores s_j with the store-slot keys key_j of its
columns -- and demotes the losers to -inf, which no threshold clears.  The rule of one row:

  candidate   0 <= key_j < cap, s_j is not NaN and s_j > -inf
  order       a larger float ranks higher, -0.0 and +0.0 are equal (score_key of ext/select_keys.h)
  leaders     the R = min(top, number of candidates) highest candidates; among candidates equal to the R-th score the lowest columns
              are taken first (compact_selected's tie rule)
  margin      (when not None) best = the highest candidate score, floor = best - margin, ONE rounded fp32 subtraction; a leader with
              s_j < floor stops being one
  output      the input's bits in the input's layout, except that a candidate that is not a leader becomes -inf.  NaN stays NaN (a NaN
              never disappears), -inf stays -inf, a column whose key is outside [0, cap) is copied unchanged: the detector never looks
              at it
  leaders     [rows, top] int32, the leaders' columns in ascending order, padded with NONE = 0x7fffffff; n_leaders [rows] int32

Under the detector's machine (clip_fsar_amd.events.reference_events) a demoted idle pair loses its streak (-inf < on) and a demoted
active pair counts a window below off, so an event ends when its class has been out of the leaders for min_off consecutive windows.  Such
an OFFSET's `score` is -inf: that is how a caller tells "outranked" from "faded".

The stage keeps no state and works per window, so its result does not depend on how frames are cut into pushes.  This module is the host
half and is pure: the rule's type and reference_contest, the rule restated with fp32 arithmetic, which the kernel of
libclipfsar_contest.so is compared against bit for bit.
"""
from __future__ import annotations

import collections
import math
import struct

import numpy as np

from .events import _fp32

NONE = 0x7FFFFFFF                        # the padding of a leader list (CFCT_NONE)
INT32_MAX = (1 << 31) - 1


class Contest(collections.namedtuple("Contest", "top margin")):
    """top: how many of a window's classes may lead, an integer in [1, 2^31); margin: None, or a finite number >= 0 (as fp32): how far
    below the window's best score a leader may lie"""
    __slots__ = ()

    def __new__(cls, top=1, margin=None):
        if isinstance(top, bool) or not isinstance(top, int) or not 1 <= top <= INT32_MAX:
            raise ValueError("Contest: top must be an integer in [1, 2^31), got %r" % (top,))
        if margin is not None:
            if isinstance(margin, bool) or not isinstance(margin, (int, float)) or not math.isfinite(_fp32(margin)) or _fp32(margin) < 0:
                raise ValueError("Contest: margin must be None or a finite number >= 0 (as fp32), got %r" % (margin,))
            margin = _fp32(margin)
        return super().__new__(cls, top, margin)


def score_keys(scores, valid=None):
    """score_key of ext/select_keys.h over an fp32 array: uint32 keys that order as the floats do, both zeros folded into +0.0, and
    0 = no candidate (NaN, -inf, or not `valid`)"""
    s = np.ascontiguousarray(scores, dtype=np.float32)
    u = np.where(s == 0, np.float32(0), s).view(np.uint32)
    key = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    with np.errstate(invalid="ignore"):
        cand = s > -np.inf                       # False for NaN and for -inf
    if valid is not None:
        cand = cand & np.asarray(valid, dtype=bool)
    return np.where(cand, key, np.uint32(0)).astype(np.uint32)


def reference_contest(scores, keys, cap, top, margin):
    """The rule over rows of one width.  scores: [rows, NC] fp32 values (numpy, a tensor on the host, or nested lists); keys: the NC
    store-slot keys of the columns, or [rows, NC] keys of their own per row, or None: every column competes (cap is then ignored);
    top, margin: Contest's -> (out [rows, NC] float32, leaders: per row the ascending list of its leaders' columns).  The padded
    [rows, top] form and n_leaders follow from the lists: leaders_table."""
    s = np.array(scores.numpy() if hasattr(scores, "numpy") else scores, dtype=np.float32)
    if s.ndim != 2:
        raise ValueError("reference_contest: scores must be [rows, NC], got shape %s" % (s.shape,))
    rows, NC = s.shape
    if keys is None:
        valid = np.ones((rows, NC), dtype=bool)
    else:
        k = np.array(keys.numpy() if hasattr(keys, "numpy") else keys, dtype=np.int64)
        valid = np.broadcast_to((k >= 0) & (k < int(cap)), (rows, NC))
    Contest(top, margin)                         # the refusals
    out, leaders = s.copy(), []
    for r in range(rows):
        key = score_keys(s[r], valid[r])
        cand = np.flatnonzero(key)
        R = min(int(top), cand.size)
        # descending by key, ascending by column among equal keys: a stable sort of the candidates' columns by the negated key
        order = cand[np.argsort(-key[cand].astype(np.int64), kind="stable")]
        lead = order[:R]
        if margin is not None and R:
            best = s[r, order[0]]
            with np.errstate(over="ignore", invalid="ignore"):
                floor = np.float32(best) - np.float32(margin)         # ONE rounded fp32 subtraction
            lead = np.array([j for j in lead if not s[r, j] < floor], dtype=np.int64)
        lost = np.setdiff1d(cand, lead)
        out[r, lost] = -np.inf
        leaders.append(sorted(int(j) for j in lead))
    return out, leaders


def leaders_table(leaders, top):
    """the leader lists of reference_contest -> ([rows, top] int32 padded with NONE, [rows] int32), as the kernel writes them"""
    table = np.full((len(leaders), int(top)), NONE, dtype=np.int32)
    for r, lead in enumerate(leaders):
        table[r, :len(lead)] = lead
    return table, np.array([len(lead) for lead in leaders], dtype=np.int32)
