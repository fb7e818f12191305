"""Adaptive baselines: a running mean and mean absolute deviation per (session, class) of a stream pool, and the deviation of every score
from them, maintained on the device while streams run.

    base = Baseline(rate=1 / 32, warm_rate=0.25, warmup=16, gate=3.0, floor=1e-6)
    p = StreamPool(live_gallery, baseline=base, events=EventRule(on=4, off=2, min_on=2, min_off=2))
    out = p.push_features({a: fa})                                # out[a].deviation [nW, C]: z per window and class, NaN through warm-up
    p.take_events()                                               # the rule judged z: on / off are in units of the pair's own deviation
    p.baseline(a)                                                 # [(class_id, mean, dev, n)] of the session's cells

The pool's scores share no scale -- OTAM logits around -8 or -40, COMBINE probabilities around 1 / (classes in the list), a class with
five shots above one enrolled from a single window -- so a fixed pair of thresholds on the raw score can only be chosen after the fact.
The usual answer for a detector over a drifting signal is a constant-false-alarm-rate threshold: every pair keeps a baseline of its own
scores, and the threshold is set on z = (s - mean) / dev.  A window that stands out (z >= gate) is not folded into the baseline, so an
event does not erase itself.

The recurrence of one pair over its scores s in window order, from the cell (m, d, n); a pair without a valid cell starts with n = 0:

  s not finite       z = NaN, the cell is untouched
  n == 0             m = s, d = 0, n = 1, z = NaN
  n < warmup         z = NaN; update with r = warm_rate; n += 1
  otherwise          z = (s - m) / max(d, floor); update with r = rate unless z >= gate; n stays at warmup
  update             keep = 1 - r;  a = |s - m| with the old m;  m = keep * m + r * s;  d = keep * d + r * a

Every operation is one correctly rounded fp32 operation, on the device (libclipfsar_baseline.so) and in reference_baseline, which
restates it in numpy float32 scalars: the two agree bit for bit.  A pair starts anew exactly where per-class smoothing and the event
detector start it: after the session's open() or reset(), after the class's registration and after the class joined the session's list.

This module is the host half and is pure.  The parameters compare as fp32, which is how the C ABI takes them.
"""
from __future__ import annotations

import collections
import math

from .events import _fp32

MAX_WARMUP = 1 << 20                     # CFBL_MAX_WARMUP

Cell = collections.namedtuple("Cell", "mean dev n")
START = Cell(0.0, 0.0, 0)                # how a cell without a valid mark starts


class Baseline(collections.namedtuple("Baseline", "rate warm_rate warmup gate floor")):
    """rate: the weight of a new window once the pair is warm, 0 < rate < 1; warm_rate: the same through warm-up, 0 < warm_rate <= 1;
    warmup: windows before the first deviation is reported, 1 .. 2^20; gate: a window with z >= gate is not folded in, > 0 (+inf: every
    window is); floor: the least deviation z is taken against, > 0 and finite"""
    __slots__ = ()

    def __new__(cls, rate=1 / 32, warm_rate=0.25, warmup=16, gate=3.0, floor=1e-6):
        for name, v in (("rate", rate), ("warm_rate", warm_rate), ("gate", gate), ("floor", floor)):
            if isinstance(v, bool) or not isinstance(v, (int, float)) or math.isnan(v):
                raise ValueError("Baseline: %s must be a number, got %r" % (name, v))
        if not 0.0 < _fp32(rate) < 1.0:
            raise ValueError("Baseline: rate must be in (0, 1) (as fp32), got %r" % (rate,))
        if not 0.0 < _fp32(warm_rate) <= 1.0:
            raise ValueError("Baseline: warm_rate must be in (0, 1] (as fp32), got %r" % (warm_rate,))
        if isinstance(warmup, bool) or not isinstance(warmup, int) or not 1 <= warmup <= MAX_WARMUP:
            raise ValueError("Baseline: warmup must be an integer in [1, 2^20], got %r" % (warmup,))
        if not _fp32(gate) > 0.0:
            raise ValueError("Baseline: gate must be above 0 (as fp32; inf: nothing is gated), got %r" % (gate,))
        if not 0.0 < _fp32(floor) < math.inf:
            raise ValueError("Baseline: floor must be above 0 and finite (as fp32), got %r" % (floor,))
        return super().__new__(cls, float(rate), float(warm_rate), warmup, float(gate), float(floor))


def reference_baseline(scores, rule, cell=None):
    """The recurrence of one (session, class) pair over its consecutive scores (floats holding fp32 values), from `cell` (a Cell, or None:
    n = 0) -> (z: a list of floats holding fp32 values, the Cell it leaves).  numpy float32 scalars: every operation is rounded to fp32
    once, as on the device.  Running it over a series in pieces, each from the cell the piece before left, gives the z of one run."""
    import numpy as np
    f = np.float32
    one, nan = f(1.0), float("nan")
    with np.errstate(all="ignore"):          # a gate beyond fp32's range is +inf
        rate, warm_rate, gate, floor = f(rule.rate), f(rule.warm_rate), f(rule.gate), f(rule.floor)
    m, d, n = START if cell is None else cell
    m, d, n = f(m), f(d), int(n)

    def fold(s, r):
        keep = one - r
        a = abs(s - m)
        return keep * m + r * s, keep * d + r * a

    z = []
    with np.errstate(all="ignore"):
        for s in scores:
            s = f(s)
            if not np.isfinite(s):
                z.append(nan)
            elif n == 0:
                m, d, n = s, f(0.0), 1
                z.append(nan)
            elif n < rule.warmup:
                m, d = fold(s, warm_rate)
                n += 1
                z.append(nan)
            else:
                zk = (s - m) / (floor if not d >= floor else d)          # fmaxf(d, floor): floor when d is below it, or NaN
                if not zk >= gate:
                    m, d = fold(s, rate)
                z.append(float(zk))
    return z, Cell(float(m), float(d), n)
