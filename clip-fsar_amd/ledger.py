"""Shot ledger: remove, move, cap and audit the single shots of a live gallery's classes.

    g = LiveGallery(head, "cuda", capacity=64, ledger=ShotLedger(shots=4096, per_class=None, features=False))       # keyword-only
    g.add_classes(v, ids); g.add_shots(w, ids2); pool.enroll(a, 7)   # every existing call: the same arguments, returns and bits
    g.last_shots                                 # serials of the shots the most recent adding call made, in its video order
    g.shot_list(7)                               # [Shot(serial, class_id, origin)], oldest first
    g.remove_shots([s1, s2])                     # -> the touched classes' shot counts, first-appearance order
    g.move_shots([s3], "kite")                   # features=True: s3 leaves its class and joins "kite" as its newest shot -> new serials
    g.shot_features(s3)                          # features=True: the shot's [T, E] tower rows, a copy
    g.shot_fit(7)                                # [(serial, fit)]: leave-one-out agreement of each shot with the rest of its class
    g.shot_fits([7, 9])                          # {class id: [(serial, fit)]} of several classes (None: every ledgered one), one launch

A LiveGallery keeps one running fp32 sum per class and nothing of the single shots, so a shot, once added, stays.  With ledger= it also
keeps THE ADDEND STORE [shots, rows_kept, E] fp32 on the device, allocated once: per shot exactly the rows cfsl_accumulate summed for
it -- context2's first T output rows as computed in the call that added the shot, or with TRAIN.MERGE_BEFORE the T + 1 rows of the
support sequence itself.  Addends are summed sequentially in shot order, so the sum of the addends that remain, taken in the same order,
is well-defined bit for bit (cfld_resum of libclipfsar_ledger.so: cfsl_accumulate's bits on those addends).  The tower and context2 do
not run again for a removal; with MERGE_BEFORE context2 runs on the re-summed means, as it does after add_shots.  features=True adds a
second store [shots, T, E] of the raw tower rows, which move_shots needs: the target's text row enters context2, so a moved shot's
addend is computed again, by add_shots_features, and the shot gets a new serial.

A SERIAL is an int that rises with every shot ever added and is never reused.  An ORIGIN says which entry made the shot: "add_classes"
and "add_shots" for the pixel forms, "enroll" for everything that arrives as tower features (add_classes_features, add_shots_features,
StreamPool.enroll*, move_shots).  per_class=k: after an adding call every class over k shots has its oldest removed -- the result is
defined as "add, then remove_shots of the oldest".  A full store raises before anything changes; with per_class a class at its cap
first counts its own eviction.  Classes loaded from a state without a ledger are UNLEDGERED: they score and take shots as ever,
shot_list is empty, remove_shots and shot_fit raise on them.

FIT.  For shot x of a class with sum s, per row r < T: m = s[r] - x[r] (the sum of the others, one fp32 subtraction per element) and
cos_r = <x[r], m> / sqrt(<x[r], x[r]> * <m, m>); the fit is the mean of the T cosines.  A class of one shot has nothing to compare with:
NaN.  The audit reports, the caller decides.

This module is the host half and is pure: the option's type, the book of slots, serials and per-class lists with its planners (they
raise, or return what a call leaves behind; nothing is changed before the device work is queued), and reference_fit, the rule restated
in float64.
"""
from __future__ import annotations

import collections
import heapq

import numpy as np

ORIGINS = ("add_classes", "add_shots", "enroll")


class ShotLedger(collections.namedtuple("ShotLedger", "shots per_class features")):
    """shots: the addends the store holds, an integer >= 1; per_class: None or the most shots a class keeps, an integer >= 1;
    features: keep the raw tower rows too (move_shots, shot_features)"""
    __slots__ = ()

    def __new__(cls, shots=4096, per_class=None, features=False):
        if isinstance(shots, bool) or not isinstance(shots, int) or shots < 1:
            raise ValueError("ShotLedger: shots must be an integer >= 1, got %r" % (shots,))
        if per_class is not None and (isinstance(per_class, bool) or not isinstance(per_class, int) or per_class < 1):
            raise ValueError("ShotLedger: per_class must be None or an integer >= 1, got %r" % (per_class,))
        if not isinstance(features, bool):
            raise ValueError("ShotLedger: features must be True or False, got %r" % (features,))
        return super().__new__(cls, shots, per_class, features)


Shot = collections.namedtuple("Shot", "serial class_id origin")

# LedgerBook: what the host knows about the addend store.  cap slots; free: a heap of the free ones (the lowest is taken first);
# next_serial; slot_of / class_of / origin_of: per live serial; lists: per ledgered class its serials, oldest first; unledgered: the
# registered classes the ledger knows nothing of.  The plan_* functions change nothing.
LedgerBook = collections.namedtuple("LedgerBook", "cap free next_serial slot_of class_of origin_of lists unledgered")
# PutPlan: serials and slots per shot of the call, class-grouped (a slot of -1: the shot is over per_class at once and never stored);
# evicted: {class: the serials per_class drops}, book: what the call leaves behind
PutPlan = collections.namedtuple("PutPlan", "book serials slots evicted")
DropPlan = collections.namedtuple("DropPlan", "book classes")              # classes: the touched ones, first-appearance order


def new_ledger_book(cap, next_serial=0):
    return LedgerBook(int(cap), list(range(int(cap))), int(next_serial), {}, {}, {}, {}, frozenset())


def room_needed(book, counts, per_class=None):
    """the store slots an adding call takes in the end: counts {class: further shots}; with per_class a class counts its own evictions"""
    need = 0
    for c, n in counts.items():
        if c in book.unledgered:
            continue
        have = len(book.lists.get(c, ()))
        need += (min(per_class, have + n) if per_class is not None else have + n) - have
    return need


def check_room(book, need, name="LiveGallery"):
    if need > len(book.free):
        raise ValueError("%s: the shot ledger is full -- the call needs %d more addends, %d of %d are free (remove shots or classes, or "
                         "build the gallery with a larger ShotLedger(shots=))" % (name, need, len(book.free), book.cap))


def plan_put(book, runs, origin, per_class=None, name="LiveGallery"):
    """runs: [(class, further shots)] of an adding call, class-grouped -> PutPlan.  Per class the newest per_class shots stay; what the
    oldest ones held is free before the call's slots are taken, the lowest free slot first, in the call's order."""
    if origin not in ORIGINS:
        raise ValueError("%s: a shot's origin is one of %r, got %r" % (name, ORIGINS, origin))
    check_room(book, room_needed(book, dict(runs), per_class), name)
    free, serial = list(book.free), book.next_serial
    slot_of, class_of, origin_of, lists = dict(book.slot_of), dict(book.class_of), dict(book.origin_of), dict(book.lists)
    serials, slots, evicted, kept_new = [], [], {}, []
    for c, n in runs:
        mine = list(range(serial, serial + n))
        serial += n
        serials += mine
        if c in book.unledgered:
            kept_new.append(())
            continue
        every = list(lists.get(c, ())) + mine
        drop = every[:max(0, len(every) - per_class)] if per_class is not None else []
        if drop:
            evicted[c] = drop
        for s in drop:
            if s in slot_of:                                  # an older shot: its slot is free for this very call
                heapq.heappush(free, slot_of.pop(s))
                del class_of[s], origin_of[s]
        lists[c] = every[len(drop):]
        kept_new.append(set(mine) - set(drop))
    for (c, n), kept, first in zip(runs, kept_new, _firsts(runs, book.next_serial)):
        for s in range(first, first + n):
            if s in kept:
                slot_of[s], class_of[s], origin_of[s] = heapq.heappop(free), c, origin
                slots.append(slot_of[s])
            else:
                slots.append(-1)
    return PutPlan(book._replace(free=free, next_serial=serial, slot_of=slot_of, class_of=class_of, origin_of=origin_of, lists=lists),
                   serials, slots, evicted)


def _firsts(runs, first):
    for _, n in runs:
        yield first
        first += n


def plan_drop(book, serials, name="LiveGallery"):
    """serials: live shots, each once, none of them its class's last -> DropPlan: their slots free, their classes' lists without them"""
    serials = list(serials)
    if not serials:
        raise ValueError("%s: remove_shots needs at least one serial" % name)
    for s in serials:
        if isinstance(s, bool) or not isinstance(s, int) or s not in book.slot_of:
            raise ValueError("%s: %r is not the serial of a ledgered shot (remove_shots; an unledgered class has none)" % (name, s))
    if len(set(serials)) != len(serials):
        raise ValueError("%s: a serial appears twice in remove_shots: %r" % (name, serials))
    classes = list(dict.fromkeys(book.class_of[s] for s in serials))
    gone = set(serials)
    lists = dict(book.lists)
    for c in classes:
        lists[c] = [s for s in lists[c] if s not in gone]
        if not lists[c]:
            raise ValueError("%s: remove_shots would take the last shot of class %r -- use remove_classes" % (name, c))
    free = list(book.free)
    for s in serials:
        heapq.heappush(free, book.slot_of[s])
    keep = lambda d: {s: v for s, v in d.items() if s not in gone}
    return DropPlan(book._replace(free=free, slot_of=keep(book.slot_of), class_of=keep(book.class_of), origin_of=keep(book.origin_of),
                                  lists=lists), classes)


def drop_classes(book, ids):
    """the book after remove_classes(ids): their shots' slots free, nothing of them left"""
    ids = set(ids)
    gone = {s for c in ids for s in book.lists.get(c, ())}
    free = list(book.free)
    for s in gone:
        heapq.heappush(free, book.slot_of[s])
    keep = lambda d: {s: v for s, v in d.items() if s not in gone}
    return book._replace(free=free, slot_of=keep(book.slot_of), class_of=keep(book.class_of), origin_of=keep(book.origin_of),
                         lists={c: l for c, l in book.lists.items() if c not in ids}, unledgered=book.unledgered - ids)


def resum_rows(book, classes, class_slot):
    """the descriptor table of cfld_resum / cfld_fit for ledgered `classes` and the shared list of ledger slots: ([(class slot, first,
    n)], [ledger slot, ...])"""
    rows, slots = [], []
    for c in classes:
        mine = [book.slot_of[s] for s in book.lists[c]]
        rows.append((class_slot[c], len(slots), len(mine)))
        slots += mine
    return rows, slots


def ledgered(book, cid, what, name="LiveGallery"):
    """the serials of a ledgered class; raises on an unledgered one"""
    if cid in book.unledgered or cid not in book.lists:
        raise ValueError("%s: class %r is unledgered -- it was loaded from a state without a ledger, so nothing is known of its single "
                         "shots (%s); remove it and add it again" % (name, cid, what))
    return book.lists[cid]


def reference_fit(addends, T=None):
    """addends [N, rows, E]: the shots of one class, oldest first -> [N] float64: per shot the mean over rows r < T (default: all) of
    the cosine between the shot's row and the sum of the other shots' rows, in float64; NaN for N = 1 and wherever a norm is 0"""
    x = np.asarray(addends, dtype=np.float64)
    if x.ndim != 3 or x.shape[0] < 1:
        raise ValueError("reference_fit: addends must be [N >= 1, rows, E], got %s" % (x.shape,))
    T = x.shape[1] if T is None else int(T)
    if not 1 <= T <= x.shape[1]:
        raise ValueError("reference_fit: T = %d outside 1 .. %d rows" % (T, x.shape[1]))
    x = x[:, :T]
    if x.shape[0] == 1:
        return np.full(1, np.nan)
    m = np.stack([np.delete(x, i, axis=0).sum(axis=0) for i in range(x.shape[0])])      # the others' sum itself: no cancellation
    with np.errstate(invalid="ignore", divide="ignore"):
        cos = (x * m).sum(-1) / np.sqrt((x * x).sum(-1) * (m * m).sum(-1))
    return cos.mean(axis=1)
