"""Live gallery: a SupportGallery whose classes also leave, receive further shots, and are scored in subsets.

SupportGallery keeps a dense P [C, T, E], so the column order is the memory order: every add_classes copies the whole gallery, a class
cannot leave, and a caller who wants some of the classes pays for all.  Here the prototypes live in a STORE of slots and a column is a slot
number (libclipfsar_live.so, clip_fsar_amd.live_hip): removal edits an int list, a subset is another list, further shots update one slot
in place, and between growths (1.5 x when full) the store's address does not move.

    g = LiveGallery(head, device, capacity=64)
    g.add_classes(videos, class_of_video)        # SupportGallery's arguments, errors, return value -- and its prototypes, bit for bit
    g.add_shots(videos, class_of_video)          # further examples of registered classes -> their shot counts
    g.add_classes_features(feats, class_of_video); g.add_shots_features(feats, class_of_video)      # the same from tower features
                                                 # [Nv, T, E]: the tower does not run (StreamPool.enroll feeds its ring's rows this way)
    g.remove_classes([3, 7])                     # the other columns close up in their order; layout_version rises
    logits = g.classify(queries, classes=[9, 2]) # [NQ, 2], columns in the order given; None: every class, in registration order
    values, index = g.topk(queries, k=5, classes=None)
    r = g.classify_grouped(queries, counts=[3, 2], classes=[[9, 2], None])      # 3 clips against [9, 2], the next 2 against every class:
    r.group(0), r.group(1), r.logits             # [3, 2] and [2, C] views of the flat logits; one scoring launch (libclipfsar_groups.so)
    g.shots(9); g.state_dict()                   # SupportGallery's keys (dense, column order) + "sums" and "counts"
    g.slot_of(9); g.slot_generations()           # a class's store slot, and every slot's generation ([capacity] int32 on the device): it rises
                                                 # when a slot is freed or changes owner, so state kept per slot elsewhere (StreamPool's
                                                 # per-class smoothing) knows whether it still belongs to the slot's class
    g.slot_revision(slot)                        # host only: rises whenever the slot's prototype rows are written, further shots included, so what
                                                 # is derived from a prototype (clip_fsar_amd.shortlist.Shortlist's coarse rows) knows when to follow

    g = LiveGallery(head, device, ledger=ShotLedger(shots=4096))       # keyword-only (clip_fsar_amd.ledger): every shot's addend is kept too,
    g.last_shots; g.shot_list(9); g.remove_shots([s]); g.move_shots([s], 2); g.shot_fit(9)    # so single shots leave, move and are audited

A class is the mean of its shots, so the store also keeps every class's running SUM (of context2's outputs; with MERGE_BEFORE of the
support sequences before context2) and its shot count: further shots continue the sum in cfsg_segment_mean's operation order
(cfsl_accumulate).  Serves the default eval branch, like SupportGallery, and is accepted wherever one is (WindowStream, StreamPool); the
other two branches, EVAL_TEXT and COMBINE, over the same store are clip_fsar_amd.live_text_gallery.LiveTextGallery.
"""
from __future__ import annotations

import collections
import heapq

import torch

from . import gallery_hip as ghip
from . import groups_hip as grhip
from . import ledger as ldg
from . import ledger_hip as ldhip
from . import live_hip as lhip
from .gallery import LAMBDA, _flag, _GalleryBase

TABLE_ROWS = 1024                  # classes per descriptor table: larger updates go in pieces

# ---------------------------------------------------------------------------------------------------------------- bookkeeping (pure)
# Book: what the host knows about the store.  cap slots; free: a heap of the free ones (the lowest is taken first); order: the class ids
# in column order; slot_of / shots: per registered id (shots 0: loaded without a sum, takes no further shots); version: rises with every
# removal.  The plan_* functions below change nothing: they raise, or return the Book a call leaves behind together with what the device
# work needs, and the caller installs the new Book once that work is queued.
Book = collections.namedtuple("Book", "cap free order slot_of shots version")
AddPlan = collections.namedtuple("AddPlan", "book slots")                 # slots: of the new classes, in their order
RemovePlan = collections.namedtuple("RemovePlan", "book slots")           # slots: freed
ShotPlan = collections.namedtuple("ShotPlan", "book classes rows")        # classes: first-appearance order; rows: (slot, off, n, prior)


def new_book(cap):
    return Book(int(cap), list(range(int(cap))), [], {}, {}, 0)


def grown(cap, need):
    """the capacity after growing 1.5 x until `need` more slots than cap holds fit"""
    want = cap + need
    while cap < want:
        cap = max(cap + 1, cap * 3 // 2)
    return cap


def plan_add(book, ids, counts=None, name="LiveGallery"):
    """ids: new classes, in order (counts: their shots, default 1 each) -> AddPlan.  The lowest free slots go to the classes in order;
    a full store grows 1.5 x, its new slots free."""
    ids = list(ids)
    dup = [c for c in ids if c in book.slot_of]
    if dup:
        raise ValueError("%s: class %r is already registered" % (name, dup[0]))
    if len(set(ids)) != len(ids):
        raise ValueError("%s: a class appears twice among the new classes: %r" % (name, ids))
    counts = [1] * len(ids) if counts is None else [int(c) for c in counts]
    if len(counts) != len(ids) or any(c < 1 for c in counts):
        raise ValueError("%s: every new class needs a shot count >= 1, got %r" % (name, counts))
    cap, free = book.cap, list(book.free)
    if len(ids) > len(free):
        cap = grown(book.cap, len(ids) - len(free))
        for s in range(book.cap, cap):
            heapq.heappush(free, s)
    slots = [heapq.heappop(free) for _ in ids]
    slot_of, shots = dict(book.slot_of), dict(book.shots)
    for c, s, k in zip(ids, slots, counts):
        slot_of[c], shots[c] = s, k
    return AddPlan(Book(cap, free, book.order + ids, slot_of, shots, book.version), slots)


def _registered(book, ids, name, what):
    ids = list(ids)
    for c in ids:
        if c not in book.slot_of:
            raise ValueError("%s: class %r is not registered (%s)" % (name, c, what))
    return ids


def plan_remove(book, ids, name="LiveGallery"):
    """ids: registered classes, each once -> RemovePlan.  Their slots become free, the other columns keep their order, version + 1."""
    ids = _registered(book, ids, name, "remove_classes")
    if len(set(ids)) != len(ids):
        raise ValueError("%s: a class appears twice in remove_classes: %r" % (name, ids))
    gone = set(ids)
    free = list(book.free)
    for c in ids:
        heapq.heappush(free, book.slot_of[c])
    slot_of = {c: s for c, s in book.slot_of.items() if c not in gone}
    shots = {c: k for c, k in book.shots.items() if c not in gone}
    return RemovePlan(Book(book.cap, free, [c for c in book.order if c not in gone], slot_of, shots, book.version + 1),
                      [book.slot_of[c] for c in ids])


def plan_shots(book, ids_of_video, name="LiveGallery"):
    """ids_of_video: the class of every further video -> ShotPlan: per class in first-appearance order a row (slot, offset of its run among
    the class-grouped videos, videos in the run, shots before)"""
    ids_of_video = _registered(book, ids_of_video, name, "add_shots takes further videos of registered classes")
    classes = list(dict.fromkeys(ids_of_video))
    if not classes:
        raise ValueError("%s: add_shots needs at least one video" % name)
    for c in classes:
        if book.shots[c] < 1:
            raise ValueError("%s: class %r was loaded without its sum (a SupportGallery state): it takes no further shots -- remove it and "
                             "add it again" % (name, c))
    shots, rows, off = dict(book.shots), [], 0
    for c in classes:
        n = sum(1 for v in ids_of_video if v == c)
        rows.append((book.slot_of[c], off, n, book.shots[c]))
        shots[c] += n
        off += n
    return ShotPlan(book._replace(shots=shots), classes, rows)


def plan_columns(book, classes=None, name="LiveGallery"):
    """the slots of the columns of a classify call: every class in column order, or `classes` in the order given (registered, no repeats)"""
    if classes is None:
        return [book.slot_of[c] for c in book.order]
    classes = _registered(book, classes, name, "classes=")
    if not classes:
        raise ValueError("%s: classes= needs at least one class" % name)
    if len(set(classes)) != len(classes):
        raise ValueError("%s: a class appears twice in classes=: %r" % (name, classes))
    return [book.slot_of[c] for c in classes]


GroupPlan = collections.namedtuple("GroupPlan", "rows slots n_out")      # rows: groups_hip's table; slots: the lists, one after the other


def plan_groups(book, counts, classes, T, name="LiveGallery"):
    """counts[i] consecutive queries against classes[i] (plan_columns' rules per group; None: every class in column order) -> GroupPlan:
    the descriptor table of the grouped kernels for frames of T, the concatenated slot lists and the number of logits"""
    counts, classes = list(counts), list(classes)
    if len(counts) != len(classes) or not counts:
        raise ValueError("%s: grouped scoring needs groups and one count for each, got %d counts and %d class lists" % (
            name, len(counts), len(classes)))
    if any(isinstance(n, bool) or not isinstance(n, int) or n < 0 for n in counts):
        raise ValueError("%s: a group's count must be an integer >= 0, got %r" % (name, counts))
    lists = [plan_columns(book, c, "%s: group %d" % (name, i)) for i, c in enumerate(classes)]
    for i, slots in enumerate(lists):
        if not slots:                                         # None on a gallery without classes
            raise ValueError("%s: group %d: classes= needs at least one class" % (name, i))
    rows, (_, _, _, n_out) = grhip.table_rows(counts, [len(l) for l in lists], T)
    return GroupPlan(rows, [s for l in lists for s in l], n_out)


def chunk_groups(rows, q0, q1, T):
    """The part of a table that the queries q0 .. q1-1 (q0 < q1) reach, as a table of its own: (rows, (first, end) of its lists in the slot
    list, the first logit it owns).  The groups from the first to the last one with a query in the range, those between without queries
    included: their lists and their logits are contiguous in the whole call's, so the chunk's launch works on slices."""
    hit = [g for g, r in enumerate(rows) if r[grhip.NQ] and r[grhip.Q0] < q1 and r[grhip.Q0] + r[grhip.NQ] > q0]
    part = rows[hit[0]:hit[-1] + 1]
    counts = [max(0, min(q1, r[grhip.Q0] + r[grhip.NQ]) - max(q0, r[grhip.Q0])) for r in part]
    first, last = part[0], part[-1]
    sub, _ = grhip.table_rows(counts, [r[grhip.NC] for r in part], T)
    return sub, (first[grhip.C0], last[grhip.C0] + last[grhip.NC]), first[grhip.OUT0] + (q0 - first[grhip.Q0]) * first[grhip.NC]


class GroupedLogits:
    """What grouped scoring returns: `logits`, flat, group i owning [offsets[i], offsets[i + 1]) as a row-major [counts[i], widths[i]]
    block -- group(i) is that view."""
    __slots__ = ("logits", "offsets", "widths", "counts")

    def __init__(self, logits, offsets, widths, counts):
        self.logits, self.offsets, self.widths, self.counts = logits, offsets, widths, counts

    def __len__(self):
        return len(self.counts)

    def group(self, i):
        return self.logits[self.offsets[i]:self.offsets[i + 1]].view(self.counts[i], self.widths[i])


# ---------------------------------------------------------------------------------------------------------------- the gallery
class LiveGallery(_GalleryBase):
    def __init__(self, head, device="cuda", capacity=64, *, ledger=None):
        head = getattr(head, "head", head)                 # BaseVideoModel -> its CNN_OTAM_CLIPFSAR head
        self._check_branch(head.args)
        if isinstance(capacity, bool) or not isinstance(capacity, int) or capacity < 1:
            raise ValueError("LiveGallery: capacity must be an integer >= 1, got %r" % (capacity,))
        if ledger is not None and not isinstance(ledger, ldg.ShotLedger):
            raise TypeError("LiveGallery: ledger must be a ShotLedger (clip_fsar_amd.ledger) or None, got %r" % (ledger,))
        self._setup(head, device)
        if self.T > lhip.MAX_T:
            raise ValueError("LiveGallery: T = %d frames, the live library scores at most %d" % (self.T, lhip.MAX_T))
        if ledger is not None and self.E % 4:
            raise ValueError("LiveGallery: ledger= needs E %% 4 == 0 (the ledger library moves 16-byte pieces), got E = %d" % self.E)
        self._ledger = ledger                              # the option; without it nothing below the next four lines exists
        self._lbook = None if ledger is None else ldg.new_ledger_book(ledger.shots)
        self._lstore = self._ltables = None                # the addend store (and the features'), allocated by the first adding call
        self._lpending = None                              # (the Book a plan returned, the ledger slots the call needs so far)
        self._levicted, self._last_shots, self._lcapped = {}, [], set()
        self._capacity = capacity
        self._store = None                                 # allocated by the first call that needs the device
        self._retired = []                                 # (outgrown store, the event behind the work queued on it)
        self._tables = self._group_tables = None
        self._book = self._active = None
        self._slot_gen, self._slot_gen_dev = [], None      # the store slots' generations (_install keeps them) and their device copy
        self._slot_rev = []                                # the store slots' revisions: host only (_install, _update_sequences)
        self._writes = 0                                   # how often _touch_slots raised a revision: unchanged means no slot was written
        self.clear()

    def _check_branch(self, cfg):
        """the eval branch the head's flags ask for is the one this gallery serves (LiveTextGallery serves the other two)"""
        for flag in ("EVAL_TEXT", "COMBINE"):
            if _flag(cfg.TRAIN, flag):
                raise NotImplementedError("LiveGallery: TRAIN.%s is not supported -- the gallery serves the default eval branch (cosine + "
                                          "OTAM of context2 features) only; use clip_fsar_amd.text_gallery.TextGallery for this branch" % flag)

    # ------------------------------------------------------------------ state
    def clear(self):
        """Drop every class (and bind to the head's current engine).  The store keeps its memory."""
        self._bind()
        version = 0 if self._book is None else self._book.version + bool(self._book.order)
        cap = self._store_cap() if self._store is not None else self._capacity
        self._install(new_book(cap)._replace(version=version), renew=True)
        if self._ledger is not None:                       # the ledger is empty; serials are never reused
            self._lbook = ldg.new_ledger_book(self._ledger.shots, self._lbook.next_serial)
            self._ledger_forget()

    def _install(self, book, renew=False):
        """the Book a call leaves behind.  The slots' generations follow it: a slot that was freed, or whose class is another one now, gets
        the next generation (renew: every slot does -- clear() and load_state_dict, after which no slot holds what it held); the slots a
        growth adds start at 1."""
        old = self._book
        gen = self._slot_gen
        if renew or old is None:
            changed = range(len(gen))
        else:
            owner = {s: c for c, s in book.slot_of.items()}
            changed = [s for c, s in old.slot_of.items() if s not in owner or owner[s] != c]
        for s in changed:
            gen[s] += 1
        gen.extend([1] * (book.cap - len(gen)))
        self._touch_slots(range(len(self._slot_rev)) if renew else (), book.cap)
        if changed or self._slot_gen_dev is None or self._slot_gen_dev.shape[0] != len(gen):
            self._slot_gen_dev = None                      # uploaded anew on demand: a launch in flight keeps the tensor it was given
        self._book = book
        self._ids = book.order                             # _GalleryBase: len(), class_ids, "no classes registered"
        self._cols = None                                  # device column list of all classes, made on demand
        self._subset = (None, None)                        # the last classes= list and its device columns
        self._group_cols = (None, None)                    # the last grouped call's slot lists and their device copy

    @property
    def layout_version(self):
        """rises whenever a column may have changed its meaning: on every remove_classes (and a clear() of a non-empty gallery)"""
        return self._book.version

    @property
    def capacity(self):
        return self._book.cap

    def slot_generation(self, slot):
        """the generation of a store slot: at least 1, and higher after every time the slot was freed or changed its owner"""
        return self._slot_gen[slot]

    def slot_generations(self):
        """[capacity] int32 on the device: every store slot's generation.  Whoever keeps state per store slot (StreamPool's per-class
        smoothing) stores the generation beside it, and the state is valid iff the two still agree."""
        if self._slot_gen_dev is None:
            self._slot_gen_dev = torch.tensor(self._slot_gen, device=self.dev, dtype=torch.int32)
        return self._slot_gen_dev

    def slot_revision(self, slot):
        """the revision of a store slot's prototype rows: it rises whenever they are written -- a registration, further shots (which leave
        the generation alone), an enrolment, and for every slot clear() and load_state_dict; a growth copies the rows and keeps it.  Host
        only.  Whoever keeps something derived from a slot's prototype (clip_fsar_amd.shortlist.Shortlist: its coarse rows) remembers the
        revision it was computed at."""
        return self._slot_rev[slot]

    def _touch_slots(self, slots, cap=0):
        """the revisions of `slots` rise; the list reaches at least cap slots (new ones start at 0)"""
        rev = self._slot_rev
        slots = list(slots)
        rev.extend([0] * (max([cap] + [s + 1 for s in slots]) - len(rev)))
        for s in slots:
            rev[s] += 1
        self._writes += bool(slots)

    def shots(self, cid):
        """the shot count of a class (0: loaded from a SupportGallery state, whose sums are not known)"""
        if cid not in self._book.shots:
            raise ValueError("LiveGallery: class %r is not registered (shots)" % (cid,))
        return self._book.shots[cid]

    def slot_of(self, cid):
        return self._book.slot_of[cid]

    # ------------------------------------------------------------------ the store
    def _rows(self):
        return self.T + 1                                  # rows of a support sequence, and of a slot of `sums`

    def _store_cap(self):
        return self._store["text"].shape[0]                # every store has a text row per slot

    def _alloc(self, cap):
        T, E, f = self.T, self.E, dict(device=self.dev, dtype=torch.float32)
        return {"P": torch.empty(cap, T, E, **f), "text": torch.empty(cap, E, **f), "sums": torch.empty(cap, self._rows(), E, **f),
                "pn": torch.empty(cap * T, **f)}                 # in the order growth copies them

    def _ensure_store(self, cap):
        """the store with at least cap slots.  Growth copies the old slots once; the outgrown buffers are kept until the work queued on
        them (a classify in flight) is done."""
        self._retired = [(b, e) for b, e in self._retired if not e.query()]
        old = self._store
        if old is not None and self._store_cap() >= cap:
            return old
        new = self._alloc(cap)
        if old is not None:
            for k, t in old.items():                          # whatever the store holds: slots (or their rows) lead every buffer
                new[k][:t.shape[0]].copy_(t)
            with torch.cuda.device(self.dev):
                ev = torch.cuda.Event()
                ev.record()
            self._retired.append((old, ev))
        self._store = new
        return new

    def _upload(self, rows):
        if self._tables is None:
            self._tables = lhip.table_uploader(self.dev, TABLE_ROWS)
        return self._tables.upload([list(r) for r in rows])

    def _update_sequences(self, eng, X0, offs, rows, shots=None):
        """Support sequences X0 [Nv, T+1, E], grouped by class (class i = sequences offs[i] .. offs[i+1]-1; rows: the classes' (slot, off,
        n, prior)) into the store: sums, prototypes, norms.  SupportGallery's launch sequence after the support sequences -- context2 class
        by class -- with cfsl_accumulate in the place of cfsg_segment_mean (prior = 0: its bits) and the norms of the touched slots alone.
        shots (a gallery with ledger=): (the classes' ids, the origin) -- every sequence's addend goes into the ledger beside the sum."""
        st, T, E, n = self._store, self.T, self.E, len(rows)
        self._touch_slots([r[0] for r in rows])
        plan, put = (None, None) if self._ledger is None else self._ledger_plan_put(shots[0], rows, shots[1])
        Y = None if self.merge_before else self._context2_by_class(eng, X0, offs)       # (:2955-2956)
        for c0 in range(0, n, TABLE_ROWS):
            c1 = min(n, c0 + TABLE_ROWS)
            v0, v1 = offs[c0], offs[c1]
            table = self._upload([(s, o - v0, k, p) for s, o, k, p in rows[c0:c1]])
            if self.merge_before:                             # class means BEFORE context2 (:2949-2954), the text row included
                seqs = torch.empty(c1 - c0, T + 1, E, device=self.dev, dtype=torch.float32)
                lhip.accumulate(X0[v0:v1], st["sums"], seqs, table, by_slot=False)
                self._prototypes_of_means(eng, seqs, [r[0] for r in rows[c0:c1]])
            else:                                             # prototype = class mean of context2's first T rows (:2957-2962)
                lhip.accumulate(Y[v0:v1], st["sums"], st["P"], table, by_slot=True)
            if put is not None:                               # exactly the rows the accumulate above summed, and the raw tower rows
                ldhip.put(X0[v0:v1] if self.merge_before else Y[v0:v1], self._lstore["addends"], put[v0:v1])
                if self._ledger.features:
                    ldhip.put(X0[v0:v1], self._lstore["features"], put[v0:v1])
            lhip.slot_norms(st["P"], st["pn"], table)
        if self._ledger is not None:                          # the launches are queued: the ledger's book follows, as the gallery's will
            self._ledger_install_put(plan)

    def _prototypes_of_means(self, eng, seqs, slots):
        """MERGE_BEFORE: the classes' mean sequences seqs [n, T+1, E] through context2, class by class, into the prototypes of `slots`"""
        n, T, E = len(slots), self.T, self.E
        Y1 = self._context2_by_class(eng, seqs, list(range(n + 1)))
        P = torch.empty(n, T, E, device=self.dev, dtype=torch.float32)
        ghip.segment_mean(Y1, torch.arange(n + 1, device=self.dev, dtype=torch.int32), P)     # a mean over one sequence
        self._store["P"].index_copy_(0, torch.tensor(slots, device=self.dev), P)

    # ------------------------------------------------------------------ registration, shots, removal
    # Each has a pixel form and a feature form, which differ in how the support sequences come about: `sequences(ids_of_video, classes,
    # trows) -> (X0, offs)` is _support_sequences behind the tower or _sequences_of_features without it.  What a call decides before the
    # device is touched (plan_classes, plan_shots) and what it does with ready sequences (_register_sequences, _shots_sequences) are
    # apart, so that StreamPool.enroll_windows, whose sequences come out of its ring, plans a whole call first and then uses the latter.
    def _plan_classes(self, eng, ids_of_video, new_ids, text, book=None):
        """-> (text rows of the new classes, their shot counts, AddPlan on `book`, default the gallery's); raises what add_classes raises
        about the classes"""
        trows = self._text_rows(eng, new_ids, text)
        counts = [sum(1 for v in ids_of_video if v == c) for c in new_ids]
        plan = plan_add(self._book if book is None else book, new_ids, counts, self._name)
        self._ledger_room(book, plan.book, dict(zip(new_ids, counts)))
        return trows, counts, plan

    def _register_sequences(self, eng, trows, counts, plan, sequences, origin="enroll"):
        """the device work of a registration planned by _plan_classes; sequences(trows) -> (X0, offs).  -> the new column indices.
        origin (a gallery with ledger=): what the shots' records say; the feature entries and StreamPool's enrolment leave the default"""
        st = self._ensure_store(plan.book.cap)
        offs = [0]
        for k in counts:
            offs.append(offs[-1] + k)
        X0, seq_offs = sequences(trows)
        assert seq_offs == offs
        self._update_sequences(eng, X0, offs, [(s, offs[i], counts[i], 0) for i, s in enumerate(plan.slots)],
                               (plan.book.order[len(plan.book.order) - len(plan.slots):], origin))
        self._write_text_rows(st, plan.slots, trows)
        C0 = len(self._book.order)
        self._install(plan.book)
        self._ledger_evict(eng)
        return list(range(C0, C0 + len(plan.slots)))

    def _write_text_rows(self, st, slots, trows):
        """the new classes' text rows into their slots (LiveTextGallery: and their norms)"""
        st["text"].index_copy_(0, torch.tensor(slots, device=self.dev), trows)

    def _shots_sequences(self, eng, plan, sequences, origin="enroll"):
        """the device work of further shots planned by plan_shots; sequences(trows) -> (X0, offs).  -> the classes' shot counts"""
        st = self._store
        trows = st["text"].index_select(0, torch.tensor([r[0] for r in plan.rows], device=self.dev))
        X0, offs = sequences(trows)
        self._update_sequences(eng, X0, offs, plan.rows, (plan.classes, origin))
        self._book = plan.book                              # the columns did not change: _ids and the device lists stay
        self._ledger_evict(eng)
        return [self._book.shots[c] for c in plan.classes]

    def _add_classes(self, eng, src, class_of_video, text, sequences_of, origin="enroll"):
        ids_of_video, new_ids = self._video_classes(src, class_of_video, text)
        trows, counts, plan = self._plan_classes(eng, ids_of_video, new_ids, text)
        cols = self._register_sequences(eng, trows, counts, plan, lambda trows: sequences_of(src, ids_of_video, new_ids, trows), origin)
        self._last_in_video_order(ids_of_video, new_ids)
        return cols

    def _shot_ids(self, class_of_video):
        ids = [c.item() if isinstance(c, torch.Tensor) else c for c in (
            class_of_video.reshape(-1).cpu() if isinstance(class_of_video, torch.Tensor) else class_of_video)]
        return [int(c) if isinstance(c, float) and c == int(c) else c for c in ids]

    def _plan_shots(self, ids, book=None):
        """plan_shots on `book`, default the gallery's (StreamPool.enroll_windows plans a whole call on a book of its own)"""
        plan = plan_shots(self._book if book is None else book, ids, self._name)
        self._ledger_room(book, plan.book, {c: r[2] for c, r in zip(plan.classes, plan.rows)})
        return plan

    def _add_shots(self, eng, src, class_of_video, sequences_of, origin="enroll"):
        ids = self._shot_ids(class_of_video)
        if len(ids) != src.shape[0]:
            raise ValueError("%s: %d videos but %d class ids" % (self._name, src.shape[0], len(ids)))
        plan = self._plan_shots(ids)
        counts = self._shots_sequences(eng, plan, lambda trows: sequences_of(src, ids, plan.classes, trows), origin)
        self._last_in_video_order(ids, plan.classes)
        return counts

    def add_classes(self, videos, class_of_video, text=None):
        """SupportGallery.add_classes: the same arguments, errors, return value (the new classes' column indices) and prototypes; nothing but
        the new classes is written."""
        eng = self._fresh_engine()
        videos = self._check_videos(videos, "videos")
        return self._add_classes(eng, videos, class_of_video, text, lambda *a: self._support_sequences(eng, *a), "add_classes")

    def add_classes_features(self, feats, class_of_video, text=None):
        """add_classes of clips whose tower features feats [Nv, T, E] fp32 (device) exist already (a cache, a stream pool's ring): the same
        arguments otherwise, errors, return value and prototypes, bit for bit; the tower does not run."""
        eng = self._fresh_engine()
        feats = self._check_feats(feats)
        return self._add_classes(eng, feats, class_of_video, text, self._sequences_of_features)

    def add_shots(self, videos, class_of_video):
        """Further videos [Nv, T, 3, H, W] of registered classes (class_of_video [Nv]) join their classes after the existing shots: the
        classes' sums go on, their prototypes and norms are recomputed in place.  Returns the classes' shot counts, in first-appearance
        order."""
        eng = self._fresh_engine()
        videos = self._check_videos(videos, "videos")
        return self._add_shots(eng, videos, class_of_video, lambda *a: self._support_sequences(eng, *a), "add_shots")

    def add_shots_features(self, feats, class_of_video):
        """add_shots of clips whose tower features feats [Nv, T, E] fp32 (device) exist already; the tower does not run."""
        eng = self._fresh_engine()
        feats = self._check_feats(feats)
        return self._add_shots(eng, feats, class_of_video, self._sequences_of_features)

    def remove_classes(self, ids):
        """Drop registered classes: their slots become free (the lowest free slot is the next one taken), the remaining columns close up
        in their order, no prototype moves.  layout_version rises.  Unknown ids raise before anything changes."""
        ids = [c.item() if isinstance(c, torch.Tensor) else c for c in (ids.reshape(-1).cpu() if isinstance(ids, torch.Tensor) else ids)]
        self._install(plan_remove(self._book, ids, self._name).book)
        if self._ledger is not None:                          # their ledger slots are free again
            self._lbook = ldg.drop_classes(self._lbook, ids)

    # ------------------------------------------------------------------ the shot ledger (ledger=ShotLedger(...); clip_fsar_amd.ledger)
    # The host half is ledger.LedgerBook and its planners.  An adding call checks the room when it is planned (_ledger_room: a call
    # that StreamPool.enroll_windows plans in two parts on a book of its own is counted as one), takes its slots and serials in
    # _update_sequences (_ledger_plan_put) and, with per_class, drops what is over the cap once its book is installed (_ledger_evict).
    def _need_ledger(self, what, features=False):
        if self._ledger is None:
            raise ValueError("%s.%s: this gallery keeps no shot ledger (build it with ledger=ShotLedger(...))" % (self._name, what))
        if features and not self._ledger.features:
            raise ValueError("%s.%s: this ledger keeps no tower rows (build it with ShotLedger(features=True))" % (self._name, what))

    def _ledger_room(self, base, planned, counts):
        """an adding call of `counts` {class: shots}, planned from the Book `base` (None: the gallery's) into `planned`, fits the store"""
        if self._ledger is None:
            return
        if base is None or base is self._book:                # a call starts: no Book from before an eviction is still to come
            self._lcapped = set()
        before = self._lpending[1] if self._lpending is not None and self._lpending[0] is base else 0
        need = before + ldg.room_needed(self._lbook, counts, self._ledger.per_class)
        ldg.check_room(self._lbook, need, self._name)
        self._lpending = (planned, need)

    def _ledger_forget(self):
        """nothing of an earlier adding call is pending, evicted or last"""
        self._lpending, self._levicted, self._last_shots, self._lcapped = None, {}, [], set()

    def _ledger_stores(self):
        if self._lstore is None:
            f = dict(device=self.dev, dtype=torch.float32)
            rows = self._rows() if self.merge_before else self.T          # the rows cfsl_accumulate sums for a shot
            self._lstore = {"addends": torch.empty(self._ledger.shots, rows, self.E, **f)}
            if self._ledger.features:
                self._lstore["features"] = torch.empty(self._ledger.shots, self.T, self.E, **f)
            self._ltables = ldhip.table_uploader(self.dev, TABLE_ROWS)
        return self._lstore

    def _ledger_plan_put(self, classes, rows, origin):
        """the serials and slots of the call's shots -> (the PutPlan, the slots [Nv] int32 on the device, class-grouped as the sequences
        are; None when no shot of the call is kept).  Nothing of the ledger changes before _ledger_install_put."""
        plan = ldg.plan_put(self._lbook, [(c, r[2]) for c, r in zip(classes, rows)], origin, self._ledger.per_class, self._name)
        if all(s < 0 for s in plan.slots):
            return plan, None
        self._ledger_stores()
        return plan, torch.tensor(plan.slots, device=self.dev, dtype=torch.int32)

    def _ledger_install_put(self, plan):
        """the ledger's book of an adding call whose device work is queued"""
        self._lbook, self._lpending = plan.book, None
        self._last_shots, self._levicted = plan.serials, plan.evicted

    def _ledger_evict(self, eng):
        """Behind the install of an adding call's Book.  per_class: the classes the call took over their cap are re-summed from the
        shots they keep.  And a ledgered class has as many shots as its list says: a Book that was planned before an earlier part of the
        same call evicted (StreamPool.enroll_windows plans its two gallery calls up front) still carries the count from before."""
        if self._ledger is None:
            return
        classes, self._levicted = list(self._levicted), {}
        self._lcapped.update(classes)
        lists, have = self._lbook.lists, self._book.shots
        wrong = {c: len(lists[c]) for c in self._lcapped if c in lists and c in have and have[c] != len(lists[c])}
        if wrong:
            shots = dict(have)
            shots.update(wrong)
            self._book = self._book._replace(shots=shots)
        if classes:
            self._resum_classes(eng, classes)

    def _last_in_video_order(self, ids_of_video, classes):
        """_last_shots, made class-grouped, in the order of the call's videos"""
        if self._ledger is None:
            return
        local = {c: i for i, c in enumerate(classes)}
        order = sorted(range(len(ids_of_video)), key=lambda v: (local[ids_of_video[v]], v))
        by_video = [None] * len(order)
        for at, v in enumerate(order):
            by_video[v] = self._last_shots[at]
        self._last_shots = by_video

    def _resum_classes(self, eng, classes):
        """sums, prototypes and norms of ledgered classes again from the addends their lists name, in that order: one cfld_resum launch
        per TABLE_ROWS classes, then the gallery's own path as after add_shots"""
        st, book, T, E = self._store, self._lbook, self.T, self.E
        lst = self._ledger_stores()
        self._touch_slots([self._book.slot_of[c] for c in classes])
        for c0 in range(0, len(classes), TABLE_ROWS):
            part = classes[c0:c0 + TABLE_ROWS]
            rows, slots = ldg.resum_rows(book, part, self._book.slot_of)
            table = self._ltables.upload([list(r) for r in rows])
            slot_list = torch.tensor(slots, device=self.dev, dtype=torch.int32)
            if self.merge_before:
                seqs = torch.empty(len(part), T + 1, E, device=self.dev, dtype=torch.float32)
                ldhip.resum(lst["addends"], slot_list, st["sums"], seqs, table, by_slot=False)
                self._prototypes_of_means(eng, seqs, [r[0] for r in rows])
            else:
                ldhip.resum(lst["addends"], slot_list, st["sums"], st["P"], table, by_slot=True)
            lhip.slot_norms(st["P"], st["pn"], self._upload([(r[0], 0, 1, 0) for r in rows]))

    @property
    def last_shots(self):
        """serials of the shots the most recent adding call made, in its video order (StreamPool.enroll_windows: in the order of its
        items, whichever of its two gallery calls made them).  A shot that per_class dropped at once has a serial too."""
        self._need_ledger("last_shots")
        return list(self._last_shots)

    def shot_list(self, cid):
        """[Shot(serial, class_id, origin)] of a registered class, oldest first; empty for an unledgered class"""
        self._need_ledger("shot_list")
        if cid not in self._book.slot_of:
            raise ValueError("%s: class %r is not registered (shot_list)" % (self._name, cid))
        return [ldg.Shot(s, cid, self._lbook.origin_of[s]) for s in self._lbook.lists.get(cid, ())]

    def _serials(self, serials):
        return [s.item() if isinstance(s, torch.Tensor) else s for s in (serials.reshape(-1).cpu() if isinstance(serials, torch.Tensor)
                                                                        else serials)]

    def remove_shots(self, serials):
        """The shots leave their classes: every touched class's sum is formed again from its remaining addends in their order, its
        prototype and norms follow; the tower does not run.  Returns the touched classes' shot counts, in first-appearance order.  The
        touched slots' revisions rise; generations, columns and layout_version stay.  An unknown or repeated serial, a class's last shot
        and a shot of an unledgered class raise before anything changes."""
        self._need_ledger("remove_shots")
        eng = self._fresh_engine()
        plan = ldg.plan_drop(self._lbook, self._serials(serials), self._name)
        shots = dict(self._book.shots)
        shots.update((c, len(plan.book.lists[c])) for c in plan.classes)
        self._lbook, self._book = plan.book, self._book._replace(shots=shots)
        self._resum_classes(eng, plan.classes)
        return [shots[c] for c in plan.classes]

    def shot_features(self, serial):
        """the [T, E] tower rows of a shot, a copy (a ledger with features=True)"""
        self._need_ledger("shot_features", features=True)
        if serial not in self._lbook.slot_of:
            raise ValueError("%s: %r is not the serial of a ledgered shot (shot_features)" % (self._name, serial))
        return self._lstore["features"][self._lbook.slot_of[serial]].clone()

    def move_shots(self, serials, target):
        """remove_shots(serials), then add_shots_features of their tower rows to the registered class `target`: the shots join it as its
        newest, in the order given, under new serials (returned).  Everything that can be refused is refused before anything changes."""
        self._need_ledger("move_shots", features=True)
        serials = self._serials(serials)
        ldg.plan_drop(self._lbook, serials, self._name)
        plan_shots(self._book, [target] * len(serials), self._name)       # the removal frees the room the shots take again
        feats = self._lstore["features"].index_select(0, torch.tensor([self._lbook.slot_of[s] for s in serials], device=self.dev))
        self.remove_shots(serials)
        self.add_shots_features(feats, [target] * len(serials))
        return self.last_shots

    def shot_fits(self, classes=None):
        """{class id: [(serial, fit)]} of ledgered classes (None: every one, in column order): fit is the mean over the T rows of the
        cosine between the shot's addend and the sum of the others of its class (NaN for a class of one shot).  One launch per
        TABLE_ROWS classes, one synchronisation."""
        self._need_ledger("shot_fit")
        book = self._lbook
        if classes is None:
            classes = [c for c in self._book.order if c in book.lists]
        else:
            classes = _registered(self._book, classes, self._name, "shot_fit")
            if len(set(classes)) != len(classes):
                raise ValueError("%s: a class appears twice in shot_fit: %r" % (self._name, classes))
            for c in classes:
                ldg.ledgered(book, c, "shot_fit", self._name)
        if not classes:
            return {}
        lst, outs = self._ledger_stores(), []
        for c0 in range(0, len(classes), TABLE_ROWS):
            rows, slots = ldg.resum_rows(book, classes[c0:c0 + TABLE_ROWS], self._book.slot_of)
            out = torch.empty(len(slots), device=self.dev, dtype=torch.float32)
            ldhip.fit(lst["addends"], self._store["sums"], torch.tensor(slots, device=self.dev, dtype=torch.int32), out,
                      self._ltables.upload([list(r) for r in rows]), self.T)
            outs.append(out)
        fits = iter(torch.cat(outs).cpu().tolist())
        return {c: [(s, next(fits)) for s in book.lists[c]] for c in classes}

    def shot_fit(self, cid):
        """[(serial, fit)] of one ledgered class, oldest first: shot_fits([cid])[cid]"""
        return self.shot_fits([cid])[cid]

    # ------------------------------------------------------------------ classification
    def _columns(self, classes):
        """device int32 column list of a call (raises on unknown or repeated ids)"""
        if classes is None:
            if self._cols is None:
                self._cols = torch.tensor(plan_columns(self._book), device=self.dev, dtype=torch.int32)
            return self._cols
        classes = list(classes)
        slots = plan_columns(self._book, classes, self._name)
        key = tuple(slots)
        if self._subset[0] != key:
            self._subset = (key, torch.tensor(slots, device=self.dev, dtype=torch.int32))
        return self._subset[1]

    def _n_columns(self):
        return self._active.shape[0]

    def _classify_cols(self, src, tower, classes):
        classes = None if classes is None else list(classes)
        self._fresh_engine()
        if not self._ids:
            raise RuntimeError("%s: no classes registered" % self._name)
        if classes is not None:
            plan_columns(self._book, classes, self._name)     # every error before the device is touched
        src = self._check_videos(src, "queries") if tower else self._check_feats(src)
        self._active = self._columns(classes)
        try:
            return self._classify(src, tower)
        finally:
            self._active = None

    def classify(self, queries, classes=None):
        """queries [NQ, T, 3, H, W] fp32 (device) -> logits [NQ, C] fp32 against every registered class in registration order, or against
        `classes` (registered ids, any order, no repeats) -> [NQ, len(classes)], columns in the order given"""
        return self._classify_cols(queries, True, classes)

    def classify_features(self, feats, classes=None):
        """feats [N, T, E] fp32 (device), the tower features of N clips -> the logits classify gives for those clips"""
        return self._classify_cols(feats, False, classes)

    def topk(self, queries, k=5, classes=None):
        """(values [NQ, k] fp32 descending, index [NQ, k] int32 into class_ids -- into `classes` when given); ties go to the lower index"""
        classes = None if classes is None else list(classes)
        C = len(self._ids) if classes is None else len(plan_columns(self._book, classes, self._name))
        if not 1 <= k <= min(ghip.TOPK_MAX, max(1, C)):
            raise ValueError("%s.topk: k must be in [1, min(16, number of classes)], got %d" % (self._name, k))
        logits = self.classify(queries, classes)
        values = torch.empty(logits.shape[0], k, device=self.dev, dtype=torch.float32)
        index = torch.empty(logits.shape[0], k, device=self.dev, dtype=torch.int32)
        ghip.topk(logits, k, values, index)
        return values, index

    def _score(self, eng, feats, n, ws, out, scratch):
        T, st = self.T, self._store
        Xq = self._context2(eng, feats, n, T, n_a_form=True)[:n * T].view(n, T, self.E)      # :2948
        ghip.row_norms(Xq, ws["qn"])
        lhip.otam_indexed(Xq, ws["qn"], st["P"], st["pn"], self._active, out, LAMBDA, self.single_direct)

    # ------------------------------------------------------------------ grouped classification
    def _upload_groups(self, rows):
        if self._group_tables is None or self._group_tables.max_rows < len(rows):
            self._group_tables = grhip.table_uploader(self.dev, max(TABLE_ROWS, len(rows)))
        return self._group_tables.upload(rows)

    def _plan_groups(self, counts, classes):
        """plan_groups, with what only the gallery knows: whether there are classes, and the library's group limit"""
        counts = [c.item() if isinstance(c, torch.Tensor) else c for c in (counts.reshape(-1).cpu() if isinstance(counts, torch.Tensor)
                                                                           else counts)]
        if not self._ids:
            raise RuntimeError("%s: no classes registered" % self._name)
        plan = plan_groups(self._book, counts, classes, self.T, self._name)
        if len(plan.rows) > grhip.MAX_GROUPS:
            raise ValueError("%s: %d groups, the grouped library scores at most %d per call" % (self._name, len(plan.rows),
                                                                                              grhip.MAX_GROUPS))
        return plan

    def _score_groups(self, eng, feats, n, ws, cols, rows, out, n_out):
        """a chunk of n clips under the table `rows` (chunk_groups) and its part of the slot lists -> out [n_out]: the eval branch"""
        T, st = self.T, self._store
        Xq = self._context2(eng, feats, n, T, n_a_form=True)[:n * T].view(n, T, self.E)      # :2948
        ghip.row_norms(Xq, ws["qn"])
        grhip.otam_grouped(Xq, ws["qn"], st["P"], st["pn"], cols, out, self._upload_groups(rows), n_out, LAMBDA, self.single_direct)

    def _classify_groups(self, src, tower, counts, classes):
        eng = self._fresh_engine()
        plan = self._plan_groups(counts, classes)             # every error before the device is touched
        src = self._check_videos(src, "queries") if tower else self._check_feats(src)
        N = sum(r[grhip.NQ] for r in plan.rows)
        if N != src.shape[0] or N < 1:
            raise ValueError("%s: the groups' counts add up to %d, the call holds %d clips (at least 1 is needed)" % (
                self._name, N, src.shape[0]))
        key = tuple(plan.slots)
        if self._group_cols[0] != key:
            self._group_cols = (key, torch.tensor(plan.slots, device=self.dev, dtype=torch.int32))
        cols, T = self._group_cols[1], self.T
        out = torch.empty(plan.n_out, device=self.dev, dtype=torch.float32)
        chunk = max(1, eng.max_frames // T)                   # _GalleryBase._classify's chunks: a chunk may start and end inside groups
        for q0 in range(0, N, chunk):
            q1 = min(N, q0 + chunk)
            n = q1 - q0
            ws = self._query_ws(n)
            feats = src[q0:q1]
            if tower:
                feats = ws["feats"]
                self._features(eng, src[q0:q1], feats)
            rows, (c_lo, c_hi), out_lo = chunk_groups(plan.rows, q0, q1, T)
            n_out = sum(r[grhip.NQ] * r[grhip.NC] for r in rows)
            self._score_groups(eng, feats, n, ws, cols[c_lo:c_hi], rows, out[out_lo:out_lo + n_out], n_out)
        offsets = [r[grhip.OUT0] for r in plan.rows] + [plan.n_out]
        return GroupedLogits(out, offsets, [r[grhip.NC] for r in plan.rows], [r[grhip.NQ] for r in plan.rows]), plan

    def classify_grouped(self, queries, counts, classes):
        """queries [NQ, T, 3, H, W] fp32 (device): counts[i] consecutive clips form group i and are scored against classes[i] (registered
        ids, any order, no repeats within a list; None: every class in registration order) -> GroupedLogits.  group(i) is what
        classify(those clips, classes=classes[i]) gives; the tower and context2 run once over all clips and every chunk of clips is
        scored by one launch, whatever the number of groups.  Lists may overlap and differ in length; a count may be 0."""
        return self._classify_groups(queries, True, counts, classes)[0]

    def classify_features_grouped(self, feats, counts, classes):
        """feats [N, T, E] fp32 (device), the tower features of N clips -> what classify_grouped gives for those clips"""
        return self._classify_groups(feats, False, counts, classes)[0]

    def topk_grouped(self, queries, counts, classes, k=5):
        """(values [NQ, k] fp32 descending, index [NQ, k] int32 into the query's own group's list -- into class_ids for a group of None);
        ties go to the lower index.  k is at most the shortest list of a group with clips."""
        plan = self._plan_groups(counts, classes)
        widths = [r[grhip.NC] for r in plan.rows if r[grhip.NQ]]
        if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= min([grhip.TOPK_MAX] + widths):
            raise ValueError("%s.topk_grouped: k must be in [1, min(16, the shortest class list of a group with clips)], got %r" % (
                self._name, k))
        res, plan = self._classify_groups(queries, True, counts, classes)
        return self.topk_of_groups(res.logits, plan.rows, k)

    def topk_of_groups(self, logits, rows, k):
        """top-k of flat grouped logits under the table `rows` (groups_hip.table_rows) -> (values, index), a row per query"""
        N = sum(r[grhip.NQ] for r in rows)
        values = torch.empty(N, k, device=self.dev, dtype=torch.float32)
        index = torch.empty(N, k, device=self.dev, dtype=torch.int32)
        grhip.topk_grouped(logits, self._upload_groups(rows), N, logits.shape[0], k, values, index)
        return values, index

    # ------------------------------------------------------------------ state dict
    def state_dict(self):
        """SupportGallery's keys, dense and in column order (SupportGallery.load_state_dict accepts it), plus "sums" [C, T+1, E] and
        "counts" [C] (0: no sum known)"""
        book = self._book
        C = len(book.order)
        if C:
            idx = torch.tensor(plan_columns(book), device=self.dev)
            st = self._store
            P, text, sums = (st[k].index_select(0, idx).cpu() for k in ("P", "text", "sums"))
            pn = st["pn"].view(-1, self.T).index_select(0, idx).reshape(-1).cpu()
        else:
            P, pn = torch.empty(0, self.T, self.E), torch.empty(0)
            text, sums = torch.empty(0, self.E), torch.empty(0, self._rows(), self.E)
        sd = {"fingerprint": self.fingerprint(), "class_ids": list(book.order), "prototypes": P, "norms": pn, "text": text, "sums": sums,
              "counts": [book.shots[c] for c in book.order]}
        if self._ledger is not None:
            sd["ledger"] = self._ledger_state()
        return sd

    def _ledger_state(self):
        """the "ledger" key of state_dict: the shots of the ledgered classes, class by class in column order, oldest first"""
        lb = self._lbook
        serials = [s for c in self._book.order for s in lb.lists.get(c, ())]
        led = {"serials": serials, "class_ids": [lb.class_of[s] for s in serials], "origins": [lb.origin_of[s] for s in serials],
               "next_serial": lb.next_serial, "addends": None, "features": None}
        rows = self._rows() if self.merge_before else self.T
        idx = torch.tensor([lb.slot_of[s] for s in serials], device=self.dev, dtype=torch.long)
        for key, r in (("addends", rows),) + ((("features", self.T),) if self._ledger.features else ()):
            led[key] = self._lstore[key].index_select(0, idx).cpu() if serials else torch.empty(0, r, self.E)
        return led

    def _load_ledger(self, led, ids, counts):
        """the ledger of a loaded state: its shots into the slots 0 .. n-1 in the state's order.  A class is ledgered when the state
        holds exactly its count of shots; every other class (all of them for a state without "ledger") is unledgered."""
        name = "LiveGallery.load_state_dict"
        lb = ldg.new_ledger_book(self._ledger.shots, self._lbook.next_serial)
        if led is None:
            self._ledger_forget()
            self._lbook = lb._replace(unledgered=frozenset(ids))
            return
        serials, cls, origins = list(led["serials"]), list(led["class_ids"]), list(led["origins"])
        n, rows = len(serials), self._rows() if self.merge_before else self.T
        if len(cls) != n or len(origins) != n or len(set(serials)) != n or any(o not in ldg.ORIGINS for o in origins):
            raise ValueError("%s: the ledger's serials, class ids and origins do not agree" % name)
        if n > self._ledger.shots:
            raise ValueError("%s: the state's ledger holds %d shots, this gallery's ShotLedger(shots=%d)" % (name, n, self._ledger.shots))
        if tuple(led["addends"].shape) != (n, rows, self.E):
            raise ValueError("%s: the ledger's addends have shape %s, expected %s" % (name, tuple(led["addends"].shape), (n, rows, self.E)))
        if self._ledger.features and (led.get("features") is None or tuple(led["features"].shape) != (n, self.T, self.E)):
            raise ValueError("%s: this gallery's ledger keeps tower rows (features=True), the state's has none of shape %s" % (
                name, (n, self.T, self.E)))
        self._ledger_forget()                                               # every refusal is behind us
        lists = {}
        for s, c in zip(serials, cls):
            lists.setdefault(c, []).append(s)
        have = dict(zip(ids, counts))
        good = {c for c, l in lists.items() if have.get(c, 0) == len(l)}
        keep = [i for i in range(n) if cls[i] in good]
        if keep:
            lst = self._ledger_stores()
            idx = torch.tensor(keep, dtype=torch.long)
            for key in ("addends", "features") if self._ledger.features else ("addends",):
                lst[key][:len(keep)].copy_(led[key].index_select(0, idx).to(device=self.dev, dtype=torch.float32))
        at = {serials[i]: j for j, i in enumerate(keep)}
        self._lbook = lb._replace(free=list(range(len(keep), lb.cap)), next_serial=max([lb.next_serial, int(led.get("next_serial", 0))] +
                                                                                   [s + 1 for s in serials]),
                                  slot_of=at, class_of={serials[i]: cls[i] for i in keep}, origin_of={serials[i]: origins[i] for i in keep},
                                  lists={c: lists[c] for c in good}, unledgered=frozenset(c for c in ids if c not in good))

    def load_state_dict(self, sd):
        """a LiveGallery's or a SupportGallery's state.  Classes without sums (a SupportGallery's) score normally and take no further shots."""
        if sd["fingerprint"] != self.fingerprint():
            raise ValueError("LiveGallery.load_state_dict: fingerprint %s does not match this gallery's %s" % (sd["fingerprint"],
                                                                                                                 self.fingerprint()))
        ids = list(sd["class_ids"])
        C, T, E = len(ids), self.T, self.E
        P, pn, text = sd["prototypes"], sd["norms"], sd["text"]
        if tuple(P.shape) != (C, T, E) or tuple(pn.shape) != (C * T,) or tuple(text.shape) != (C, E):
            raise ValueError("LiveGallery.load_state_dict: inconsistent shapes %s %s %s for %d classes" % (
                tuple(P.shape), tuple(pn.shape), tuple(text.shape), C))
        sums, counts = sd.get("sums"), sd.get("counts")
        if (sums is None) != (counts is None):
            raise ValueError("LiveGallery.load_state_dict: \"sums\" and \"counts\" come together")
        if sums is not None:
            counts = [int(c) for c in counts]
            if tuple(sums.shape) != (C, self._rows(), E) or len(counts) != C or any(c < 0 for c in counts):
                raise ValueError("LiveGallery.load_state_dict: inconsistent sums %s / %d counts for %d classes" % (
                    tuple(sums.shape), len(counts), C))
        if len(set(ids)) != C:
            raise ValueError("LiveGallery.load_state_dict: a class id appears twice")
        self._bind()
        if self._ledger is not None:                          # (raises on a ledger that does not fit before the store is written)
            self._load_ledger(sd.get("ledger"), ids, counts if sums is not None else [0] * C)
        old_version = self._book.version
        book = new_book(max(self._capacity, C, self._store_cap() if self._store is not None else 0))
        if C:
            plan = plan_add(book, ids, None, self._name)
            book = plan.book._replace(shots=dict(zip(ids, counts if sums is not None else [0] * C)))
            st = self._ensure_store(book.cap)
            f32 = lambda t: t.to(device=self.dev, dtype=torch.float32)
            st["P"][:C].copy_(f32(P))
            st["pn"][:C * T].copy_(f32(pn))
            st["text"][:C].copy_(f32(text))
            if sums is not None:
                st["sums"][:C].copy_(f32(sums))
        self._install(book._replace(version=old_version + 1), renew=True)
