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
    def __init__(self, head, device="cuda", capacity=64):
        head = getattr(head, "head", head)                 # BaseVideoModel -> its CNN_OTAM_CLIPFSAR head
        self._check_branch(head.args)
        if isinstance(capacity, bool) or not isinstance(capacity, int) or capacity < 1:
            raise ValueError("LiveGallery: capacity must be an integer >= 1, got %r" % (capacity,))
        self._setup(head, device)
        if self.T > lhip.MAX_T:
            raise ValueError("LiveGallery: T = %d frames, the live library scores at most %d" % (self.T, lhip.MAX_T))
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

    def _update_sequences(self, eng, X0, offs, rows):
        """Support sequences X0 [Nv, T+1, E], grouped by class (class i = sequences offs[i] .. offs[i+1]-1; rows: the classes' (slot, off,
        n, prior)) into the store: sums, prototypes, norms.  SupportGallery's launch sequence after the support sequences -- context2 class
        by class -- with cfsl_accumulate in the place of cfsg_segment_mean (prior = 0: its bits) and the norms of the touched slots alone."""
        st, T, E, n = self._store, self.T, self.E, len(rows)
        self._touch_slots([r[0] for r in rows])
        Y = None if self.merge_before else self._context2_by_class(eng, X0, offs)       # (:2955-2956)
        for c0 in range(0, n, TABLE_ROWS):
            c1 = min(n, c0 + TABLE_ROWS)
            v0, v1 = offs[c0], offs[c1]
            table = self._upload([(s, o - v0, k, p) for s, o, k, p in rows[c0:c1]])
            if self.merge_before:                             # class means BEFORE context2 (:2949-2954), the text row included
                seqs = torch.empty(c1 - c0, T + 1, E, device=self.dev, dtype=torch.float32)
                lhip.accumulate(X0[v0:v1], st["sums"], seqs, table, by_slot=False)
                Y1 = self._context2_by_class(eng, seqs, list(range(c1 - c0 + 1)))
                P = torch.empty(c1 - c0, T, E, device=self.dev, dtype=torch.float32)
                ghip.segment_mean(Y1, torch.arange(c1 - c0 + 1, device=self.dev, dtype=torch.int32), P)     # a mean over one sequence
                st["P"].index_copy_(0, torch.tensor([r[0] for r in rows[c0:c1]], device=self.dev), P)
            else:                                             # prototype = class mean of context2's first T rows (:2957-2962)
                lhip.accumulate(Y[v0:v1], st["sums"], st["P"], table, by_slot=True)
            lhip.slot_norms(st["P"], st["pn"], table)

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
        return trows, counts, plan_add(self._book if book is None else book, new_ids, counts, self._name)

    def _register_sequences(self, eng, trows, counts, plan, sequences):
        """the device work of a registration planned by _plan_classes; sequences(trows) -> (X0, offs).  -> the new column indices"""
        st = self._ensure_store(plan.book.cap)
        offs = [0]
        for k in counts:
            offs.append(offs[-1] + k)
        X0, seq_offs = sequences(trows)
        assert seq_offs == offs
        self._update_sequences(eng, X0, offs, [(s, offs[i], counts[i], 0) for i, s in enumerate(plan.slots)])
        self._write_text_rows(st, plan.slots, trows)
        C0 = len(self._book.order)
        self._install(plan.book)
        return list(range(C0, C0 + len(plan.slots)))

    def _write_text_rows(self, st, slots, trows):
        """the new classes' text rows into their slots (LiveTextGallery: and their norms)"""
        st["text"].index_copy_(0, torch.tensor(slots, device=self.dev), trows)

    def _shots_sequences(self, eng, plan, sequences):
        """the device work of further shots planned by plan_shots; sequences(trows) -> (X0, offs).  -> the classes' shot counts"""
        st = self._store
        trows = st["text"].index_select(0, torch.tensor([r[0] for r in plan.rows], device=self.dev))
        X0, offs = sequences(trows)
        self._update_sequences(eng, X0, offs, plan.rows)
        self._book = plan.book                              # the columns did not change: _ids and the device lists stay
        return [plan.book.shots[c] for c in plan.classes]

    def _add_classes(self, eng, src, class_of_video, text, sequences_of):
        ids_of_video, new_ids = self._video_classes(src, class_of_video, text)
        trows, counts, plan = self._plan_classes(eng, ids_of_video, new_ids, text)
        return self._register_sequences(eng, trows, counts, plan, lambda trows: sequences_of(src, ids_of_video, new_ids, trows))

    def _shot_ids(self, class_of_video):
        ids = [c.item() if isinstance(c, torch.Tensor) else c for c in (
            class_of_video.reshape(-1).cpu() if isinstance(class_of_video, torch.Tensor) else class_of_video)]
        return [int(c) if isinstance(c, float) and c == int(c) else c for c in ids]

    def _plan_shots(self, ids, book=None):
        """plan_shots on `book`, default the gallery's (StreamPool.enroll_windows plans a whole call on a book of its own)"""
        return plan_shots(self._book if book is None else book, ids, self._name)

    def _add_shots(self, eng, src, class_of_video, sequences_of):
        ids = self._shot_ids(class_of_video)
        if len(ids) != src.shape[0]:
            raise ValueError("%s: %d videos but %d class ids" % (self._name, src.shape[0], len(ids)))
        plan = self._plan_shots(ids)
        return self._shots_sequences(eng, plan, lambda trows: sequences_of(src, ids, plan.classes, trows))

    def add_classes(self, videos, class_of_video, text=None):
        """SupportGallery.add_classes: the same arguments, errors, return value (the new classes' column indices) and prototypes; nothing but
        the new classes is written."""
        eng = self._fresh_engine()
        videos = self._check_videos(videos, "videos")
        return self._add_classes(eng, videos, class_of_video, text, lambda *a: self._support_sequences(eng, *a))

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
        return self._add_shots(eng, videos, class_of_video, lambda *a: self._support_sequences(eng, *a))

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
        return {"fingerprint": self.fingerprint(), "class_ids": list(book.order), "prototypes": P, "norms": pn, "text": text, "sums": sums,
                "counts": [book.shots[c] for c in book.order]}

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
