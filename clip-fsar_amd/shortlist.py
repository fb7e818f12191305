"""Shortlist: two-stage scoring over a LiveGallery -- a cheap score over all classes picks `keep` candidates per group of clips, and the
exact cosine + OTAM kernel runs on those alone.

Every scoring path of the galleries pays a T x T x E similarity block and two soft-min DPs per (query, class) pair, and topk, events and
an operator's screen only ever look at a handful of classes per window.  OTAM walks the matrix cos(q_i, p_j); the mean of that matrix over
its T x T cells is one dot product <u_q, u_p>, with u the mean of a sequence's unit-normalised rows -- about T * T times cheaper than the
pair's OTAM.  That coarse score is a heuristic, not a bound, so the contract is exact where it can be:

  * which classes are selected is a bit-for-bit function of the coarse scores (reference_select restates the rule on the host);
  * the logits of the selected classes are the bits LiveGallery.classify_features_grouped gives for the same clips, groups and lists --
    which are the bits of classify(those clips, classes=<selected>) wherever context2 does not depend on its batch (its fp32 GEMMs pick
    their kernel by row count: up to 192 rows, 24 clips of T = 8, they are one kernel);
  * recall against full scoring is measured (tools/shortlist_time.py), not promised.

    sl = Shortlist(g, keep=64)                               # g: a LiveGallery (the default eval branch)
    r = sl.classify(queries, counts=None, classes=None)      # counts None: every clip its own group; else counts[i] consecutive clips
                                                             # share one shortlist (the windows of one stream)
    r.logits, r.columns, r.keep                              # [N, K] fp32; [G, K] int32 on the device: indices into classes= (into
                                                             # g.class_ids when None), ascending, 0x7fffffff = none; K = min(keep, candidates)
    r.class_ids()                                            # the one sync: per group the ids behind r.columns (None: no class)
    values, index = sl.topk(queries, k=5, counts=None, classes=None)   # index counts in classes= / class_ids, not in the shortlist
    sl.classify_features(feats, ...); sl.topk_features(feats, ...)     # tower features [N, T, E] instead of pixels
    sl.coarse_features(feats, classes=None)                  # [N, NC] coarse scores, for inspection and for the tests
    sl.stats                                                 # {"calls", "refreshed"}: coarse rows recomputed so far

A call first sends up the lists it makes on the host (the candidates' slots, the stale slots, for topk the group of every clip), as the
gallery does with its column lists.  Then it runs the tower and context2 in the gallery's chunks into one [N, T, E] buffer, takes the
row norms, recomputes the coarse rows of the candidate slots whose prototype was written since (LiveGallery.slot_revision), computes the query rows, the coarse scores and the
selection (libclipfsar_shortlist.so, clip_fsar_amd.shortlist_hip), and makes ONE cfgr_otam_grouped launch over the selected slot lists,
which never leave the device: between the first launch and the result the host does not synchronise.  A place without a class (fewer than
K selectable candidates) has slot -1 and a NaN logit, cfgr's rule, and topk never selects it.

The group score of a class is the MAXIMUM of its coarse scores over the group's clips: a class that only one window of a stream likes
still gets in.  With one clip per group an OTAM tile carries a single query row; counts= is the efficient form.
"""
from __future__ import annotations

import collections

import torch

from . import gallery_hip as ghip
from . import groups_hip as grhip
from . import shortlist_hip as shhip
from .gallery import LAMBDA
from .live_gallery import LiveGallery, plan_columns

MAX_KEEP = shhip.MAX_KEEP
NONE = shhip.NONE
TINY = shhip.TINY


# ---------------------------------------------------------------------------------------------------------------- references (pure)
def reference_mean_unit_rows(X, norms, tiny=TINY):
    """float64: X [n, T, E], norms [n * T] (as given: the fp32 norms the kernel reads) -> [n, E], the mean over t of X[., t] / max(norm, tiny)"""
    X = torch.as_tensor(X).double()
    n, T, _ = X.shape
    d = torch.as_tensor(norms).double().reshape(n, T).clamp_min(float(tiny))
    return (X / d[:, :, None]).sum(1) / T


def reference_coarse(U, C):
    """float64: U [NQ, E], C [NC, E] -> [NQ, NC] dot products"""
    return torch.as_tensor(U).double() @ torch.as_tensor(C).double().T


def reference_select(S, counts, keep):
    """The selection rule of cfsh_select on the host.  S: [NQ, NC] scores (a tensor or nested lists; fp32 values are exact as Python
    floats), counts: clips per group, consecutive; keep >= 1 -> per group a list of K = min(keep, NC) columns: the K best by group score
    (the maximum over the group's clips, NaN ignored; a column without a score, or with -inf, is not selectable), the larger score first
    and the lower column on equal scores (-0.0 == +0.0), written in ascending column order and padded with NONE at the end."""
    rows = S.tolist() if hasattr(S, "tolist") else [list(r) for r in S]
    counts = list(counts)
    if sum(counts) != len(rows):
        raise ValueError("reference_select: the counts add up to %d, S has %d rows" % (sum(counts), len(rows)))
    NC = len(rows[0]) if rows else 0
    K = min(int(keep), NC)
    out, q = [], 0
    for n in counts:
        best = []
        for c, column in enumerate(zip(*rows[q:q + n])):       # a group without clips has no columns here: nothing is selectable
            vals = [v for v in column if v == v]
            if vals and max(vals) > float("-inf"):
                best.append((-max(vals), c))                   # -(-0.0) == -(+0.0): the column decides
        q += n
        kept = sorted(c for _, c in sorted(best)[:K])
        out.append(kept + [NONE] * (K - len(kept)))
    return out


def reference_select_pinned(S, counts, keep, pinned):
    """The selection rule of cfps_select_pinned (include/ext/clipfsar_pool_select.h) on the host.  S, counts, keep: as reference_select;
    pinned: per group the pinned columns with their bits, {column: bits != 0} (or None: no pins) -> (columns, pins, n_pins): per group
    the K = min(keep, NC) kept columns in ascending order padded with NONE, their bits (0: kept on its score, and at padded places), and
    P, the number of pinned columns.  P <= K: every pin is kept whatever its score, the other K - P places go to the best selectable
    columns that are not pinned (reference_select's order).  P > K: the K best pins, the larger score first and the lower column on equal
    scores, a pin that is not selectable below every score by lower column.  A group without clips keeps nothing and counts no pin."""
    rows = S.tolist() if hasattr(S, "tolist") else [list(r) for r in S]
    counts = list(counts)
    if sum(counts) != len(rows):
        raise ValueError("reference_select_pinned: the counts add up to %d, S has %d rows" % (sum(counts), len(rows)))
    if len(pinned) != len(counts):
        raise ValueError("reference_select_pinned: %d groups, pins for %d" % (len(counts), len(pinned)))
    NC = len(rows[0]) if rows else 0
    K = min(int(keep), NC)
    columns, pins, n_pins, q = [], [], [], 0
    for n, pin in zip(counts, pinned):
        pin = dict(pin or {}) if n else {}
        if any(not 0 <= c < NC or not bits for c, bits in pin.items()):
            raise ValueError("reference_select_pinned: a pin names a column outside [0, %d) or carries no bit: %r" % (NC, pin))
        score = {}                                             # the selectable columns' group scores
        for c, column in enumerate(zip(*rows[q:q + n])):
            vals = [v for v in column if v == v]
            if vals and max(vals) > float("-inf"):
                score[c] = max(vals)
        q += n
        if len(pin) <= K:
            free = sorted((-v, c) for c, v in score.items() if c not in pin)[:K - len(pin)]
            kept = sorted(list(pin) + [c for _, c in free])
        else:                                                  # (0, -score, column) before (1, column): a pin without a score is last
            kept = sorted(sorted(pin, key=lambda c: (0, -score[c], c) if c in score else (1, 0.0, c))[:K])
        columns.append(kept + [NONE] * (K - len(kept)))
        pins.append([pin.get(c, 0) for c in kept] + [0] * (K - len(kept)))
        n_pins.append(len(pin))
    return columns, pins, n_pins


# ---------------------------------------------------------------------------------------------------------------- the class
class ShortlistResult:
    """logits [N, K] fp32, columns [G, K] int32 (device; indices into the call's candidate list, ascending, NONE = no class), keep = K,
    counts: clips per group."""
    __slots__ = ("logits", "columns", "keep", "counts", "_ids")

    def __init__(self, logits, columns, keep, counts, ids):
        self.logits, self.columns, self.keep, self.counts, self._ids = logits, columns, keep, counts, ids

    def class_ids(self):
        """per group the class ids behind `columns` (None where a place holds no class).  Synchronises: the columns come to the host."""
        return [[self._ids[c] if c != NONE else None for c in row] for row in self.columns.cpu().tolist()]


_Plan = collections.namedtuple("_Plan", "eng ids slots K counts N")
_PoolPrep = collections.namedtuple("_PoolPrep", "eng ids K cols pending")


class Shortlist:
    def __init__(self, gallery, keep=64):
        from .live_text_gallery import LiveTextGallery
        if isinstance(gallery, LiveTextGallery):
            raise ValueError("Shortlist: a %s is refused -- its softmaxes are defined over the listed classes, and a softmax over a "
                             "shortlist is a different quantity" % type(gallery).__name__)
        if not isinstance(gallery, LiveGallery):
            raise TypeError("Shortlist: needs a LiveGallery (a slot store whose lists live on the device), not a %s"
                            % type(gallery).__name__)
        if isinstance(keep, bool) or not isinstance(keep, int) or not 1 <= keep <= MAX_KEEP:
            raise ValueError("Shortlist: keep must be an integer in [1, %d], got %r" % (MAX_KEEP, keep))
        self.gallery, self.keep = gallery, keep
        self._coarse = None                                # [cap, E] coarse rows, slot by slot
        self._rev = []                                     # the revision of the slot each row was computed at; -1: never
        self._tables = None
        self._all = (None, None, None)                     # (the gallery's book, the slots of all its classes, their ids)
        self._clean = (None, None)                         # (the candidate slots last found fresh, the gallery's write count then)
        self._groups = (None, None)                        # (the counts of the last topk, the clips' groups on the device)
        self.stats = {"calls": 0, "refreshed": 0}

    # ------------------------------------------------------------------ what a call decides before the device is touched
    def _ready(self):
        """the gallery's engine, fresh, and at least one class"""
        eng = self.gallery._fresh_engine()
        if not self.gallery._ids:
            raise RuntimeError("Shortlist: no classes registered")
        return eng

    def _every_class(self):
        """(the slots of all the gallery's classes, their ids): the lists are kept while the gallery's book is the same one"""
        g = self.gallery
        if self._all[0] is not g._book:
            self._all = (g._book, plan_columns(g._book), list(g._book.order))
        return self._all[1], self._all[2]

    def _plan(self, src, tower, counts, classes, k=None):
        g = self.gallery
        eng = self._ready()
        if classes is None:
            slots, ids = self._every_class()
        else:
            ids = list(classes)
            slots = plan_columns(g._book, ids, "Shortlist")
        K = min(self.keep, len(slots))
        if k is not None and (isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= min(grhip.TOPK_MAX, K)):
            raise ValueError("Shortlist.topk: k must be in [1, min(16, K = %d = min(keep, number of candidates))], got %r" % (K, k))
        if counts is not None:
            counts = [c.item() if isinstance(c, torch.Tensor) else c for c in (counts.reshape(-1).cpu() if isinstance(counts, torch.Tensor)
                                                                               else counts)]
            if not counts or any(isinstance(n, bool) or not isinstance(n, int) or n < 0 for n in counts):
                raise ValueError("Shortlist: counts must be a non-empty list of integers >= 0, got %r" % (counts,))
        src = g._check_videos(src, "queries") if tower else g._check_feats(src)
        N = src.shape[0]
        counts = [1] * N if counts is None else counts
        if sum(counts) != N or N < 1:
            raise ValueError("Shortlist: the groups' counts add up to %d, the call holds %d clips (at least 1 is needed)" % (sum(counts), N))
        if len(counts) > shhip.MAX_GROUPS:
            raise ValueError("Shortlist: %d groups, at most %d are scored per call" % (len(counts), shhip.MAX_GROUPS))
        return src, _Plan(eng, ids, slots, K, counts, N)

    # ------------------------------------------------------------------ the stages
    def _queries(self, eng, src, tower):
        """tower (pixels) and context2 in the gallery's chunks -> (Xq [N, T, E], qn [N * T])"""
        g = self.gallery
        N, T, E = src.shape[0], g.T, g.E
        Xq = torch.empty(N, T, E, device=g.dev, dtype=torch.float32)
        chunk = max(1, eng.max_frames // T)
        for q0 in range(0, N, chunk):
            q1 = min(N, q0 + chunk)
            n = q1 - q0
            feats = src[q0:q1]
            if tower:
                feats = g._query_ws(n)["feats"]
                g._features(eng, src[q0:q1], feats)
            Xq[q0:q1].view(n * T, E).copy_(g._context2(eng, feats, n, T, n_a_form=True)[:n * T])
        qn = torch.empty(N * T, device=g.dev, dtype=torch.float32)
        ghip.row_norms(Xq, qn)
        return Xq, qn

    def _stale(self, slots):
        """What a call uploads BEFORE its first launch (a list made on the host reaches the device by a copy that waits for the stream, as
        the gallery's own lists do): the candidate slots whose prototype was written since their coarse row was computed -> (slots, the
        gallery's write count now, the stale ones, their device list), or None when there are none.  No launch, and nothing is marked
        fresh yet: _refresh does both."""
        g = self.gallery
        mine, theirs, writes = self._rev, g._slot_rev, g._writes
        mine.extend([-1] * (g._store_cap() - len(mine)))
        if writes == self._clean[1] and (slots is self._clean[0] or slots == self._clean[0]):
            return None                                    # the list that was clean last time, and no slot of the gallery written since
        stale = [s for s in slots if mine[s] != theirs[s]]
        if not stale:
            self._clean = (slots, writes)
            return None
        return slots, writes, stale, torch.tensor(stale, device=g.dev, dtype=torch.int32)

    def _refresh(self, pending):
        """the coarse store, grown with the gallery's, and the coarse rows of the stale candidate slots (_stale's answer): one launch over
        their list"""
        g = self.gallery
        cap = g._store_cap()
        if self._coarse is None or self._coarse.shape[0] != cap:
            grown = torch.empty(cap, g.E, device=g.dev, dtype=torch.float32)
            if self._coarse is not None:
                grown[:self._coarse.shape[0]].copy_(self._coarse)      # the gallery's growth copied the prototypes: the rows stay valid
            self._coarse = grown
        if pending is not None:
            slots, writes, stale, stale_dev = pending
            st, mine, theirs = g._store, self._rev, g._slot_rev
            shhip.mean_unit_rows(st["P"], st["pn"], stale_dev, self._coarse)
            for s in stale:
                mine[s] = theirs[s]
            self.stats["refreshed"] += len(stale)
            self._clean = (slots, writes)
        return self._coarse

    def _group_of(self, counts):
        """[N] int64 on the device: the group of every clip (topk's gather through sel_cols).  Uploaded before the call's first launch,
        and kept while the counts stay the same."""
        if self._groups[0] != counts:
            group = [i for i, n in enumerate(counts) for _ in range(n)]
            self._groups = (list(counts), torch.tensor(group, device=self.gallery.dev, dtype=torch.int64))
        return self._groups[1]

    def _coarse_scores(self, Xq, qn, pending, cols):
        """-> S [N, NC]: the query rows against the (refreshed) coarse rows of the candidates (cols: their slots on the device)"""
        g = self.gallery
        coarse = self._refresh(pending)
        N = Xq.shape[0]
        U = torch.empty(N, g.E, device=g.dev, dtype=torch.float32)
        shhip.mean_unit_rows(Xq, qn, None, U)
        S = torch.empty(N, cols.shape[0], device=g.dev, dtype=torch.float32)
        shhip.coarse_scores(U, coarse, cols, S)
        return S

    def _select(self, S, cols, counts, K):
        """-> (sel_cols, sel_slots) [G, K] int32 on the device"""
        g = self.gallery
        G, NC = len(counts), S.shape[1]
        if self._tables is None or self._tables.max_rows < G:
            self._tables = shhip.table_uploader(g.dev, max(1024, G))
        rows, _ = shhip.table_rows(counts)
        sel_cols = torch.empty(G, K, device=g.dev, dtype=torch.int32)
        sel_slots = torch.empty(G, K, device=g.dev, dtype=torch.int32)
        work = torch.empty(shhip.workspace_floats(G, NC), device=g.dev, dtype=torch.float32)
        shhip.select(S, cols, self._tables.upload(rows), self.keep, sel_cols, sel_slots, work)
        return sel_cols, sel_slots

    def _exact(self, Xq, qn, sel_slots, counts, K):
        """one grouped launch over the selected lists (every width is K: the table is known on the host) -> (flat logits, table rows)"""
        g = self.gallery
        st = g._store
        rows, (_, _, _, n_out) = grhip.table_rows(counts, [K] * len(counts), g.T)
        out = torch.empty(n_out, device=g.dev, dtype=torch.float32)
        grhip.otam_grouped(Xq, qn, st["P"], st["pn"], sel_slots.view(-1), out, g._upload_groups(rows), n_out, LAMBDA, g.single_direct)
        return out, rows

    def _run(self, src, tower, counts, classes, k=None):
        src, p = self._plan(src, tower, counts, classes, k)
        g = self.gallery
        cols = g._columns(None if classes is None else p.ids)             # every list made on the host goes up here, ahead of the
        pending = self._stale(p.slots)                                    # first launch: from there on the host only enqueues
        group = None if k is None else self._group_of(p.counts)
        Xq, qn = self._queries(p.eng, src, tower)
        S = self._coarse_scores(Xq, qn, pending, cols)
        sel_cols, sel_slots = self._select(S, cols, p.counts, p.K)
        flat, rows = self._exact(Xq, qn, sel_slots, p.counts, p.K)
        self.stats["calls"] += 1
        res = ShortlistResult(flat.view(p.N, p.K), sel_cols, p.K, p.counts, p.ids)
        if k is None:
            return res
        values, index = g.topk_of_groups(flat, rows, k)                   # index: places of the shortlist, NONE where there is none
        found = index != NONE
        place = torch.where(found, index, torch.zeros_like(index)).long()
        return values, torch.where(found, sel_cols[group].gather(1, place), index)

    # ------------------------------------------------------------------ the entry of StreamPool(shortlist=...)
    def _pool_prepare(self):
        """The host half of a pool's push, before its first launch: the candidates are every registered class.  -> _PoolPrep(eng, ids,
        K, cols: the candidates' slots on the device, pending: _stale's answer).  Every list made on the host goes up here."""
        g = self.gallery
        eng = self._ready()
        slots, ids = self._every_class()
        return _PoolPrep(eng, ids, min(self.keep, len(slots)), g._columns(None), self._stale(slots))

    def _pool_score(self, prep, X, counts, select):
        """The device half: X [NW, T, E], the tower features of the push's windows, group-major (counts[i] consecutive windows per group)
        -> (sel_cols, sel_slots [G, K] on the device, the flat logits, the table rows of the grouped launch).  _run's stages with
        select(S, cols, K) -> (sel_cols, sel_slots) -- the pool's pinned selection -- in the place of _select.  Only enqueues."""
        Xq, qn = self._queries(prep.eng, X, False)
        S = self._coarse_scores(Xq, qn, prep.pending, prep.cols)
        sel_cols, sel_slots = select(S, prep.cols, prep.K)
        flat, rows = self._exact(Xq, qn, sel_slots, counts, prep.K)
        self.stats["calls"] += 1
        return sel_cols, sel_slots, flat, rows

    # ------------------------------------------------------------------ the public calls
    def classify(self, queries, counts=None, classes=None):
        """queries [N, T, 3, H, W] fp32 (device) -> ShortlistResult: per group of counts[i] consecutive clips (None: every clip alone) the K
        best candidates of `classes` (registered ids, any order, no repeats; None: every class) by coarse score, and the exact logits of
        the group's clips against them"""
        return self._run(queries, True, counts, classes)

    def classify_features(self, feats, counts=None, classes=None):
        """feats [N, T, E] fp32 (device), the tower features of N clips -> what classify gives for those clips"""
        return self._run(feats, False, counts, classes)

    def topk(self, queries, k=5, counts=None, classes=None):
        """(values [N, k] fp32 descending, index [N, k] int32 into classes= -- into class_ids when None; 0x7fffffff where the shortlist
        holds fewer than k classes); ties go to the lower index.  k is at most min(16, K)."""
        return self._run(queries, True, counts, classes, k)

    def topk_features(self, feats, k=5, counts=None, classes=None):
        """topk from tower features [N, T, E]"""
        return self._run(feats, False, counts, classes, k)

    def coarse_features(self, feats, classes=None):
        """[N, NC] fp32: the coarse score of every clip against every candidate, the matrix the selection of a classify_features call on
        the same clips reads"""
        src, p = self._plan(feats, False, None, classes)
        cols = self.gallery._columns(None if classes is None else p.ids)
        pending = self._stale(p.slots)
        Xq, qn = self._queries(p.eng, src, False)
        return self._coarse_scores(Xq, qn, pending, cols)
