"""Live text gallery: the EVAL_TEXT and COMBINE eval branches (clip_fsar_amd.text_gallery.TextGallery's) over a LiveGallery's store --
classes that leave, take further shots (COMBINE) and are scored in subsets, per tenant or per episode, and that a stream pool enrols.

    g = LiveTextGallery(head, device, mode=None, capacity=64)     # mode as TextGallery's: the head's flags, or "eval_text" / "combine"
    g.add_classes(videos, class_of_video)        # COMBINE: LiveGallery's prototypes, bit for bit; EVAL_TEXT: the ids alone, no tower
    g.add_text_classes([3, "kite"], text={"kite": row_or_name})   # EVAL_TEXT only
    g.add_shots(videos, class_of_video)          # COMBINE only: an EVAL_TEXT class is its text row
    g.remove_classes([3, 7])                     # LiveGallery's: an int list changes, layout_version rises
    probs = g.classify(queries, classes=[9, 2])  # [NQ, 2]: BOTH softmaxes over exactly the listed classes, columns in the order given
    r = g.classify_grouped(queries, counts=[3, 2], classes=[[9, 2], None])       # GroupedLogits, each group over its own list
    g.topk(queries, k=5, classes=None); g.topk_grouped(queries, counts, classes, k=5)
    g.state_dict()                               # TextGallery's keys (dense, column order) + "sums" and "counts"; each loads the other's

Both branches end in a softmax over the classes (few_shot.py:2849, :2921-2928), so the scores against a subset are not columns of the
scores against all: classify(classes=L) is what a TextGallery holding exactly L returns.  The store is LiveGallery's with one more
buffer, the text rows' norms; a column is a slot number, and the kernels (libclipfsar_live_text.so, clip_fsar_amd.live_text_hip) take
their classes from slot lists, one per group.  There is ONE scoring path: classify is the grouped call with one group.  Per chunk of
clips: cfgt_frame_mean, cfsg_row_norms, one cflt_text_logits_grouped, then cflt_text_softmax_grouped (EVAL_TEXT) or context2 +
cfsg_row_norms + cfgr_otam_grouped + cflt_text_combine_grouped (COMBINE).
"""
from __future__ import annotations

import collections

import torch

from . import gallery_hip as ghip
from . import gallery_text_hip as gt
from . import groups_hip as grhip
from . import live_text_hip as ltx
from .live_gallery import TABLE_ROWS, LiveGallery, new_book, plan_add, plan_columns, plan_groups
from .text_gallery import resolve_mode, text_coff

# GroupPlan's fields and, for the text kernels, the same groups as live_text_hip's table and their number of softmax partials
TextGroupPlan = collections.namedtuple("TextGroupPlan", "rows slots n_out text_rows n_part")


def text_rows_of(rows):
    """groups_hip's table -> (live_text_hip's table of the same groups, NPART)"""
    trows, (_, _, _, _, n_part) = ltx.table_rows([r[grhip.NQ] for r in rows], [r[grhip.NC] for r in rows])
    return trows, n_part


def plan_text_groups(book, counts, classes, T, name="LiveTextGallery"):
    """plan_groups (its rules and errors) -> TextGroupPlan: the OTAM table for frames of T, the slot lists, the number of outputs, and
    the text kernels' 8-column table with its number of partials"""
    plan = plan_groups(book, counts, classes, T, name)
    trows, n_part = text_rows_of(plan.rows)
    return TextGroupPlan(plan.rows, plan.slots, plan.n_out, trows, n_part)


class LiveTextGallery(LiveGallery):
    def __init__(self, head, device="cuda", mode=None, capacity=64):
        head = getattr(head, "head", head)                 # BaseVideoModel -> its CNN_OTAM_CLIPFSAR head
        self.mode = resolve_mode(head.args, mode)
        self.text_coff = text_coff(head.args)
        self._text_tables = None
        self._bufs = {}                                    # partials and the visual half: grown on demand
        super().__init__(head, device, capacity)

    def _check_branch(self, cfg):
        pass                                               # resolve_mode decided: this gallery serves the two text branches

    def fingerprint(self):
        return dict(super().fingerprint(), mode=self.mode, text_coff=self.text_coff)         # TextGallery's

    # ------------------------------------------------------------------ the store: LiveGallery's + the text rows' norms
    def _alloc(self, cap):
        f = dict(device=self.dev, dtype=torch.float32)
        st = super()._alloc(cap) if self.mode == "combine" else {"text": torch.empty(cap, self.E, **f)}      # EVAL_TEXT: no P, no sums
        st["tn"] = torch.empty(cap, **f)
        return st

    def _write_text_rows(self, st, slots, trows):
        super()._write_text_rows(st, slots, trows)
        tn = torch.empty(len(slots), device=self.dev, dtype=torch.float32)
        ghip.row_norms(trows, tn)
        st["tn"].index_copy_(0, torch.tensor(slots, device=self.dev), tn)

    # ------------------------------------------------------------------ registration
    # COMBINE: everything is LiveGallery's.  EVAL_TEXT: a class is its text row (few_shot.py:2838: the mean of its supports' identical
    # rows) -- registration uses the ids alone, the shot count is 0 and no shot can follow.
    def _plan_classes(self, eng, ids_of_video, new_ids, text, book=None):
        if self.mode == "combine":
            return super()._plan_classes(eng, ids_of_video, new_ids, text, book)
        trows = self._text_rows(eng, new_ids, text)
        plan = plan_add(self._book if book is None else book, new_ids, None, self._name)
        shots = dict(plan.book.shots)
        shots.update(dict.fromkeys(new_ids, 0))               # plan_add counts a shot each: here a class has none
        return trows, [0] * len(new_ids), plan._replace(book=plan.book._replace(shots=shots))

    def _register_sequences(self, eng, trows, counts, plan, sequences, origin="enroll"):
        if self.mode == "combine":
            return super()._register_sequences(eng, trows, counts, plan, sequences, origin)
        st = self._ensure_store(plan.book.cap)                # the sequences are not made: nothing reads them
        self._write_text_rows(st, plan.slots, trows)
        C0 = len(self._book.order)
        self._install(plan.book)
        return list(range(C0, C0 + len(plan.slots)))

    def _register_text(self, eng, new_ids, text):
        trows, counts, plan = self._plan_classes(eng, [], new_ids, text)
        return self._register_sequences(eng, trows, counts, plan, None)

    def add_classes(self, videos, class_of_video, text=None):
        """COMBINE: LiveGallery.add_classes.  EVAL_TEXT: TextGallery.add_classes -- the ids and text rules alone, the tower does not run."""
        if self.mode == "combine":
            return super().add_classes(videos, class_of_video, text)
        eng = self._fresh_engine()
        videos = self._check_videos(videos, "videos")
        return self._register_text(eng, self._video_classes(videos, class_of_video, text)[1], text)

    def add_classes_features(self, feats, class_of_video, text=None):
        if self.mode == "combine":
            return super().add_classes_features(feats, class_of_video, text)
        eng = self._fresh_engine()
        feats = self._check_feats(feats)
        return self._register_text(eng, self._video_classes(feats, class_of_video, text)[1], text)

    def add_text_classes(self, class_ids, text=None):
        """EVAL_TEXT only: register zero-shot classes from their text alone (TextGallery.add_text_classes' rules).  Returns the new
        classes' column indices."""
        if self.mode != "eval_text":
            raise ValueError("LiveTextGallery.add_text_classes: a COMBINE gallery needs support videos -- a class with no supports has no "
                             "visual prototype; use add_classes")
        eng = self._fresh_engine()
        ids = self._new_ids(class_ids, text)
        if len(set(ids)) != len(ids):
            raise ValueError("LiveTextGallery.add_text_classes: class ids repeat in %r" % (ids,))
        return self._register_text(eng, ids, text)

    def _plan_shots(self, ids, book=None):
        if self.mode == "eval_text":
            raise ValueError("%s: an EVAL_TEXT class is its text row and takes no shots (further videos cannot change its scores); "
                             "add_shots needs a COMBINE gallery" % self._name)
        return super()._plan_shots(ids, book)

    def add_shots(self, videos, class_of_video):
        if self.mode == "eval_text":
            self._plan_shots(None)                            # before the device tensor is looked at
        return super().add_shots(videos, class_of_video)

    def add_shots_features(self, feats, class_of_video):
        if self.mode == "eval_text":
            self._plan_shots(None)
        return super().add_shots_features(feats, class_of_video)

    # ------------------------------------------------------------------ classification: one path, the grouped one
    def _plan_groups(self, counts, classes):
        plan = super()._plan_groups(counts, classes)          # LiveGallery's checks and errors (grhip.MAX_GROUPS == ltx.MAX_GROUPS)
        trows, n_part = text_rows_of(plan.rows)
        return TextGroupPlan(plan.rows, plan.slots, plan.n_out, trows, n_part)

    def _upload_text_groups(self, rows):
        if self._text_tables is None or self._text_tables.max_rows < len(rows):
            self._text_tables = ltx.table_uploader(self.dev, max(TABLE_ROWS, len(rows)))
        return self._text_tables.upload(rows)

    def _buf(self, key, n):
        b = self._bufs.get(key)
        if b is None or b.shape[0] < n:
            b = self._bufs[key] = torch.empty(n, device=self.dev, dtype=torch.float32)
        return b

    def _score_groups(self, eng, feats, n, ws, cols, rows, out, n_out):
        st = self._store
        trows, n_part = text_rows_of(rows)
        table = self._upload_text_groups(trows)
        partials = self._buf("partials", 2 * n_part)
        if "emb" not in ws:
            ws.update(emb=torch.empty(n, self.E, device=self.dev, dtype=torch.float32), en=torch.empty(n, device=self.dev, dtype=torch.float32))
        gt.frame_mean(feats, ws["emb"])                       # :2838-2841 (tower features, not context2's)
        ghip.row_norms(ws["emb"], ws["en"])
        ltx.text_logits_grouped(ws["emb"], ws["en"], st["text"], st["tn"], cols, eng.scale, out, partials, table, n_out, n_part)
        if self.mode == "eval_text":
            ltx.text_softmax_grouped(out, partials, out, table, n, n_out, n_part)
            return
        vis = self._buf("visual", n_out)
        super()._score_groups(eng, feats, n, ws, cols, rows, vis, n_out)        # context2, its norms, cfgr_otam_grouped: the same OUT0
        ltx.text_combine_grouped(out, partials, vis, out, table, n, n_out, n_part, self.text_coff)

    def _classify_cols(self, src, tower, classes):
        """classify / classify_features: LiveGallery's checks in its order, then the grouped path with one group"""
        classes = None if classes is None else list(classes)
        self._fresh_engine()
        if not self._ids:
            raise RuntimeError("%s: no classes registered" % self._name)
        C = len(plan_columns(self._book, classes, self._name))   # every error before the device is touched
        src = self._check_videos(src, "queries") if tower else self._check_feats(src)
        N = src.shape[0]
        if N == 0:
            return torch.empty(0, C, device=self.dev, dtype=torch.float32)
        return self._classify_groups(src, tower, [N], [classes])[0].logits.view(N, C)

    def topk(self, queries, k=5, classes=None):
        """(values [NQ, k] fp32 descending, index [NQ, k] int32 into class_ids -- into `classes` when given); ties go to the lower index"""
        classes = None if classes is None else list(classes)
        C = len(self._ids) if classes is None else len(plan_columns(self._book, classes, self._name))
        if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= min(grhip.TOPK_MAX, max(1, C)):
            raise ValueError("%s.topk: k must be in [1, min(16, number of classes)], got %r" % (self._name, k))
        probs = self.classify(queries, classes)
        N = probs.shape[0]
        if N == 0:
            return (torch.empty(0, k, device=self.dev, dtype=torch.float32), torch.empty(0, k, device=self.dev, dtype=torch.int32))
        return self.topk_of_groups(probs.view(-1), grhip.table_rows([N], [C], self.T)[0], k)

    # ------------------------------------------------------------------ state dict
    def state_dict(self):
        """TextGallery's keys, dense and in column order (TextGallery.load_state_dict accepts it), plus "sums" [C, T+1, E] and "counts"
        [C] (0: no sum known; EVAL_TEXT: no prototypes, no sums, every count 0)"""
        book, T, E = self._book, self.T, self.E
        C = len(book.order)
        Cp = C if self.mode == "combine" else 0
        P, pn, sums = torch.empty(Cp, T, E), torch.empty(Cp * T), torch.empty(Cp, self._rows(), E)
        text, tn = torch.empty(C, E), torch.empty(C)
        if C:
            idx = torch.tensor(plan_columns(book), device=self.dev)
            st = self._store
            text, tn = st["text"].index_select(0, idx).cpu(), st["tn"].index_select(0, idx).cpu()
            if Cp:
                P, sums = st["P"].index_select(0, idx).cpu(), st["sums"].index_select(0, idx).cpu()
                pn = st["pn"].view(-1, T).index_select(0, idx).reshape(-1).cpu()
        return {"fingerprint": self.fingerprint(), "class_ids": list(book.order), "text": text, "text_norms": tn, "prototypes": P,
                "norms": pn, "sums": sums, "counts": [book.shots[c] for c in book.order]}

    def load_state_dict(self, sd):
        """a LiveTextGallery's or a TextGallery's state.  Classes without sums (a TextGallery's) score normally and take no further shots."""
        who = "LiveTextGallery.load_state_dict"
        if sd["fingerprint"] != self.fingerprint():
            raise ValueError("%s: fingerprint %s does not match this gallery's %s" % (who, sd["fingerprint"], self.fingerprint()))
        ids = list(sd["class_ids"])
        C, T, E = len(ids), self.T, self.E
        Cp = C if self.mode == "combine" else 0
        text, tn, P, pn = sd["text"], sd["text_norms"], sd["prototypes"], sd["norms"]
        if tuple(text.shape) != (C, E) or tuple(tn.shape) != (C,) or tuple(P.shape) != (Cp, T, E) or tuple(pn.shape) != (Cp * T,):
            raise ValueError("%s: inconsistent shapes %s %s %s %s for %d classes" % (who, tuple(text.shape), tuple(tn.shape),
                                                                                     tuple(P.shape), tuple(pn.shape), C))
        sums, counts = sd.get("sums"), sd.get("counts")
        if (sums is None) != (counts is None):
            raise ValueError("%s: \"sums\" and \"counts\" come together" % who)
        if sums is not None:
            counts = [int(c) for c in counts]
            if tuple(sums.shape) != (Cp, self._rows(), E) or len(counts) != C or any(c < 0 for c in counts):
                raise ValueError("%s: inconsistent sums %s / %d counts for %d classes" % (who, tuple(sums.shape), len(counts), C))
        if len(set(ids)) != C:
            raise ValueError("%s: a class id appears twice" % who)
        self._bind()
        old_version = self._book.version
        book = new_book(max(self._capacity, C, self._store_cap() if self._store is not None else 0))
        if C:
            plan = plan_add(book, ids, None, self._name)
            book = plan.book._replace(shots=dict(zip(ids, counts if sums is not None and Cp else [0] * C)))
            st = self._ensure_store(book.cap)
            f32 = lambda t: t.to(device=self.dev, dtype=torch.float32)
            st["text"][:C].copy_(f32(text))
            st["tn"][:C].copy_(f32(tn))
            if Cp:
                st["P"][:C].copy_(f32(P))
                st["pn"][:C * T].copy_(f32(pn))
                if sums is not None:
                    st["sums"][:C].copy_(f32(sums))
        self._install(book._replace(version=old_version + 1), renew=True)
