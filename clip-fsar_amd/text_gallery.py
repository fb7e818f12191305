"""Text gallery: the EVAL_TEXT and COMBINE eval branches of the head over a set of registered classes, for any number of classes.

    g = TextGallery(head, device)                 # mode from TRAIN.EVAL_TEXT / TRAIN.COMBINE (EVAL_TEXT wins), or mode="eval_text" / "combine"
    g.add_text_classes([3, 7, "kite"], text={"kite": row_or_name})   # EVAL_TEXT only: zero-shot classes from their text alone
    g.add_classes(videos, class_of_video)         # as SupportGallery.add_classes; COMBINE builds the visual prototypes
    probs = g.classify(queries)                   # [NQ, T, 3, H, W] -> [NQ, C] fp32, columns in registration order
    probs = g.classify_features(feats)            # [N, T, E] tower features -> the same [N, C] (clip_fsar_amd.stream.WindowStream)
    values, index = g.topk(queries, k=5)

EVAL_TEXT (few_shot.py:2835-2852): softmax over the classes of scale * cos(mean_T of the query's tower features, the class's text row).
The class's text feature is the mean of its supports' text rows (:2838), all equal, so a class contributes its text row alone: add_classes
uses only the ids (the tower does not run) and add_text_classes registers a class from a TEST.CLASS_NAME index, an explicit [E] row or, with
VIDEO.HEAD.TEXT_TOWER, a name.  The query features are the tower's, not context2's (:2841).
COMBINE (:2855-2930): p_text^coff * softmax((8 + v) / 8)^(1 - coff), v = the default branch's OTAM logits against the class prototypes --
the prototypes of SupportGallery, since mid_layer and classification_layer are identity in this head (few_shot.py:115-116).  coff =
TRAIN.TEXT_COFF, 0.9 when unset or 0 (:2923-2926).  MERGE_BEFORE and SINGLE_DIRECT are honoured as in SupportGallery.

Both softmaxes run over the REGISTERED classes: a gallery that holds exactly an episode's classes reproduces that episode's EVAL_TEXT /
COMBINE logits, and a larger gallery gives the probabilities over all of its classes.  Both outputs are monotone in scale * cos (EVAL_TEXT)
and in coff * scale * cos + (1 - coff) * (8 + v) / 8 (COMBINE), so the ranking among classes does not depend on which other classes are
registered -- except for rounding and for values that underflow to 0, exactly as the reference's softmax.

Every arithmetic step runs on the HIP kernels: the engine's tower and context2 (libclipfsar_hip.so), norms, prototypes, OTAM and top-k
(libclipfsar_gallery.so), frame means, the text-logit GEMM, the softmax and the fusion (libclipfsar_gallery_text.so,
clip_fsar_amd.gallery_text_hip).
"""
from __future__ import annotations

import torch

from . import gallery_hip as ghip
from . import gallery_text_hip as gt
from .gallery import LAMBDA, _flag, _GalleryBase

MODES = ("eval_text", "combine")


def resolve_mode(cfg, mode=None):
    """The eval branch a TextGallery serves: the head's flags in the head's precedence (EVAL_TEXT over COMBINE, few_shot.py:240), or an
    explicit `mode` that no set flag contradicts.  Raises ValueError when neither gives one."""
    flag_mode = "eval_text" if _flag(cfg.TRAIN, "EVAL_TEXT") else ("combine" if _flag(cfg.TRAIN, "COMBINE") else None)
    if mode is None:
        if flag_mode is None:
            raise ValueError("TextGallery: the head sets neither TRAIN.EVAL_TEXT nor TRAIN.COMBINE; pass mode='eval_text' or 'combine' "
                             "(the default eval branch is SupportGallery's)")
        return flag_mode
    if mode not in MODES:
        raise ValueError("TextGallery: mode must be one of %s, got %r" % (MODES, mode))
    if flag_mode is not None and mode != flag_mode:
        raise ValueError("TextGallery: mode=%r contradicts the head's TRAIN.%s, under which the head runs the %r branch" % (
            mode, "EVAL_TEXT" if flag_mode == "eval_text" else "COMBINE", flag_mode))
    return mode


def text_coff(cfg):
    """TRAIN.TEXT_COFF as the head reads it: a falsy value means 0.9 (few_shot.py:241)"""
    return float(cfg.TRAIN.TEXT_COFF) if _flag(cfg.TRAIN, "TEXT_COFF") else 0.9


class TextGallery(_GalleryBase):
    def __init__(self, head, device="cuda", mode=None):
        head = getattr(head, "head", head)                 # BaseVideoModel -> its CNN_OTAM_CLIPFSAR head
        self.mode = resolve_mode(head.args, mode)
        self.text_coff = text_coff(head.args)
        self._setup(head, device)
        self.clear()

    def fingerprint(self):
        return dict(super().fingerprint(), mode=self.mode, text_coff=self.text_coff)

    # ------------------------------------------------------------------ state
    def clear(self):
        """Drop every class (and bind to the head's current engine)."""
        self._bind()
        f32 = lambda *s: torch.empty(*s, device=self.dev, dtype=torch.float32)
        self._ids = []
        self._text = f32(0, self.E)               # text row of every class [C, E]
        self._tn = f32(0)                         # their norms [C]
        self._P = f32(0, self.T, self.E)          # COMBINE: visual prototypes [C, T, E] (empty in EVAL_TEXT)
        self._pn = f32(0)                         # their frame-row norms [C * T]

    def state_dict(self):
        return {"fingerprint": self.fingerprint(), "class_ids": list(self._ids), "text": self._text.cpu(), "text_norms": self._tn.cpu(),
                "prototypes": self._P.cpu(), "norms": self._pn.cpu()}

    def load_state_dict(self, sd):
        if sd["fingerprint"] != self.fingerprint():
            raise ValueError("TextGallery.load_state_dict: fingerprint %s does not match this gallery's %s" % (sd["fingerprint"],
                                                                                                                 self.fingerprint()))
        C = len(sd["class_ids"])
        Cp = C if self.mode == "combine" else 0
        text, tn, P, pn = sd["text"], sd["text_norms"], sd["prototypes"], sd["norms"]
        if (tuple(text.shape) != (C, self.E) or tuple(tn.shape) != (C,) or tuple(P.shape) != (Cp, self.T, self.E)
                or tuple(pn.shape) != (Cp * self.T,)):
            raise ValueError("TextGallery.load_state_dict: inconsistent shapes %s %s %s %s for %d classes" % (
                tuple(text.shape), tuple(tn.shape), tuple(P.shape), tuple(pn.shape), C))
        self._bind()
        f32 = lambda t: t.to(device=self.dev, dtype=torch.float32).contiguous()
        self._ids, self._text, self._tn, self._P, self._pn = list(sd["class_ids"]), f32(text), f32(tn), f32(P), f32(pn)

    # ------------------------------------------------------------------ registration
    def _append(self, new_ids, trows, P=None, pn=None):
        tn = torch.empty(len(new_ids), device=self.dev, dtype=torch.float32)
        ghip.row_norms(trows, tn)
        C0 = len(self._ids)
        self._text = torch.cat([self._text, trows]).contiguous()
        self._tn = torch.cat([self._tn, tn]).contiguous()
        if P is not None:
            self._P = torch.cat([self._P, P]).contiguous()
            self._pn = torch.cat([self._pn, pn]).contiguous()
        self._ids.extend(new_ids)
        return list(range(C0, C0 + len(new_ids)))

    def add_classes(self, videos, class_of_video, text=None):
        """Register the classes of `videos` [Nv, T, 3, H, W] (fp32, device) with the ids and text rules of SupportGallery.add_classes.
        COMBINE: the visual prototypes are built exactly as SupportGallery builds them.  EVAL_TEXT: the support pixels cannot change the
        result (a class's text feature is the mean of identical rows, few_shot.py:2838), so only the ids are used and the tower does not run.
        Returns the new classes' column indices."""
        eng = self._fresh_engine()
        videos = self._check_videos(videos, "videos")
        ids_of_video, new_ids = self._video_classes(videos, class_of_video, text)
        trows = self._text_rows(eng, new_ids, text)
        if self.mode == "eval_text":
            return self._append(new_ids, trows)
        P, pn = self._prototypes(eng, videos, ids_of_video, new_ids, trows)
        return self._append(new_ids, trows, P, pn)

    def add_text_classes(self, class_ids, text=None):
        """EVAL_TEXT only: register zero-shot classes from their text alone.  class_ids: TEST.CLASS_NAME indices, or any hashable id with an
        entry in `text` ({id: class name (encoded by the text tower) or [E] text row}).  Returns the new classes' column indices."""
        if self.mode != "eval_text":
            raise ValueError("TextGallery.add_text_classes: a COMBINE gallery needs support videos -- a class with no supports has no "
                             "visual prototype; use add_classes")
        eng = self._fresh_engine()
        ids = self._new_ids(class_ids, text)
        if len(set(ids)) != len(ids):
            raise ValueError("TextGallery.add_text_classes: class ids repeat in %r" % (ids,))
        return self._append(ids, self._text_rows(eng, ids, text))

    # ------------------------------------------------------------------ classification
    def classify(self, queries):
        """queries [NQ, T, 3, H, W] fp32 (device) -> [NQ, C] fp32 against every registered class, in registration order: the text
        probabilities (EVAL_TEXT) or their fusion with the OTAM logits (COMBINE)"""
        return self._classify(queries, tower=True)

    def classify_features(self, feats):
        """feats [N, T, E] fp32 (device), the tower features of N clips -> what classify gives for those clips [N, C]"""
        return self._classify(feats, tower=False)

    def _scratch(self, nmax, C):
        partials = torch.empty(gt.workspace_floats(nmax, C), device=self.dev, dtype=torch.float32)
        vis = torch.empty(nmax, C, device=self.dev, dtype=torch.float32) if self.mode == "combine" else None
        return partials, vis

    def _score(self, eng, feats, n, ws, o, scratch):
        T, E = self.T, self.E
        partials, vis = scratch
        if "emb" not in ws:
            ws.update(emb=torch.empty(n, E, device=self.dev, dtype=torch.float32), en=torch.empty(n, device=self.dev, dtype=torch.float32))
        gt.frame_mean(feats, ws["emb"])                             # :2838-2841 (tower features, not context2's); both halves read them
        ghip.row_norms(ws["emb"], ws["en"])
        gt.text_logits(ws["emb"], ws["en"], self._text, self._tn, eng.scale, o, partials)
        if self.mode == "eval_text":
            gt.text_softmax(o, partials, o)
            return
        Xq = self._context2(eng, feats, n, T, n_a_form=True)[:n * T].view(n, T, E)        # :2948
        ghip.row_norms(Xq, ws["qn"])
        ghip.otam_gallery(Xq, ws["qn"], self._P, self._pn, vis[:n], LAMBDA, self.single_direct)
        gt.text_combine(o, partials, vis[:n], o, self.text_coff)
