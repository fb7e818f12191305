"""Support gallery: register classes once from a few example videos each, then classify any stream of query videos against all of them.
(Whole T-frame clips, that is; for the overlapping windows of a continuous frame stream see clip_fsar_amd.stream.WindowStream, which runs
the tower once per frame and scores the windows through classify_features.)

In the reference's eval branch (few_shot.py:2944-2990) queries and supports meet only in cos_sim and OTAM: a query goes through context2
alone (:2948), a support sequence is its T frame features plus its class's text token and goes through context2 without any query
(:2955-2956), and the prototype is the class mean of those outputs (:2957-2962) -- or, with MERGE_BEFORE, context2 of the class mean taken
before it.  So a prototype depends only on its own class's supports, and stored prototypes give an episode's logits exactly; the support
work is paid once, at registration.

    g = SupportGallery(head, device)             # a CNN_OTAM_CLIPFSAR head (or build_model(cfg)[0].head)
    g.add_classes(videos, class_of_video)        # videos [Nv, T, 3, H, W] fp32 on the device; ids index TEST.CLASS_NAME
    logits = g.classify(queries)                 # [NQ, T, 3, H, W] -> [NQ, C] fp32, columns in registration order
    logits = g.classify_features(feats)          # [N, T, E] tower features (a cache, a WindowStream's ring) -> the same [N, C]
    values, index = g.topk(queries, k=5)

Every arithmetic step runs on the HIP kernels: the engine's tower (HipViT / HipResNet) and context2 (libclipfsar_hip.so), the support
sequences, class means, norms, the gallery cosine + OTAM and the top-k (libclipfsar_gallery.so, clip_fsar_amd.gallery_hip).

The head's other two eval branches, TRAIN.EVAL_TEXT (zero-shot text matching) and TRAIN.COMBINE (text probabilities fused with these
OTAM logits), are served by clip_fsar_amd.text_gallery.TextGallery, which shares the machinery below (_GalleryBase).  A gallery whose classes also leave,
receive further shots and are scored in subsets is clip_fsar_amd.live_gallery.LiveGallery.
"""
from __future__ import annotations

import torch

from . import gallery_hip as ghip

LAMBDA = 0.5                       # OTAM soft-min temperature (few_shot.py:2979-2982)


def _flag(ns, name):
    return bool(hasattr(ns, name) and getattr(ns, name))


class _GalleryBase:
    """What SupportGallery and TextGallery (clip_fsar_amd.text_gallery) share: the binding to the head's engine, class ids and their text
    rows, the tower, context2 and the visual prototypes of the default eval branch."""

    def _setup(self, head, device):
        cfg = head.args
        self.head = head
        self.dev = torch.device(device)
        self.T = int(cfg.DATA.NUM_INPUT_FRAMES)
        self.merge_before = _flag(cfg.TRAIN, "MERGE_BEFORE")
        self.single_direct = _flag(cfg.TRAIN, "SINGLE_DIRECT")
        self._bind()
        self.E = int(self._engine.arch["embed"])
        self._qws = {}

    @property
    def _name(self):
        return type(self).__name__

    # ------------------------------------------------------------------ engine binding
    def _bind(self):
        self._engine = self.head._get_engine(self.dev)
        self._engine_key = self.head._engine_key

    def _fresh_engine(self):
        """The engine the prototypes were computed with.  Raises when the head has rebuilt it since (load_state_dict, new text tables,
        invalidate_engine ...): old prototypes are never mixed with new weights."""
        eng = self.head._get_engine(self.dev)
        if eng is not self._engine or self.head._engine_key != self._engine_key:
            raise RuntimeError("%s: the head's weights or text tables changed since these prototypes were computed; clear() "
                               "the gallery and add the classes again" % self._name)
        return eng

    def fingerprint(self):
        h = self.head
        return {"arch": h.arch_name, "precision": h.precision, "depth": int(h.depth), "T": self.T, "merge_before": self.merge_before}

    # ------------------------------------------------------------------ state
    def __len__(self):
        return len(self._ids)

    @property
    def class_ids(self):
        return list(self._ids)

    # ------------------------------------------------------------------ registration
    def _text_rows(self, eng, ids, text):
        """[n, E] fp32 device text rows of the new classes: TEST.CLASS_NAME rows (:2946), explicit [E] rows, or names through the text tower"""
        n_test = eng.text_test.shape[0]
        rows, names = [None] * len(ids), {}
        for i, cid in enumerate(ids):
            src = text.get(cid) if text is not None else None
            if src is None:
                if isinstance(cid, bool) or not isinstance(cid, int) or not 0 <= cid < n_test:
                    raise ValueError("%s: class %r is not an index into TEST.CLASS_NAME (%d classes) and has no entry in `text`"
                                     % (self._name, cid, n_test))
                rows[i] = eng.text_test[cid]
            elif isinstance(src, str):
                names[i] = src
            else:
                t = torch.as_tensor(src).to(device=self.dev, dtype=torch.float32).reshape(-1)
                if t.numel() != self.E:
                    raise ValueError("%s: text row of class %r has %d values, expected %d" % (self._name, cid, t.numel(), self.E))
                rows[i] = t
        if names:
            enc = self._encode_names([names[i] for i in sorted(names)])
            for j, i in enumerate(sorted(names)):
                rows[i] = enc[j]
        return torch.stack(rows).contiguous()

    def _encode_names(self, names):
        """New class names -> text rows through the HIP text encoder (clip_fsar_amd.text), as the head builds TEST.CLASS_NAME's table"""
        h = self.head
        cfg = h.args
        src = getattr(cfg.VIDEO.HEAD, "TEXT_TOWER", None)
        if not src:
            raise ValueError("%s: class names outside TEST.CLASS_NAME need VIDEO.HEAD.TEXT_TOWER (the text encoder); pass "
                             "explicit [E] text rows instead" % self._name)
        from . import text as ctext
        from .models.base.few_shot import _load_state_dict_file
        if src == "synthetic":
            tsd = ctext.text_tower_state_dict(width=768 if self.E == 768 else 512, layers=12, embed=self.E,
                                              seed=int(getattr(cfg, "RANDOM_SEED", 18)))
        else:
            tsd = {k: v for k, v in _load_state_dict_file(src).items() if not k.startswith("visual.")}
        template = cfg.TEST.PROMPT if (hasattr(cfg.TEST, "PROMPT") and cfg.TEST.PROMPT) else None
        tok = ctext.ClipBpeTokenizer(getattr(cfg.VIDEO.HEAD, "BPE_PATH", None))
        enc = ctext.HipTextEncoder(tsd, device=self.dev)
        return enc.encode(tok.tokenize(ctext.prompts(list(names), template))).to(device=self.dev, dtype=torch.float32)

    def _features(self, eng, videos, out):
        """videos [N, T, 3, H, W] -> out [N, T, E]: the engine's tower, in chunks of engine.max_frames frames"""
        N, T = videos.shape[0], self.T
        frames = videos.reshape(N * T, *videos.shape[2:])
        out2d = out.view(N * T, self.E)
        chunk = max(1, eng.max_frames // T)
        for v0 in range(0, N, chunk):
            v1 = min(N, v0 + chunk)
            eng.vit.forward(frames[v0 * T:v1 * T], out2d[v0 * T:v1 * T])

    def _context2(self, eng, seqs, n_seq, seq_len, n_a_form):
        """context2 on n_seq sequences of seq_len rows (seqs [n_seq * seq_len, E], contiguous) -> the workspace buffer holding the output"""
        rows = n_seq * seq_len
        th = eng.temporal
        th._workspace(rows)["X"][:rows].copy_(seqs.view(rows, self.E))
        if n_a_form:                                          # queries: the a-sequences of cfsar_seq_attention
            return th.run_layers(rows, n_seq, seq_len, 0, seq_len + 1)
        return th.run_layers(rows, 0, seq_len - 1, n_seq, seq_len)

    def _check_videos(self, videos, what):
        if not isinstance(videos, torch.Tensor) or not videos.is_cuda:
            raise RuntimeError("%s: %s must be a HIP device tensor (no CPU path exists)" % (self._name, what))
        if videos.dim() != 5 or videos.shape[1] != self.T or videos.shape[2] != 3:
            raise ValueError("%s: %s must be [N, T=%d, 3, H, W], got %s" % (self._name, what, self.T, tuple(videos.shape)))
        return videos.to(dtype=torch.float32).contiguous()

    def _new_ids(self, ids, text):
        """ids as plain hashables; raises on ids already registered and on a `text` that is not a dict"""
        ids = [c.item() if isinstance(c, torch.Tensor) else c for c in (ids.reshape(-1).cpu() if isinstance(ids, torch.Tensor) else ids)]
        ids = [int(c) if isinstance(c, float) and c == int(c) else c for c in ids]
        dup = [c for c in dict.fromkeys(ids) if c in self._ids]
        if dup:
            raise ValueError("%s: class %r is already registered" % (self._name, dup[0]))
        if text is not None and not isinstance(text, dict):
            raise TypeError("%s: `text` must map class id -> class name or [E] text row" % self._name)
        return ids

    def _video_classes(self, videos, class_of_video, text):
        """(class id of every video, the new classes in first-appearance order)"""
        ids_of_video = self._new_ids(class_of_video, text)
        if len(ids_of_video) != videos.shape[0]:
            raise ValueError("%s: %d videos but %d class ids" % (self._name, videos.shape[0], len(ids_of_video)))
        return ids_of_video, list(dict.fromkeys(ids_of_video))

    def _support_sequences(self, eng, videos, ids_of_video, new_ids, trows):
        """(X0 [Nv, T+1, E]: the support sequences grouped by class in the order of new_ids, video order inside a class; offs: the classes'
        runs in it, len(new_ids) + 1 prefix sums).  The tower runs in the caller's video order."""
        feats = torch.empty(videos.shape[0], self.T, self.E, device=self.dev, dtype=torch.float32)
        self._features(eng, videos, feats)
        return self._sequences_of_features(feats, ids_of_video, new_ids, trows)

    def _sequences_of_features(self, feats, ids_of_video, new_ids, trows):
        """_support_sequences after the tower: feats [Nv, T, E] in the caller's video order -> (X0, offs)"""
        Nv = feats.shape[0]
        n = len(new_ids)
        local = {c: i for i, c in enumerate(new_ids)}
        order = sorted(range(Nv), key=lambda v: (local[ids_of_video[v]], v))     # videos grouped by class, video order inside a class
        counts = [0] * n
        for c in ids_of_video:
            counts[local[c]] += 1
        offs = [0]
        for k in counts:
            offs.append(offs[-1] + k)
        T, E = self.T, self.E
        # the class-grouped support sequences [Nv, T+1, E]
        feats = feats[torch.tensor(order, device=self.dev)].contiguous()
        cls_local = torch.tensor([local[ids_of_video[v]] for v in order], device=self.dev, dtype=torch.int32)
        X0 = torch.empty(Nv, T + 1, E, device=self.dev, dtype=torch.float32)
        ghip.support_sequences(feats, trows, cls_local, X0)
        return X0, offs

    def _context2_by_class(self, eng, seqs, seq_offs):
        """context2 class by class (seqs [., T+1, E], class i = sequences seq_offs[i] .. seq_offs[i+1]-1): a class's prototype never depends
        on how the classes were grouped into calls"""
        T, E = self.T, self.E
        Y = torch.empty_like(seqs)
        for i in range(len(seq_offs) - 1):
            s0, s1 = seq_offs[i], seq_offs[i + 1]
            out = self._context2(eng, seqs[s0:s1], s1 - s0, T + 1, n_a_form=False)
            Y[s0:s1].view(-1, E).copy_(out[:(s1 - s0) * (T + 1)])
        return Y

    def _prototypes(self, eng, videos, ids_of_video, new_ids, trows):
        """The visual prototypes [n, T, E] of the new classes and their frame-row norms [n * T] (few_shot.py:2944-2962)"""
        n = len(new_ids)
        T, E = self.T, self.E
        X0, offs = self._support_sequences(eng, videos, ids_of_video, new_ids, trows)
        offsets = torch.tensor(offs, device=self.dev, dtype=torch.int32)
        if self.merge_before:                                 # class means BEFORE context2 (:2949-2954), the text row included
            seqs = torch.empty(n, T + 1, E, device=self.dev, dtype=torch.float32)
            ghip.segment_mean(X0, offsets, seqs)
            seq_offs = list(range(n + 1))
        else:
            seqs, seq_offs = X0, offs
        Y = self._context2_by_class(eng, seqs, seq_offs)
        P = torch.empty(n, T, E, device=self.dev, dtype=torch.float32)
        # prototype = class mean of the first T rows (:2957-2962); with MERGE_BEFORE the one merged sequence's rows (a mean over one video)
        ghip.segment_mean(Y, offsets if not self.merge_before else torch.arange(n + 1, device=self.dev, dtype=torch.int32), P)
        pn = torch.empty(n * T, device=self.dev, dtype=torch.float32)
        ghip.row_norms(P, pn)
        return P, pn

    # ------------------------------------------------------------------ classification
    def _query_ws(self, n):
        ws = self._qws.get(n)
        if ws is None:
            ws = dict(feats=torch.empty(n, self.T, self.E, device=self.dev, dtype=torch.float32),
                      qn=torch.empty(n * self.T, device=self.dev, dtype=torch.float32))
            self._qws[n] = ws
        return ws

    def _check_feats(self, feats):
        if not isinstance(feats, torch.Tensor) or not feats.is_cuda:
            raise RuntimeError("%s: feats must be a HIP device tensor (no CPU path exists)" % self._name)
        if feats.dim() != 3 or feats.shape[1] != self.T or feats.shape[2] != self.E:
            raise ValueError("%s: feats must be [N, T=%d, E=%d], got %s" % (self._name, self.T, self.E, tuple(feats.shape)))
        return feats.to(dtype=torch.float32).contiguous()

    def _n_columns(self):
        """columns of the logits a classify call returns (LiveGallery: of the subset it was asked for)"""
        return len(self._ids)

    def _scratch(self, nmax, C):
        """per-call buffers of _score for chunks of at most nmax clips"""
        return None

    def _classify(self, src, tower):
        """classify (tower=True: src = the clips' pixels, the tower runs chunk by chunk) and classify_features (src = their tower features):
        one loop, so both score a chunk with the same launches.  The subclass's _score(eng, feats [n, T, E], n, ws, out [n, C], scratch)
        holds its eval branch."""
        eng = self._fresh_engine()
        if not self._ids:
            raise RuntimeError("%s: no classes registered" % self._name)
        src = self._check_videos(src, "queries") if tower else self._check_feats(src)
        N, C = src.shape[0], self._n_columns()
        out = torch.empty(N, C, device=self.dev, dtype=torch.float32)
        chunk = max(1, eng.max_frames // self.T)
        scratch = self._scratch(min(N, chunk), C)
        for q0 in range(0, N, chunk):
            q1 = min(N, q0 + chunk)
            ws = self._query_ws(q1 - q0)
            feats = src[q0:q1]
            if tower:
                feats = ws["feats"]
                self._features(eng, src[q0:q1], feats)
            self._score(eng, feats, q1 - q0, ws, out[q0:q1], scratch)
        return out

    def topk(self, queries, k=5):
        """(values [NQ, k] fp32 descending, class index [NQ, k] int32 into class_ids); ties go to the lower index"""
        if not 1 <= k <= min(ghip.TOPK_MAX, max(1, len(self._ids))):
            raise ValueError("%s.topk: k must be in [1, min(16, number of classes)], got %d" % (self._name, k))
        logits = self.classify(queries)
        values = torch.empty(logits.shape[0], k, device=self.dev, dtype=torch.float32)
        index = torch.empty(logits.shape[0], k, device=self.dev, dtype=torch.int32)
        ghip.topk(logits, k, values, index)
        return values, index


class SupportGallery(_GalleryBase):
    def __init__(self, head, device="cuda"):
        head = getattr(head, "head", head)                 # BaseVideoModel -> its CNN_OTAM_CLIPFSAR head
        cfg = head.args
        for flag in ("EVAL_TEXT", "COMBINE"):
            if _flag(cfg.TRAIN, flag):
                raise NotImplementedError("SupportGallery: TRAIN.%s is not supported -- the gallery serves the default eval branch "
                                          "(cosine + OTAM of context2 features, few_shot.py:2944-2990) only; use "
                                          "clip_fsar_amd.text_gallery.TextGallery for this branch" % flag)
        self._setup(head, device)
        self.clear()

    def clear(self):
        """Drop every class (and bind to the head's current engine)."""
        self._bind()
        self._ids = []
        self._P = torch.empty(0, self.T, self.E, device=self.dev, dtype=torch.float32)      # prototypes [C, T, E]
        self._pn = torch.empty(0, device=self.dev, dtype=torch.float32)                     # their frame-row norms [C * T]
        self._text = torch.empty(0, self.E, device=self.dev, dtype=torch.float32)           # text row of every class [C, E]

    def state_dict(self):
        return {"fingerprint": self.fingerprint(), "class_ids": list(self._ids), "prototypes": self._P.cpu(), "norms": self._pn.cpu(),
                "text": self._text.cpu()}

    def load_state_dict(self, sd):
        if sd["fingerprint"] != self.fingerprint():
            raise ValueError("SupportGallery.load_state_dict: fingerprint %s does not match this gallery's %s" % (sd["fingerprint"],
                                                                                                                    self.fingerprint()))
        C = len(sd["class_ids"])
        P, pn, text = sd["prototypes"], sd["norms"], sd["text"]
        if tuple(P.shape) != (C, self.T, self.E) or tuple(pn.shape) != (C * self.T,) or tuple(text.shape) != (C, self.E):
            raise ValueError("SupportGallery.load_state_dict: inconsistent shapes %s %s %s for %d classes" % (
                tuple(P.shape), tuple(pn.shape), tuple(text.shape), C))
        self._bind()
        f32 = lambda t: t.to(device=self.dev, dtype=torch.float32).contiguous()
        self._ids, self._P, self._pn, self._text = list(sd["class_ids"]), f32(P), f32(pn), f32(text)

    def add_classes(self, videos, class_of_video, text=None):
        """Register the classes of `videos` [Nv, T, 3, H, W] (fp32, device).  class_of_video [Nv]: the class id of every video -- an index into
        TEST.CLASS_NAME (text row = text_features_test[id], few_shot.py:2946), or any hashable id with an entry in `text` ({id: class name
        (encoded by the text tower) or [E] text row}).  Classes are appended in order of first appearance; any number of videos per class.
        Returns the new classes' column indices."""
        eng = self._fresh_engine()
        videos = self._check_videos(videos, "videos")
        ids_of_video, new_ids = self._video_classes(videos, class_of_video, text)
        trows = self._text_rows(eng, new_ids, text)
        P, pn = self._prototypes(eng, videos, ids_of_video, new_ids, trows)
        C0, n = len(self._ids), len(new_ids)
        self._P = torch.cat([self._P, P]).contiguous()
        self._pn = torch.cat([self._pn, pn]).contiguous()
        self._text = torch.cat([self._text, trows]).contiguous()
        self._ids.extend(new_ids)
        return list(range(C0, C0 + n))

    def classify(self, queries):
        """queries [NQ, T, 3, H, W] fp32 (device) -> logits [NQ, C] fp32 = -(OTAM + OTAM^T) against every registered class, in registration order"""
        return self._classify(queries, tower=True)

    def classify_features(self, feats):
        """feats [N, T, E] fp32 (device), the tower features of N clips -> the logits [N, C] classify gives for those clips"""
        return self._classify(feats, tower=False)

    def _score(self, eng, feats, n, ws, out, scratch):
        T = self.T
        Xq = self._context2(eng, feats, n, T, n_a_form=True)[:n * T].view(n, T, self.E)      # :2948
        # the gallery kernel at every class count: faster than the episode kernel (cfsar_cos_otam_logits) from C = 5 on
        # (1.7 x at 1 024 queries x 5 classes, 4.9 x at 24, 11.5 x at 1 024; profiles/gallery_time.json)
        ghip.row_norms(Xq, ws["qn"])
        ghip.otam_gallery(Xq, ws["qn"], self._P, self._pn, out, LAMBDA, self.single_direct)
