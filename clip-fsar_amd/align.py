"""Aligner: the OTAM soft alignment behind a score, frame by frame, over a LiveGallery.

A logit of the default eval branch is -(F(D) + F(D^T)): D is the T x T cosine-distance matrix of one (clip, class) pair and F the OTAM
soft-min DP.  That DP defines a soft alignment over frames, the gradient dF/dD: cell (l, m) is the probability that the soft path pairs
query frame l with prototype frame m.  The scoring kernels compute D, walk it and throw both away; libclipfsar_align.so
(clip_fsar_amd.align_hip) keeps them -- one workgroup per pair, a stabilised forward pass and a backward pass.

    al = Aligner(g)                                          # g: a LiveGallery (the default eval branch)
    a = al.align_features(feats, classes=[9, 2])             # feats [N, T, E] tower features: every clip against class 9 and class 2
    a = al.align_features(feats, classes=[[9], [], [2, 4]])  # N lists: clip i against its own classes (an empty list: no pair)
    a = al.align_features(feats, k=3)                        # every clip against its own top-3 classes, found on the device
    a = al.align(queries, ...)                               # the same from pixels [N, T, 3, H, W]
    a.plan, a.dists, a.logits                                # [NP, T, T], [NP, T, T], [NP] fp32 on the device, pair by pair
    a.pairs, a.offsets                                       # [NP, 2] int32 on the device: (clip, column into the call's class list -- into
                                                             # the clip's own list, into g.class_ids with k=); clip i owns the pairs
                                                             # offsets[i] .. offsets[i + 1] - 1 (a host list)
    a.class_ids()                                            # the one sync: per clip the class ids of its pairs (None: no class)
    a.frame_cost, a.frame_match                              # [NP, T]: a query frame's share of the pair's cost, sum_m plan * dists, and
                                                             # the prototype frame it is expected at, sum_m plan * m / sum_m plan

A call first sends up the lists it makes on the host (the pairs' clips, columns and store slots), as the gallery does with its column
lists.  Then context2 runs once, in the gallery's chunks; with k= the clips are scored against every class and the top-k taken by the
gallery's own launches (cfsl_otam_indexed, cfsg_topk), and the slot list is made on the device from the top-k index: between the first
launch and the result the host only enqueues.  A top-k place without a class has slot -1 and is NaN in every output.

reference_alignment restates the arithmetic on the host, in float64 or -- every step -- in float32.
"""
from __future__ import annotations

import torch

from . import align_hip as alhip
from . import gallery_hip as ghip
from . import live_hip as lhip
from .gallery import LAMBDA
from .live_gallery import LiveGallery, plan_columns

NONE = 0x7fffffff                  # a top-k place without a class: the index cfsg_topk writes there


# ---------------------------------------------------------------------------------------------------------------- the reference (pure)
def _predecessors(l, m, T):
    """of cell (l, m), l >= 1, of the padded grid, in the order the sums are taken"""
    if m == 1:
        return [(l - 1, 0), (l - 1, 1), (l, 0)]
    if m == T + 1:
        return [(l - 1, T), (l - 1, T + 1), (l, T)]
    return [(l - 1, m - 1), (l, m - 1)]


def _forward_backward(d, lam):
    """d [B, T, T] -> (F [B], G [B, T, T]) in d's dtype: the padded recurrence with the stabilised soft-min and its gradient, cell by cell"""
    B, T, _ = d.shape
    zero = torch.zeros(B, dtype=d.dtype)
    pad = lambda l, m: d[:, l, m - 1] if m <= T else zero                     # the padded d: 0 at m = T + 1
    c = [[zero] * (T + 2) for _ in range(T)]
    for m in range(1, T + 2):
        c[0][m] = pad(0, m) + c[0][m - 1]
    for l in range(1, T):
        for m in range(1, T + 2):
            xs = [c[i][j] for i, j in _predecessors(l, m, T)]
            mn = xs[0]
            for x in xs[1:]:
                mn = torch.minimum(mn, x)
            total = torch.exp((mn - xs[0]) / lam)
            for x in xs[1:]:
                total = total + torch.exp((mn - x) / lam)
            c[l][m] = pad(l, m) + (mn - lam * torch.log(total))
    a = [[zero] * (T + 2) for _ in range(T)]
    a[T - 1][T + 1] = torch.ones(B, dtype=d.dtype)
    G = torch.zeros(B, T, T, dtype=d.dtype)
    for l in range(T - 1, 0, -1):
        for m in range(T + 1, 0, -1):
            s = c[l][m] - pad(l, m)
            for i, j in _predecessors(l, m, T):
                if j:                                                         # flow into a padding cell c[.][0] is dropped
                    a[i][j] = a[i][j] + a[l][m] * torch.exp((s - c[i][j]) / lam)
            if m <= T:
                G[:, l, m - 1] = a[l][m]
    run = zero
    for m in range(T + 1, 0, -1):                                             # row 0 is a running sum
        run = run + a[0][m]
        if m <= T:
            G[:, 0, m - 1] = run
    return c[T - 1][T + 1], G


def reference_alignment(D, lam, single_direct=False, dtype=torch.float64):
    """D [..., T, T] cosine distances -> (value [...], plan [..., T, T]) in `dtype`: value = F(D) + F(D^T) and plan = G(D) + G(D^T)^T, or
    F(D) and G(D) with single_direct -- F the OTAM soft-min DP with the soft-min taken relative to its smallest argument, G = dF/dD.
    dtype=torch.float32 performs every step in fp32 (what cfal_align's error is measured against float64 with)."""
    D = (D if isinstance(D, torch.Tensor) else torch.tensor(D, dtype=torch.float64)).detach().cpu().to(dtype)
    if D.dim() < 2 or D.shape[-1] != D.shape[-2] or D.shape[-1] < 1:
        raise ValueError("reference_alignment: D must be [..., T, T], got %s" % (tuple(D.shape),))
    if not float(lam) > 0.0:
        raise ValueError("reference_alignment: lambda must be positive, got %r" % (lam,))
    T = D.shape[-1]
    d = D.reshape(-1, T, T)
    value, plan = _forward_backward(d, float(lam))
    if not single_direct:
        v1, g1 = _forward_backward(d.transpose(1, 2).contiguous(), float(lam))
        value, plan = value + v1, plan + g1.transpose(1, 2)
    return value.reshape(D.shape[:-2]), plan.reshape(D.shape)


# ---------------------------------------------------------------------------------------------------------------- the result
class Alignment:
    """pairs [NP, 2] int32 (device): (clip, column into the call's class list); offsets: host list, clip i owns the pairs
    offsets[i] .. offsets[i + 1] - 1; plan, dists [NP, T, T] and logits [NP] fp32 (device)."""
    __slots__ = ("pairs", "offsets", "plan", "dists", "logits", "_ids")

    def __init__(self, pairs, offsets, plan, dists, logits, ids):
        self.pairs, self.offsets, self.plan, self.dists, self.logits, self._ids = pairs, offsets, plan, dists, logits, ids

    def __len__(self):
        return self.plan.shape[0]

    def class_ids(self):
        """per clip the class ids of its pairs, in pair order (None where a place holds no class).  Synchronises: the columns come to
        the host."""
        cols = self.pairs[:, 1].cpu().tolist()
        ids, out = self._ids, []
        for i, (p0, p1) in enumerate(zip(self.offsets, self.offsets[1:])):
            mine = ids[i] if ids and isinstance(ids[0], list) else ids
            out.append([mine[c] if 0 <= c < len(mine) else None for c in cols[p0:p1]])
        return out

    @property
    def frame_cost(self):
        """[NP, T]: per query frame the cost the soft path pays there, sum over m of plan * dists"""
        return (self.plan * self.dists).sum(-1)

    @property
    def frame_match(self):
        """[NP, T]: per query frame the prototype frame the soft path is expected at, sum over m of plan * m / sum over m of plan"""
        m = torch.arange(self.plan.shape[-1], device=self.plan.device, dtype=self.plan.dtype)
        return (self.plan * m).sum(-1) / self.plan.sum(-1)


class _Plan:
    """what a call decides before the device is touched: N clips; k, or the host lists pair_q, column, slot of the NP pairs; offsets; ids"""
    __slots__ = ("eng", "N", "k", "pair_q", "column", "slot", "offsets", "ids")

    def __init__(self, eng, N, k, pair_q, column, slot, offsets, ids):
        self.eng, self.N, self.k, self.pair_q, self.column, self.slot, self.offsets, self.ids = eng, N, k, pair_q, column, slot, offsets, ids


# ---------------------------------------------------------------------------------------------------------------- the class
class Aligner:
    def __init__(self, gallery):
        from .live_text_gallery import LiveTextGallery
        if isinstance(gallery, LiveTextGallery):
            raise ValueError("Aligner: a %s is refused -- its scores are softmaxes over text and OTAM logits, and the alignment explains "
                             "the OTAM logit of the default eval branch alone" % type(gallery).__name__)
        if not isinstance(gallery, LiveGallery):
            raise TypeError("Aligner: needs a LiveGallery (a slot store whose lists live on the device), not a %s" % type(gallery).__name__)
        if gallery.T > alhip.MAX_T:
            raise ValueError("Aligner: T = %d frames, the alignment library takes at most %d" % (gallery.T, alhip.MAX_T))
        self.gallery = gallery

    # ------------------------------------------------------------------ what a call decides before the device is touched
    def _plan(self, N, classes, k):
        g = self.gallery
        eng = g._fresh_engine()
        if not g._ids:
            raise RuntimeError("Aligner: no classes registered")
        if (classes is None) == (k is None):
            raise ValueError("Aligner: give exactly one of classes= and k=, got classes=%r and k=%r" % (classes, k))
        if N < 1:
            raise ValueError("Aligner: the call holds %d clips, at least 1 is needed" % N)
        if k is not None:
            if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= min(ghip.TOPK_MAX, len(g)):
                raise ValueError("Aligner: k must be in [1, min(16, number of classes = %d)], got %r" % (len(g), k))
            return _Plan(eng, N, k, None, None, None, [i * k for i in range(N + 1)], list(g._book.order))
        classes = list(classes)
        if classes and all(isinstance(c, (list, tuple)) for c in classes):    # N lists, clip i against its own
            if len(classes) != N:
                raise ValueError("Aligner: %d class lists for %d clips" % (len(classes), N))
            ids = [list(c) for c in classes]
            lists = [plan_columns(g._book, c, "Aligner: clip %d" % i) if c else [] for i, c in enumerate(ids)]
        else:                                                                 # one flat list: every clip against each
            ids = classes
            lists = [plan_columns(g._book, classes, "Aligner")] * N
        pair_q = [i for i, l in enumerate(lists) for _ in l]
        if not pair_q:
            raise ValueError("Aligner: every clip's class list is empty -- there is no pair to align")
        offsets = [0]
        for l in lists:
            offsets.append(offsets[-1] + len(l))
        return _Plan(eng, N, None, pair_q, [j for l in lists for j in range(len(l))], [s for l in lists for s in l], offsets, ids)

    # ------------------------------------------------------------------ the stages
    def _queries(self, eng, src, tower):
        """tower (pixels) and context2 in the gallery's chunks -> (Xq [N, T, E], qn [N * T]); the call's first launch"""
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

    def _topk_pairs(self, Xq, qn, cols, k):
        """every clip scored against every class and its top-k taken, the gallery's own launches -> (pairs [N * k, 2], slots [N * k])
        on the device; a place without a class has column NONE and slot -1"""
        g = self.gallery
        st, N, C = g._store, Xq.shape[0], cols.shape[0]
        logits = torch.empty(N, C, device=g.dev, dtype=torch.float32)
        lhip.otam_indexed(Xq, qn, st["P"], st["pn"], cols, logits, LAMBDA, g.single_direct)
        values = torch.empty(N, k, device=g.dev, dtype=torch.float32)
        index = torch.empty(N, k, device=g.dev, dtype=torch.int32)
        ghip.topk(logits, k, values, index)
        found = (index >= 0) & (index < C)
        place = torch.where(found, index, torch.zeros_like(index)).long()
        slots = torch.where(found, cols[place], torch.full_like(index, -1))
        clip = torch.arange(N, device=g.dev, dtype=torch.int32).view(N, 1).expand(N, k)
        return torch.stack((clip, index), dim=2).view(N * k, 2).contiguous(), slots.reshape(N * k).contiguous()

    def _run(self, p, src, tower):
        g = self.gallery
        T = g.T
        if p.k is None:                                                       # every list made on the host goes up here, ahead of the
            pairs = torch.tensor(list(zip(p.pair_q, p.column)), device=g.dev, dtype=torch.int32)     # first launch: from there on the
            slots = torch.tensor(p.slot, device=g.dev, dtype=torch.int32)                            # host only enqueues
        else:
            cols = g._columns(None)
        Xq, qn = self._queries(p.eng, src, tower)
        if p.k is not None:
            pairs, slots = self._topk_pairs(Xq, qn, cols, p.k)
        NP = pairs.shape[0]
        st = g._store
        plan = torch.empty(NP, T, T, device=g.dev, dtype=torch.float32)
        dists = torch.empty(NP, T, T, device=g.dev, dtype=torch.float32)
        logits = torch.empty(NP, device=g.dev, dtype=torch.float32)
        alhip.align(Xq, qn, st["P"], st["pn"], pairs[:, 0].contiguous(), slots, LAMBDA, g.single_direct, plan, dists, logits)
        return Alignment(pairs, p.offsets, plan, dists, logits, p.ids)

    # ------------------------------------------------------------------ the public calls
    def align_features(self, feats, classes=None, k=None):
        """feats [N, T, E] fp32 (device), the tower features of N clips -> Alignment.  Give exactly one of classes -- a flat list of
        registered ids (any order, no repeats): every clip against each; or N lists: clip i against its own, an empty list allowed -- and
        k in [1, min(16, number of classes)]: every clip against its own top-k classes."""
        if not isinstance(feats, torch.Tensor) or feats.dim() != 3:
            self.gallery._check_feats(feats)                                  # raises
        p = self._plan(feats.shape[0], classes, k)
        return self._run(p, self.gallery._check_feats(feats), False)

    def align(self, queries, classes=None, k=None):
        """queries [N, T, 3, H, W] fp32 (device) -> what align_features gives for those clips' tower features"""
        if not isinstance(queries, torch.Tensor) or queries.dim() != 5:
            self.gallery._check_videos(queries, "queries")                    # raises
        p = self._plan(queries.shape[0], classes, k)
        return self._run(p, self.gallery._check_videos(queries, "queries"), True)
