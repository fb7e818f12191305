"""Window streams: sliding-window classification of continuous frame streams against a gallery.

    s = WindowStream(gallery, n_streams=4, stride=2, rate=1, max_push=64, smooth=0.0)   # gallery: SupportGallery or TextGallery
    out = s.push(frames)               # frames [B, n, 3, H, W] fp32 on the device, any n >= 1
    out.first_window, out.logits       # k of the first window this push completed; [B, nW, C] fp32 (nW may be 0); out.smoothed or None
    values, index = s.topk(out, k=5)
    out = s.push_features(feats)       # feats [B, n, E] fp32: tower features computed elsewhere
    out = s.push_u8(frames_u8)         # decoded uint8 [B, n, H, W, 3] on the host or the device: clip_fsar_amd.ingest.FrameIngest, then push
    s.reset(); s.stats

In the eval branch the tower is per frame (few_shot.py:971-999, get_feats): nothing mixes frames before context2, so a frame's tower
features are the same in every window that holds it.  gallery.classify on overlapping windows runs the tower T / stride times per frame;
a WindowStream runs it once, keeps the features of the last (T-1) * rate + max_push frames of every stream in a device ring, gathers the
windows a push completes (libclipfsar_stream.so, clip_fsar_amd.stream_hip) and scores them with gallery.classify_features -- context2 and
the gallery kernels, in the gallery's own mode.

Streams advance in lockstep; frames are numbered t = 0, 1, ... from construction or the last reset().  Window k >= 0 holds frames
k * stride + j * rate, j = 0 .. T-1 (T = the gallery's DATA.NUM_INPUT_FRAMES), and is emitted once, by the push that delivers its last
frame.  A window's logits are what gallery.classify returns for the clip made of those frames; columns are in gallery.class_ids order.
Classes may be added to the gallery between pushes.  Optional smoothing over a stream's consecutive windows: y_0 = x_0,
y_k = fmaf(alpha, y_{k-1}, (1 - alpha) * x_k), carried across pushes.
"""
from __future__ import annotations

import collections

import torch

from . import gallery_hip as ghip
from . import stream_hip as shp
from .gallery import _GalleryBase
from .ingest import FrameIngest

StreamOutput = collections.namedtuple("StreamOutput", "first_window logits smoothed")


def window_plan(frames_before, n, T, stride, rate):
    """(first_window, n_windows) of the windows completed by pushing frames frames_before .. frames_before + n - 1: the k whose last
    frame k * stride + (T-1) * rate lies in that range.  first_window is also the number of windows completed before this push."""
    if frames_before < 0 or n < 0 or T < 1 or stride < 1 or rate < 1:
        raise ValueError("window_plan: need frames_before >= 0, n >= 0, T >= 1, stride >= 1, rate >= 1, got %r" % (
            (frames_before, n, T, stride, rate),))
    span = (T - 1) * rate

    def completed(frames):                      # windows whose last frame is below `frames`
        return 0 if frames <= span else (frames - 1 - span) // stride + 1

    first = completed(frames_before)
    return first, completed(frames_before + n) - first


class WindowStream:
    def __init__(self, gallery, n_streams=1, stride=1, rate=1, max_push=64, smooth=0.0, ingest=None):
        if not isinstance(gallery, _GalleryBase):
            raise TypeError("WindowStream: gallery must be a SupportGallery or a TextGallery, got %s" % type(gallery).__name__)
        for name, v in (("n_streams", n_streams), ("stride", stride), ("rate", rate), ("max_push", max_push)):
            if isinstance(v, bool) or not isinstance(v, int) or v < 1:
                raise ValueError("WindowStream: %s must be an integer >= 1, got %r" % (name, v))
        smooth = float(smooth)
        if not 0.0 <= smooth < 1.0:
            raise ValueError("WindowStream: smooth must be in [0, 1), got %r" % smooth)
        if gallery.T > shp.MAX_T:
            raise ValueError("WindowStream: T = %d frames per window, the stream library gathers at most %d" % (gallery.T, shp.MAX_T))
        self.gallery = gallery
        self.dev = gallery.dev
        self.B, self.stride, self.rate, self.max_push, self.alpha = n_streams, stride, rate, max_push, smooth
        self.T, self.E = gallery.T, gallery.E
        self.cap = (self.T - 1) * rate + max_push
        self._ring = torch.empty(self.B, self.cap, self.E, device=self.dev, dtype=torch.float32)
        self._X = None                           # gathered windows [rows, T, E], grown on demand
        if ingest is not None and not isinstance(ingest, FrameIngest):
            raise TypeError("WindowStream: ingest must be a FrameIngest, got %s" % type(ingest).__name__)
        if ingest is not None:
            ingest.serves(self.dev, who="WindowStream")
        self._ingest = ingest                    # push_u8's transform; None: built from gallery.head.args by the first push_u8
        self.reset()

    def reset(self):
        """Frame counter 0; the ring's contents and the smoothing state are dropped."""
        self._t = 0
        self._tower_frames = 0
        self._state = None                       # smoothing state [B, C]
        self._state_layout = None                # the gallery's layout_version when it was made (None: a gallery without one)

    @property
    def stats(self):
        return {"frames": self._t, "tower_frames": self._tower_frames,
                "windows": window_plan(0, self._t, self.T, self.stride, self.rate)[1]}

    # ------------------------------------------------------------------ pushes
    def _ready(self):
        g = self.gallery
        eng = g._fresh_engine()
        if not len(g):
            raise RuntimeError("%s: no classes registered" % g._name)
        return eng

    def _check(self, t, tail, what, layout):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise RuntimeError("WindowStream: %s must be a HIP device tensor (no CPU path exists)" % what)
        if t.dim() != 2 + len(tail) or t.shape[0] != self.B or t.shape[1] < 1 or any(
                want is not None and got != want for got, want in zip(t.shape[2:], tail)):
            raise ValueError("WindowStream: %s must be %s with B = %d, n >= 1, got %s" % (what, layout, self.B, tuple(t.shape)))
        return t.to(dtype=torch.float32)

    def push(self, frames):
        """frames [B, n, 3, H, W] fp32 (device): the next n frames of every stream -> StreamOutput of the windows they complete.  The
        tower runs once per frame."""
        eng = self._ready()
        frames = self._check(frames, (3, None, None), "frames", "[B, n, 3, H, W]")
        return self._pieces(eng, frames, tower=True)

    def push_features(self, feats):
        """feats [B, n, E] fp32 (device): the tower features of the next n frames of every stream -> as push"""
        eng = self._ready()
        feats = self._check(feats, (self.E,), "feats", "[B, n, E=%d]" % self.E)
        return self._pieces(eng, feats, tower=False)

    @property
    def ingest(self):
        """the FrameIngest of push_u8: the constructor's, or one built here from gallery.head.args (DATA.TEST_SCALE, TEST_CROP_SIZE, MEAN, STD)"""
        if self._ingest is None:
            self._ingest = FrameIngest.from_cfg(self.gallery.head.args, self.dev)
        return self._ingest

    def push_u8(self, frames):
        """frames uint8 [B, n, H, W, 3], on the device, in pinned or in pageable host memory: the next n decoded frames of every stream ->
        as push.  One FrameIngest.transform over all of them (one group), then push on its result; errors are raised before the upload."""
        eng = self._ready()
        ingest = self.ingest
        ingest.serves(self.dev, getattr(eng, "arch", {}).get("res"), "WindowStream")
        if not isinstance(frames, torch.Tensor) or frames.dim() != 5 or frames.shape[0] != self.B or frames.shape[1] < 1:
            raise ValueError("WindowStream: frames must be uint8 [B, n, H, W, 3] with B = %d, n >= 1, got %s" % (
                self.B, tuple(frames.shape) if isinstance(frames, torch.Tensor) else type(frames).__name__))
        B, n = frames.shape[:2]
        clip = frames.reshape(B * n, *frames.shape[2:])
        ingest.check([clip])
        return self.push(ingest.transform([clip]).view(B, n, 3, ingest.crop, ingest.crop))

    def _pieces(self, eng, src, tower):
        """pushes of at most max_push frames; the result is their concatenation"""
        n = src.shape[1]
        first = window_plan(self._t, 0, self.T, self.stride, self.rate)[0]
        outs = []
        for p0 in range(0, n, self.max_push):
            piece = src[:, p0:min(n, p0 + self.max_push)]
            outs.append(self._push_piece(eng, self._tower(eng, piece) if tower else piece.contiguous()))
        logits = outs[0][0] if len(outs) == 1 else torch.cat([o[0] for o in outs], 1)
        smoothed = None
        if self.alpha:
            smoothed = outs[0][1] if len(outs) == 1 else torch.cat([o[1] for o in outs], 1)
        return StreamOutput(first, logits, smoothed)

    def _tower(self, eng, frames):
        """frames [B, n, 3, H, W] -> [B, n, E]: engine.vit.forward on [B * n, 3, H, W], in chunks of engine.max_frames frames"""
        B, n = frames.shape[:2]
        flat = frames.reshape(B * n, *frames.shape[2:]).contiguous()
        feats = torch.empty(B, n, self.E, device=self.dev, dtype=torch.float32)
        out2d = feats.view(B * n, self.E)
        for f0 in range(0, B * n, eng.max_frames):
            f1 = min(B * n, f0 + eng.max_frames)
            eng.vit.forward(flat[f0:f1], out2d[f0:f1])
        self._tower_frames += B * n
        return feats

    def _push_piece(self, eng, feats):
        """feats [B, n <= max_push, E] into the ring; (logits, smoothed or None) [B, nW, C] of the windows that completes"""
        g, B, T = self.gallery, self.B, self.T
        n = feats.shape[1]
        C = len(g)
        if self.alpha and self._state is not None and self._state.shape[1] != C:
            raise RuntimeError("WindowStream: the gallery has %d classes, the smoothing state %d -- reset() the stream after adding "
                               "classes when smoothing is on" % (C, self._state.shape[1]))
        if self.alpha and self._state is not None and self._state_layout != getattr(g, "layout_version", None):
            raise RuntimeError("WindowStream: classes were removed from the gallery since the smoothing state was made, its columns mean "
                               "other classes now -- reset() the stream after removing classes when smoothing is on")
        first, nW = window_plan(self._t, n, T, self.stride, self.rate)
        shp.ring_put(feats, self._ring, self._t)
        self._t += n
        logits = torch.empty(B, nW, C, device=self.dev, dtype=torch.float32)
        if nW == 0:
            return logits, (logits if self.alpha else None)
        # classify_features scores max_frames // T clips per chunk: gather whole windows of all streams up to that many rows at a time
        per = max(1, max(1, eng.max_frames // T) // B)
        rows = B * min(nW, per)
        if self._X is None or self._X.shape[0] < rows:
            self._X = torch.empty(rows, T, self.E, device=self.dev, dtype=torch.float32)
        for w0 in range(0, nW, per):
            w1 = min(nW, w0 + per)
            X = self._X[:B * (w1 - w0)]
            shp.window_sequences(self._ring, X, w1 - w0, T, self.stride, self.rate, first + w0, self._t)
            logits[:, w0:w1].copy_(g.classify_features(X).view(B, w1 - w0, C))
        if not self.alpha:
            return logits, None
        if self._state is None:
            self._state = torch.empty(B, C, device=self.dev, dtype=torch.float32)
            self._state_layout = getattr(g, "layout_version", None)
        smoothed = torch.empty_like(logits)
        shp.smooth_logits(logits, self._state, smoothed, self.alpha, first)
        return logits, smoothed

    # ------------------------------------------------------------------ top-k
    def topk(self, out, k=5, smoothed=False):
        """(values [B, nW, k] fp32 descending, class index [B, nW, k] int32 into gallery.class_ids) of every window of a push's output
        (of out.smoothed with smoothed=True); ties go to the lower index"""
        src = out.smoothed if smoothed else out.logits
        if src is None:
            raise ValueError("WindowStream.topk: this output has no smoothed scores (smooth = 0)")
        B, nW, C = src.shape
        if not 1 <= k <= min(ghip.TOPK_MAX, max(1, C)):
            raise ValueError("WindowStream.topk: k must be in [1, min(16, number of classes)], got %d" % k)
        values = torch.empty(B, nW, k, device=src.device, dtype=torch.float32)
        index = torch.empty(B, nW, k, device=src.device, dtype=torch.int32)
        if nW:
            ghip.topk(src.reshape(B * nW, C), k, values.view(B * nW, k), index.view(B * nW, k))
        return values, index
