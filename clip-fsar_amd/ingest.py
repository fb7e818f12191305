"""Frame ingest: a tick's worth of decoded uint8 clips, each of its own geometry, on the host or on the device -> the tower's packed input.

    fi = FrameIngest(device, test_scale=256, crop=224, mean=MEAN, std=STD)      # or FrameIngest.from_cfg(cfg, device)
    x = fi.transform([clip_a, clip_b, ...])       # clip_i: uint8 [n_i, H_i, W_i, 3] -> x: fp32 [sum n_i, 3, crop, crop] on the device
    pool.push_packed(x, sessions, [c.shape[0] for c in clips])                   # what StreamPool.push_u8_packed does
    gallery.classify(fi.transform(videos).view(N, T, 3, crop, crop))             # the galleries take the result as it is

The transform is clip_fsar_amd.preprocess.preprocess_video's (bilinear resize to DATA.TEST_SCALE, crop window of DATA.TEST_CROP_SIZE,
NormalizeVideo, [n, 3, crop, crop]) and a frame comes out with the same bits; what differs is the shape of the work.  All clips of a call
go through ONE descriptor table and ONE launch (libclipfsar_ingest.so, clip_fsar_amd.ingest_hip), and clips that lie in host memory are
uploaded as uint8 at source resolution on a COPY stream owned by the object, so the compute stream never carries an upload:

  * a ring of `depth` device staging buffers, grown on demand; the clips of a call are laid out in one of them by plan_ingest;
  * a pinned host clip is copied straight to its offset (the caller must leave it unchanged until fi.uploaded has completed -- the usual
    contract of a non_blocking copy); a pageable one goes through the buffer's pinned host twin; a device clip is copied on the compute
    stream (a single device clip is read where it lies);
  * the compute stream waits for the event behind the copies; the copy stream waits, before it rewrites a buffer, for the event recorded
    behind the kernel that last read it.  The caller never synchronises: the upload of call k + 1 runs under whatever consumes call k.

Every error of a call is raised before any copy or launch.
"""
from __future__ import annotations

import collections

import torch

from . import ingest_hip as ihp
from .preprocess import crop_window

ALIGN = 256              # staging offset of every group: a multiple of ingest_hip.SRC_ALIGN, and of the 64-byte sectors copies move
IngestPlan = collections.namedtuple("IngestPlan", "rows offsets total_bytes n_frames scale_hw crop")


def scale_hw(test_scale):
    """the reference's DATA.TEST_SCALE rule: an int is a square, [h, w] is that size"""
    if isinstance(test_scale, bool):
        raise ValueError("TEST_SCALE must be an int or [h, w], got %r" % (test_scale,))
    if isinstance(test_scale, int):
        return test_scale, test_scale
    if isinstance(test_scale, (list, tuple)) and len(test_scale) == 2 and all(isinstance(v, int) and not isinstance(v, bool) for v in test_scale):
        return int(test_scale[0]), int(test_scale[1])
    raise ValueError("TEST_SCALE must be an int or [h, w], got %r" % (test_scale,))


def plan_ingest(shapes, test_scale, crop, num_spatial_crops=1, idx=1, align=ALIGN):
    """The host plan of one transform call, a pure function.  shapes: (n, H, W) per group -> IngestPlan: the descriptor-table rows
    (ingest_hip's column order), the byte offset of every group in the staging buffer (multiples of `align`, groups in the order given,
    each n * H * W * 3 dense bytes), the bytes the buffer needs, the frames.  idx: the spatial-crop selection of preprocess.crop_window,
    one for all groups or one per group."""
    sh, sw = scale_hw(test_scale)
    crop = int(crop)
    if crop < 1 or sh < crop or sw < crop:
        raise ValueError("plan_ingest: the scale %d x %d must be at least the crop size %d >= 1" % (sh, sw, crop))
    if align < ihp.SRC_ALIGN or align % ihp.SRC_ALIGN:
        raise ValueError("plan_ingest: align must be a multiple of %d, got %r" % (ihp.SRC_ALIGN, align))
    shapes = [tuple(int(v) for v in s) for s in shapes]
    if not shapes:
        raise ValueError("plan_ingest: no groups")
    idxs = list(idx) if isinstance(idx, (list, tuple)) else [idx] * len(shapes)
    if len(idxs) != len(shapes):
        raise ValueError("plan_ingest: %d crop selections for %d groups" % (len(idxs), len(shapes)))
    rows, offsets, off, frames = [], [], 0, 0
    for (n, H, W), ix in zip(shapes, idxs):
        if n < 1 or H < 2 or W < 2:
            raise ValueError("plan_ingest: a group needs n >= 1 frames of H, W >= 2, got (n, H, W) = %r" % ((n, H, W),))
        y0, x0 = crop_window((sh, sw), crop, num_spatial_crops, ix)
        rows.append([off // ihp.SRC_ALIGN, n, frames, H, W, sh, sw, y0, x0])
        offsets.append(off)
        frames += n
        end = off + n * H * W * 3
        off = -(-end // align) * align
    if len(rows) > ihp.MAX_GROUPS or frames > 0x7fffffff or off // ihp.SRC_ALIGN > 0x7fffffff:
        raise ValueError("plan_ingest: %d groups, %d frames, %d bytes are too many for one call" % (len(rows), frames, end))
    return IngestPlan(rows, offsets, end, frames, (sh, sw), crop)


class _Slot:
    """one staging buffer: dev (device uint8), twin (its pinned host twin, made when a pageable clip first needs it), done (recorded on the
    compute stream behind the kernel that last read dev), uploaded (recorded on the copy stream behind the last copies into dev)"""
    __slots__ = ("dev", "twin", "done", "uploaded")

    def __init__(self):
        self.dev = self.twin = self.done = self.uploaded = None


class FrameIngest:
    def __init__(self, device, test_scale, crop, mean, std, depth=2, num_spatial_crops=1, idx=1):
        self.dev = torch.device(device)
        self.scale_hw = scale_hw(test_scale)
        if isinstance(crop, bool) or not isinstance(crop, int) or crop < 1:
            raise ValueError("FrameIngest: crop must be an integer >= 1, got %r" % (crop,))
        if min(self.scale_hw) < crop:
            raise ValueError("FrameIngest: the scale %d x %d is below the crop size %d" % (self.scale_hw + (crop,)))
        if isinstance(depth, bool) or not isinstance(depth, int) or depth < 1:
            raise ValueError("FrameIngest: depth must be an integer >= 1, got %r" % (depth,))
        self.crop, self.depth = crop, depth
        self.mean, self.std = tuple(float(v) for v in mean), tuple(float(v) for v in std)
        if len(self.mean) != 3 or len(self.std) != 3 or not all(self.std):
            raise ValueError("FrameIngest: mean and std must have 3 values, std none of them 0, got %r, %r" % (mean, std))
        self.num_spatial_crops, self.idx = num_spatial_crops, idx
        for ix in (idx if isinstance(idx, (list, tuple)) else [idx]):         # one selection for all clips of a call, or one per clip
            crop_window(self.scale_hw, crop, num_spatial_crops, ix)           # an unsupported selection raises here
        self._slots = [_Slot() for _ in range(depth)]
        self._next = 0
        self._copy_stream = None                 # made by the first call that uploads
        self._tables = None
        self._retired = []                       # (outgrown staging buffer, the event behind its last reader)
        self.uploaded = None                     # the event behind the last call's host-to-device copies (None: it had none)

    @classmethod
    def from_cfg(cls, cfg, device, depth=2):
        """DATA.TEST_SCALE, DATA.TEST_CROP_SIZE, DATA.MEAN, DATA.STD of a project config"""
        data = getattr(cfg, "DATA", None)
        missing = [k for k in ("TEST_SCALE", "TEST_CROP_SIZE", "MEAN", "STD") if not hasattr(data, k)]
        if missing:
            raise ValueError("FrameIngest.from_cfg: the config lacks DATA.%s -- set them, or build a FrameIngest yourself and pass it "
                             "as ingest=" % ", DATA.".join(missing))
        return cls(device, data.TEST_SCALE, int(data.TEST_CROP_SIZE), data.MEAN, data.STD, depth=depth)

    # ------------------------------------------------------------------ checks: everything a call can get wrong, before any device work
    def _on_device(self, t):
        return self.dev.type == "cuda" and (t.device.index == self.dev.index or (
            self.dev.index is None and t.device.index == torch.cuda.current_device()))

    def check(self, clips):
        """-> [(n, H, W)] of a list of uint8 [n, H, W, 3] clips, or the error transform(clips) would raise"""
        if not isinstance(clips, (list, tuple)) or not clips:
            raise ValueError("FrameIngest: a call takes a non-empty list of uint8 [n, H, W, 3] clips, got %s" % (
                "an empty one" if isinstance(clips, (list, tuple)) else type(clips).__name__))
        shapes = []
        for i, c in enumerate(clips):
            if not isinstance(c, torch.Tensor):
                raise TypeError("FrameIngest: clip %d is a %s, not a tensor" % (i, type(c).__name__))
            if c.dtype != torch.uint8:
                raise TypeError("FrameIngest: clip %d has dtype %s, the ingest takes uint8 frames (fp32 frames go to push / classify "
                                "directly)" % (i, c.dtype))
            if c.dim() != 4 or c.shape[3] != 3:
                raise ValueError("FrameIngest: clip %d must be [n, H, W, 3], got %s" % (i, tuple(c.shape)))
            n, H, W = (int(v) for v in c.shape[:3])
            if n < 1 or H < 2 or W < 2:
                raise ValueError("FrameIngest: clip %d needs n >= 1 frames of H, W >= 2, got %s" % (i, tuple(c.shape)))
            if c.is_cuda and not self._on_device(c):
                raise RuntimeError("FrameIngest: clip %d lives on %s, this ingest on %s" % (i, c.device, self.dev))
            shapes.append((n, H, W))
        return shapes

    # ------------------------------------------------------------------ the call
    def transform(self, clips):
        """clips: a list of uint8 [n_i, H_i, W_i, 3], each on this device, in pinned or in pageable host memory -> fp32
        [sum n_i, 3, crop, crop] on the device, clip after clip: one table upload and one launch on the current stream"""
        shapes = self.check(clips)
        plan = plan_ingest(shapes, self.scale_hw, self.crop, self.num_spatial_crops, self.idx)
        if self.dev.type != "cuda":
            raise RuntimeError("FrameIngest: built on %s -- the transform runs on a HIP device (no CPU path exists)" % self.dev)
        clips = [c if c.is_contiguous() else c.contiguous() for c in clips]
        with torch.cuda.device(self.dev):
            comp = torch.cuda.current_stream(self.dev)
            out = torch.empty(plan.n_frames, 3, self.crop, self.crop, device=self.dev, dtype=torch.float32)
            self.uploaded = None
            if len(clips) == 1 and clips[0].is_cuda:
                slot, src = None, clips[0]       # plan.offsets == [0]: read in place
            else:
                slot = self._stage(clips, plan, comp)
                src = slot.dev[:plan.total_bytes]
            try:
                if self._tables is None or self._tables.max_rows < len(plan.rows):
                    self._tables = ihp.table_uploader(self.dev, max(64, 2 * len(plan.rows)))
                ihp.transform_frames(src, out, self._tables.upload(plan.rows), self.crop, self.mean, self.std)
            finally:
                # also when the launch raised: the buffer holds this call's bytes, and whatever the compute stream has queued up to here
                # is all that may still read it -- an event of an earlier kernel must not stay behind as the guard of its next rewrite
                if slot is not None:
                    slot.done = torch.cuda.Event()
                    slot.done.record(comp)
        return out

    def serves(self, device, res=None, who="FrameIngest"):
        """raises unless this ingest lives on `device` and (res given) crops to the res x res frames the tower there takes"""
        other = torch.device(device)
        same = other.type == self.dev.type
        if same and other.index != self.dev.index:               # an index left out means the current device
            cur = torch.cuda.current_device()
            same = (cur if other.index is None else other.index) == (cur if self.dev.index is None else self.dev.index)
        if not same:
            raise ValueError("%s: the ingest lives on %s, the gallery on %s" % (who, self.dev, other))
        if res is not None and int(res) != self.crop:
            raise ValueError("%s: the ingest crops to %d x %d, the tower takes %d x %d frames (DATA.TEST_CROP_SIZE)" % (
                who, self.crop, self.crop, int(res), int(res)))

    def _stage(self, clips, plan, comp):
        """the clips into the next staging buffer at plan.offsets -> its slot; on return the compute stream waits for every copy"""
        slot = self._slots[self._next]
        self._next = (self._next + 1) % self.depth
        if self._copy_stream is None:
            self._copy_stream = torch.cuda.Stream(self.dev)
        cs = self._copy_stream
        self._retired = [(b, e) for b, e in self._retired if not e.query()]      # outgrown buffers whose last reader has finished
        if slot.dev is None or slot.dev.numel() < plan.total_bytes:
            if slot.dev is not None and slot.done is not None:
                # the outgrown buffer may still be read by the kernel in flight: keep it until that has finished instead of returning it
                # to the allocator with compute-stream ordering only (utils/prefetch.py does the same)
                self._retired.append((slot.dev, slot.done))
            size = max(plan.total_bytes, 0 if slot.dev is None else slot.dev.numel() * 3 // 2)
            slot.dev = torch.empty(-(-size // (1 << 20)) << 20, dtype=torch.uint8, device=self.dev)
            slot.dev.record_stream(cs)           # allocated on the compute stream, written on the copy stream
            cs.wait_stream(comp)                 # the block's previous owner may still have kernels queued there
            slot.done = None
        host = [k for k, c in enumerate(clips) if not c.is_cuda]
        pageable = [k for k in host if not clips[k].is_pinned()]
        if pageable:
            if slot.uploaded is not None:
                slot.uploaded.synchronize()      # the copies that last read the twin: issued `depth` calls ago, long completed
            if slot.twin is None or slot.twin.numel() < plan.total_bytes:
                slot.twin = torch.empty(slot.dev.numel(), dtype=torch.uint8).pin_memory()
        if host:
            runs = []                            # (first byte, last byte, source): a pinned clip, or a run of pageable ones in the twin
            for k in host:
                off, flat = plan.offsets[k], clips[k].view(-1)
                if k in pageable:
                    slot.twin[off:off + flat.numel()].copy_(flat)
                    if runs and runs[-1][2] is None and runs[-1][3] == k - 1:
                        runs[-1] = (runs[-1][0], off + flat.numel(), None, k)
                    else:
                        runs.append((off, off + flat.numel(), None, k))
                else:
                    runs.append((off, off + flat.numel(), flat, k))
            with torch.cuda.stream(cs):
                if slot.done is not None:
                    cs.wait_event(slot.done)     # the kernel that last read this buffer
                for b0, b1, flat, _ in runs:
                    slot.dev[b0:b1].copy_(slot.twin[b0:b1] if flat is None else flat, non_blocking=True)
                slot.uploaded = torch.cuda.Event()
                slot.uploaded.record(cs)
            comp.wait_event(slot.uploaded)
            self.uploaded = slot.uploaded
        if slot.done is not None:
            comp.wait_event(slot.done)           # nothing to wait for unless the caller changed streams between calls
        for k, c in enumerate(clips):
            if c.is_cuda:
                slot.dev[plan.offsets[k]:plan.offsets[k] + c.numel()].copy_(c.view(-1))
        return slot
