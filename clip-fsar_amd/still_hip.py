"""ctypes binding of libclipfsar_still.so (C ABI declared in include/ext/clipfsar_still.h): the still-frame gate of
clip_fsar_amd.pool.StreamPool(still=...) -- the change count of every frame of a pixel push against its predecessor, the packing of the
frames that go through the tower together with the update of the store of every session's newest frame, and the expansion of the kept
frames' tower rows to a row per frame.  The rule that turns counts into a keep pattern is clip_fsar_amd.still.plan_still, on the host.

A library and a signature table of their own, like clip_fsar_amd.pool_hip: contiguous HIP device tensors only (no CPU path), launches on
the current stream of the operands' device, a non-zero return code raises with the library's message.  The descriptor table (four
columns: SLOT, F0, N, LAST_POS) and the index lists `kept` and `src` travel twice, as the pool's table does: the library validates the
host copy and the kernels read the device copy.  pool_hip.TableUploader(cols=TABLE_COLS) uploads the table, ListUploader the lists.
"""
from __future__ import annotations

import collections
import ctypes
import os

import torch  # noqa: F401  (imported first so that torch's HIP runtime is the one the library binds to)

from . import _cabi, hip

ABI_VERSION = 1          # CFSK_ABI_VERSION of include/ext/clipfsar_still.h this file's SIGNATURES were written against
LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libclipfsar_still.so")
MAX_STREAMS = 65536      # CFSK_MAX_STREAMS
CHUNK = 8192             # CFSK_CHUNK: elements of a frame per workgroup and item
MAX_L = (1 << 31) - 1    # elements of a frame: indexed with 32 bits
TABLE_COLS = 4           # CFSK_TABLE_COLS; the columns, in order:
SLOT, F0, N, LAST_POS = range(TABLE_COLS)
_lib = None

_c_int, _c_p, _c_ll, _c_f = ctypes.c_int, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_float

# symbol -> argtypes; must match include/ext/clipfsar_still.h (tests/test_still_abi.py cross-checks against the header text)
SIGNATURES = {
    "cfsk_version": [],
    "cfsk_abi_version": [],
    "cfsk_workspace_ints": [_c_int, _c_ll],
    "cfsk_changed": [_c_p] * 6 + [_c_int, _c_int, _c_ll, _c_int, _c_f, _c_p],
    "cfsk_pack": [_c_p] * 5 + [_c_int, _c_p, _c_p, _c_int, _c_int, _c_ll, _c_int, _c_p],
    "cfsk_expand": [_c_p] * 5 + [_c_int, _c_p, _c_p] + [_c_int] * 5 + [_c_p],
}


def lib():
    """Load (once) and return the ctypes handle.  Raises when the library is not built."""
    global _lib
    if _lib is None:
        _lib = _cabi.load(LIB_PATH, SIGNATURES, "cfsk_", ABI_VERSION, "the still-frame gate")
    return _lib


_check = _cabi.checker(lib, "cfsk_")
_shape = _cabi.shape_checker("still_hip")
_dev, _stream = hip._dev, hip._stream

Table = _cabi.Table
List = collections.namedtuple("List", "host dev n")            # host: pinned [n] int32; dev: its device copy


class ListUploader:
    """upload(values) -> List: the int32 values in a pinned host buffer and their device copy, enqueued on the current stream.  `depth`
    buffer pairs are used in turn and grow on demand; before a pair is rewritten the event recorded after its last copy is waited for
    (pool_hip.TableUploader's scheme: the host never waits for the device in steady state)."""

    def __init__(self, device, depth=4):
        self.dev, self.depth = torch.device(device), int(depth)
        self._host, self._devbuf, self._events = [None] * self.depth, [None] * self.depth, [None] * self.depth
        self._next = 0

    def upload(self, values):
        n = len(values)
        i = self._next
        self._next = (i + 1) % self.depth
        if self._events[i] is not None:
            self._events[i].synchronize()
        if self._host[i] is None or self._host[i].shape[0] < n:
            room = max(64, 2 * n)
            self._host[i] = torch.empty(room, dtype=torch.int32).pin_memory()
            self._devbuf[i] = torch.empty(room, dtype=torch.int32, device=self.dev)
        host, dev = self._host[i][:n], self._devbuf[i][:n]
        if n:
            host.copy_(torch.tensor(values, dtype=torch.int32))
            with torch.cuda.device(self.dev):
                dev.copy_(host, non_blocking=True)
                ev = self._events[i] or torch.cuda.Event()
                ev.record()
            self._events[i] = ev
        return List(host, dev, n)


def _table(t):
    return _cabi.table_args(t, TABLE_COLS, "still_hip")


def _list(l, n, name):
    """(host pointer, device pointer) of a List of n values"""
    if not isinstance(l, List) or l.n != n or l.host.is_cuda or l.host.dtype != torch.int32 or tuple(l.host.shape) != (n,) \
            or tuple(l.dev.shape) != (n,):
        raise RuntimeError("clip_fsar_amd.still_hip: %s must be a List of %d int32 host values and their device copy" % (name, n))
    return ctypes.c_void_p(l.host.data_ptr()), _dev(l.dev, torch.int32, name)


def workspace_ints(n_frames, L):
    """int32 values of the `work` buffer changed() needs for n_frames frames of L elements"""
    n = lib().cfsk_workspace_ints(int(n_frames), int(L))
    if n < 0:
        raise RuntimeError("clip_fsar_amd.still_hip: no workspace for N=%d frames of L=%d elements" % (n_frames, L))
    return n


def changed(frames, prev, counts, work, table, tol):
    """frames [N, L], prev [max_streams, L] fp32 -> counts [N] int32: per frame the number of elements that differ from its predecessor's
    by more than tol (clip_fsar_amd.still.reference_changed restates it), -1 for a frame without one.  work: int32, at least
    workspace_ints(N, L) values.  Two launches."""
    n, L = frames.shape
    _shape(prev, (prev.shape[0], L), "prev")
    _shape(counts, (n,), "counts")
    if work.dim() != 1 or work.numel() < workspace_ints(n, L):
        raise RuntimeError("clip_fsar_amd.still_hip: work has shape %s, expected at least [%d]" % (tuple(work.shape), workspace_ints(n, L)))
    th, td, S = _table(table)
    _check(lib().cfsk_changed(_dev(frames, torch.float32, "frames"), _dev(prev, torch.float32, "prev"), _dev(counts, torch.int32, "counts"),
                              _dev(work, torch.int32, "work"), th, td, S, n, L, prev.shape[0], float(tol), _stream()), "cfsk_changed")


def pack(frames, packed, prev, kept, table):
    """packed[r] = frames[kept[r]] for the NK = kept.n kept frames, and prev[SLOT_s] = frames[F0_s + N_s - 1] for every table row, in one
    launch.  With NK == 0 or NK == N nothing is packed and `packed` may be None (kept still says which of the two: a List of 0 or of N
    values)."""
    n, L = frames.shape
    _shape(prev, (prev.shape[0], L), "prev")
    NK = kept.n if isinstance(kept, List) else -1
    if 0 < NK < n:
        _shape(packed, (NK, L), "packed")
        kh, kd = _list(kept, NK, "kept")
        pk = _dev(packed, torch.float32, "packed")
    else:
        kh = kd = pk = None
    th, td, S = _table(table)
    _check(lib().cfsk_pack(_dev(frames, torch.float32, "frames"), pk, _dev(prev, torch.float32, "prev"), kh, kd, NK, th, td, S, n, L,
                           prev.shape[0], _stream()), "cfsk_pack")


def expand(kept_feats, ring, feats, src, table):
    """feats[i] = kept_feats[src[i]] when src[i] >= 0, the ring row of the session's newest frame before the push (ring[SLOT_s,
    LAST_POS_s]) otherwise.  kept_feats [NK, E] (None when NK == 0), ring [max_streams, cap, E], feats [N, E].  One launch."""
    n, E = feats.shape
    M, cap = ring.shape[0], ring.shape[1]
    _shape(ring, (M, cap, E), "ring")
    NK = 0 if kept_feats is None else kept_feats.shape[0]
    if kept_feats is not None:
        _shape(kept_feats, (NK, E), "kept_feats")
    sh, sd = _list(src, n, "src")
    th, td, S = _table(table)
    _check(lib().cfsk_expand(None if kept_feats is None else _dev(kept_feats, torch.float32, "kept_feats"), _dev(ring, torch.float32, "ring"),
                             _dev(feats, torch.float32, "feats"), sh, sd, NK, th, td, S, n, E, M, cap, _stream()), "cfsk_expand")
