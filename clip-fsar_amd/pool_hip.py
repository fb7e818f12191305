"""ctypes binding of libclipfsar_pool.so (C ABI declared in include/clipfsar_pool.h): the ring, gather and smoothing kernels of
clip_fsar_amd.pool.StreamPool, which take a per-session descriptor table instead of stream_hip's one (B, n, first_frame) triple.

A library and a signature table of their own, like clip_fsar_amd.stream_hip: contiguous HIP device tensors only (no CPU path), launches on
the current stream of the operands' device, a non-zero return code raises with the library's message.

The table travels twice (include/clipfsar_pool.h): the library validates the host rows and the kernels read the device copy.  TableUploader
makes both: a small ring of pinned host buffers, each paired with a device buffer and guarded by an event recorded after its asynchronous
copy, so a buffer is rewritten only once the copy that read it has completed and the host never waits for the device in steady state.
"""
from __future__ import annotations

import ctypes
import os

import torch  # noqa: F401  (imported first so that torch's HIP runtime is the one the library binds to)

from . import _cabi, hip

ABI_VERSION = 1          # CFSP_ABI_VERSION of include/clipfsar_pool.h this file's SIGNATURES were written against
LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libclipfsar_pool.so")
MAX_T = 32               # CFSP_MAX_T
MAX_STREAMS = 65536      # CFSP_MAX_STREAMS
TABLE_COLS = 8           # CFSP_TABLE_COLS; the columns, in order:
SLOT, PUT_POS, N, FEAT_OFF, WIN_POS, NW, WIN_OFF, HAS_STATE = range(TABLE_COLS)
_lib = None

_c_int, _c_p, _c_f = ctypes.c_int, ctypes.c_void_p, ctypes.c_float

# symbol -> argtypes; must match include/clipfsar_pool.h (tests/test_build_recipe.py cross-checks against the header text)
SIGNATURES = {
    "cfsp_version": [],
    "cfsp_abi_version": [],
    "cfsp_ring_put": [_c_p] * 4 + [_c_int] * 5 + [_c_p],
    "cfsp_window_sequences": [_c_p] * 4 + [_c_int] * 10 + [_c_p],
    "cfsp_smooth_logits": [_c_p] * 5 + [_c_int] * 4 + [_c_f, _c_p],
}


def lib():
    """Load (once) and return the ctypes handle.  Raises when the library is not built."""
    global _lib
    if _lib is None:
        _lib = _cabi.load(LIB_PATH, SIGNATURES, "cfsp_", ABI_VERSION, "stream pools")
    return _lib


_check = _cabi.checker(lib, "cfsp_")
_shape = _cabi.shape_checker("pool_hip")
_dev, _stream = hip._dev, hip._stream

Table = _cabi.Table


class TableUploader:
    """upload(rows) -> Table: the rows in a pinned host buffer and their device copy, enqueued on the current stream.  `depth` buffer pairs
    are used in turn; before a pair is rewritten the event recorded after its last copy is waited for (it has long completed unless the
    host runs `depth` uploads ahead of the device).  `cols`: values per row (clip_fsar_amd.ingest_hip uploads its own table layout)."""

    def __init__(self, device, max_rows, depth=4, cols=TABLE_COLS):
        self.dev, self.max_rows, self.depth, self.cols = torch.device(device), int(max_rows), int(depth), int(cols)
        self._host = self._devbuf = self._events = None
        self._next = 0

    def upload(self, rows):
        S = len(rows)
        if not 1 <= S <= self.max_rows or any(len(r) != self.cols for r in rows):
            raise RuntimeError("clip_fsar_amd.pool_hip: a table must have 1 .. %d rows of %d values, got %d rows" % (
                self.max_rows, self.cols, S))
        if self._host is None:
            self._host = [torch.empty(self.max_rows, self.cols, dtype=torch.int32).pin_memory() for _ in range(self.depth)]
            self._devbuf = torch.empty(self.depth, self.max_rows, self.cols, dtype=torch.int32, device=self.dev)
            self._events = [None] * self.depth
        i = self._next
        self._next = (i + 1) % self.depth
        if self._events[i] is not None:
            self._events[i].synchronize()
        host = self._host[i][:S]
        host.copy_(torch.tensor(rows, dtype=torch.int32))
        dev = self._devbuf[i, :S]
        with torch.cuda.device(self.dev):
            dev.copy_(host, non_blocking=True)
            ev = self._events[i] or torch.cuda.Event()
            ev.record()
        self._events[i] = ev
        return Table(host, dev, S)


def _table(t):
    return _cabi.table_args(t, TABLE_COLS, "pool_hip")


def ring_put(feats, ring, table):
    """feats [N, E] packed session-major -> ring [max_streams, cap, E]: ring[slot, (put_pos + i) mod cap] = feats[feat_off + i] per row"""
    N, E = feats.shape
    _shape(ring, (ring.shape[0], ring.shape[1], E), "ring")
    th, td, S = _table(table)
    _check(lib().cfsp_ring_put(_dev(feats, torch.float32, "feats"), _dev(ring, torch.float32, "ring"), th, td, S, N, E, ring.shape[0],
                               ring.shape[1], _stream()), "cfsp_ring_put")


def window_sequences(ring, X, table, n_windows, w0, w1, T, stride, rate):
    """ring [max_streams, cap, E] -> X [w1 - w0, T, E] (at least: a larger X is written in its first rows): the windows w0 .. w1 - 1 of
    the table's packed window list of n_windows windows"""
    M, cap, E = ring.shape
    if X.dim() != 3 or X.shape[0] < w1 - w0 or tuple(X.shape[1:]) != (T, E):
        raise RuntimeError("clip_fsar_amd.pool_hip: X has shape %s, expected [>= %d, %d, %d]" % (tuple(X.shape), w1 - w0, T, E))
    th, td, S = _table(table)
    _check(lib().cfsp_window_sequences(_dev(ring, torch.float32, "ring"), _dev(X, torch.float32, "X"), th, td, S, int(n_windows), int(w0),
                                       int(w1), int(T), E, M, cap, int(stride), int(rate), _stream()), "cfsp_window_sequences")


def smooth_logits(logits, state, out, table, alpha):
    """logits [NW, C] packed as the table's window list, state [max_streams, C] by slot -> out [NW, C]: per session y_0 = x_0 (or the
    recurrence from state[slot] when the row's has_state is 1), y_k = fmaf(alpha, y_{k-1}, (1 - alpha) * x_k).  out may be logits."""
    NW_, C = logits.shape
    _shape(state, (state.shape[0], C), "state")
    _shape(out, (NW_, C), "out")
    th, td, S = _table(table)
    _check(lib().cfsp_smooth_logits(_dev(logits, torch.float32, "logits"), _dev(state, torch.float32, "state"),
                                    _dev(out, torch.float32, "out"), th, td, S, NW_, C, state.shape[0], float(alpha), _stream()),
           "cfsp_smooth_logits")
