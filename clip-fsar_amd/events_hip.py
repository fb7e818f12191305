"""ctypes binding of libclipfsar_events.so (C ABI declared in include/ext/clipfsar_events.h): the onset / offset detector of
clip_fsar_amd.pool.StreamPool(events=EventRule(...)), a hysteresis machine per (session slot, class store slot) whose state is guarded by
the store slots' generations as clip_fsar_amd.class_smooth_hip's is.

A library and a signature table of their own, like clip_fsar_amd.class_smooth_hip: contiguous HIP device tensors only (no CPU path),
launches on the current stream of the operands' device, a non-zero return code raises with the library's message.  The descriptor table
is class_smooth_hip's -- the same six columns, planned by class_smooth_hip.plan_rows, uploaded by its table_uploader -- and so are the
key lists: a pool that smooths by class and detects events plans and uploads once per push.
"""
from __future__ import annotations

import ctypes
import os

import torch  # noqa: F401  (imported first so that torch's HIP runtime is the one the library binds to)

from . import _cabi, hip
from .class_smooth_hip import plan_rows, table_uploader  # noqa: F401  (one planner and one table layout for both libraries)

ABI_VERSION = 1          # CFEV_ABI_VERSION of include/ext/clipfsar_events.h this file's SIGNATURES were written against
LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libclipfsar_events.so")
MAX_STREAMS = 65536      # CFEV_MAX_STREAMS
CHUNK = 256              # CFEV_CHUNK: columns per workgroup
MAX_CELLS = (1 << 31) - 1            # max_streams * cap: the kernels' cell index has 32 bits
TABLE_COLS = 6           # CFEV_TABLE_COLS; the columns, in order:
SLOT, NW, OUT0, NC, KEY0, CHUNK0 = range(TABLE_COLS)
ONSET, OFFSET = 1, 2     # CFEV_ONSET, CFEV_OFFSET: a record's kind
EVENT_COLS, VALUE_COLS = 5, 2        # events [max_events, 5] int32: row, column, window, kind, len; values [max_events, 2] fp32: score, peak
_lib = None

_c_int, _c_p, _c_f = ctypes.c_int, ctypes.c_void_p, ctypes.c_float

# symbol -> argtypes; must match include/ext/clipfsar_events.h (tests/test_events_abi.py cross-checks against the header text)
SIGNATURES = {
    "cfev_version": [],
    "cfev_abi_version": [],
    "cfev_workspace_ints": [_c_int],
    "cfev_detect": [_c_p] * 13 + [_c_int] * 5 + [_c_f, _c_f] + [_c_int] * 3 + [_c_p],
}


def lib():
    """Load (once) and return the ctypes handle.  Raises when the library is not built."""
    global _lib
    if _lib is None:
        _lib = _cabi.load(LIB_PATH, SIGNATURES, "cfev_", ABI_VERSION, "stream events")
    return _lib


_check = _cabi.checker(lib, "cfev_")
_shape = _cabi.shape_checker("events_hip")
_dev, _stream = hip._dev, hip._stream

Table = _cabi.Table


def workspace_ints(n_chunks):
    """int32 elements of detect's `work` for a table of n_chunks workgroups (the plan's n_chunks)"""
    n = lib().cfev_workspace_ints(int(n_chunks))
    if n < 0:
        raise RuntimeError("clip_fsar_amd.events_hip: no workspace for n_chunks=%r (below 1, or 2^31 ints and more)" % (n_chunks,))
    return n


def detect(scores, streak, length, peak, marks, gens, keys, events, values, n_events, work, table, on, off, min_on, min_off):
    """scores [NOUT] flat (row i of the table owns a row-major [NW, NC] block at OUT0), streak / length / marks [max_streams, cap] int32,
    peak [max_streams, cap] fp32, gens [cap] int32, keys [NKEYS] int32 -> events [max_events, 5] int32 and values [max_events, 2] fp32,
    the records in the order (row, column, window), and n_events [1] int32, their true number (records beyond max_events are dropped);
    the cells advance and their marks receive the generations.  work: int32, at least workspace_ints(n_chunks), n_chunks the table's
    sum of ceil(NC / CHUNK) (the plan's n_chunks).  NOUT == 0: nothing is launched and n_events is zeroed here.  Three launches."""
    M, cap = streak.shape
    for t, name in ((length, "length"), (peak, "peak"), (marks, "marks")):
        _shape(t, (M, cap), name)
    _shape(gens, (cap,), "gens")
    _shape(n_events, (1,), "n_events")
    if scores.dim() != 1 or keys.dim() != 1 or work.dim() != 1:
        raise RuntimeError("clip_fsar_amd.events_hip: scores, keys and work must be flat, got %s, %s and %s" % (
            tuple(scores.shape), tuple(keys.shape), tuple(work.shape)))
    if events.dim() != 2 or events.shape[1] != EVENT_COLS or events.shape[0] < 1:
        raise RuntimeError("clip_fsar_amd.events_hip: events has shape %s, expected [max_events >= 1, %d]" % (tuple(events.shape), EVENT_COLS))
    _shape(values, (events.shape[0], VALUE_COLS), "values")
    host = getattr(table, "host", None)            # the workspace against the host rows, before any pointer is taken (table_args checks the
    if isinstance(host, torch.Tensor) and host.dim() == 2 and host.shape[1] == TABLE_COLS and host.shape[0]:       # table itself below)
        n_chunks = int(((host[:, NC].clamp(min=0) + (CHUNK - 1)) // CHUNK).sum())
        if n_chunks >= 1 and work.shape[0] < workspace_ints(n_chunks):
            raise RuntimeError("clip_fsar_amd.events_hip: work holds %d ints, the table's %d workgroups need %d" % (
                work.shape[0], n_chunks, workspace_ints(n_chunks)))
    th, td, S = _cabi.table_args(table, TABLE_COLS, "events_hip")
    x = _dev(scores, torch.float32, "scores")
    if scores.shape[0] == 0:                       # no windows at all: an empty tensor has no address; the table is still validated, and
        x = _dev(peak, torch.float32, "peak")      # nothing is launched, so the stand-in is never dereferenced
        n_events.zero_()
    _check(lib().cfev_detect(x, _dev(streak, torch.int32, "streak"), _dev(length, torch.int32, "length"), _dev(peak, torch.float32, "peak"),
                             _dev(marks, torch.int32, "marks"), _dev(gens, torch.int32, "gens"), _dev(keys, torch.int32, "keys"),
                             _dev(events, torch.int32, "events"), _dev(values, torch.float32, "values"),
                             _dev(n_events, torch.int32, "n_events"), _dev(work, torch.int32, "work"), th, td, S, scores.shape[0],
                             keys.shape[0], M, cap, float(on), float(off), int(min_on), int(min_off), events.shape[0], _stream()),
           "cfev_detect")
