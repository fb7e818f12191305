"""ctypes binding of libclipfsar_timeline.so (C ABI declared in include/ext/clipfsar_timeline.h): the timeline of
clip_fsar_amd.pool.StreamPool(timeline=Timeline(...)) -- every push's class scores folded into buckets of windows, a peak, its window
and a count above a level per (session slot, bucket, class store slot), guarded by the store slots' generations as
clip_fsar_amd.baseline_hip's cells are -- and the read of a range of buckets (clip_fsar_amd.timeline states the rule).

A library and a signature table of their own, like clip_fsar_amd.baseline_hip: contiguous HIP device tensors only (no CPU path), launches
on the current stream of the operands' device, a non-zero return code raises with the library's message.  The fold's descriptor table
is class_smooth_hip's -- the same six columns, planned by class_smooth_hip.plan_rows -- and so are the key lists: a pool that smooths by
class, keeps baselines, detects events and keeps a timeline plans and uploads once per push.  The read's table has seven columns
(clip_fsar_amd.timeline.read_rows) and is uploaded by pool_hip.TableUploader at that width.
"""
from __future__ import annotations

import ctypes
import os

import torch  # noqa: F401  (imported first so that torch's HIP runtime is the one the library binds to)

from . import _cabi, hip
from .class_smooth_hip import plan_rows  # noqa: F401  (one planner and one table layout for the libraries over it)
from .pool_hip import TableUploader

ABI_VERSION = 1          # CFTL_ABI_VERSION of include/ext/clipfsar_timeline.h this file's SIGNATURES were written against
LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libclipfsar_timeline.so")
MAX_STREAMS = 65536      # CFTL_MAX_STREAMS
CHUNK = 256              # CFTL_CHUNK: columns per workgroup
MAX_CELLS = (1 << 31) - 1            # max_streams * B * cap: the kernels' cell index has 32 bits
MAX_SPAN = 1 << 20       # CFTL_MAX_SPAN
MAX_BUCKETS = 1 << 16    # CFTL_MAX_BUCKETS
TABLE_COLS = 6           # CFTL_TABLE_COLS; the fold's columns, in order:
SLOT, NW, OUT0, NC, KEY0, CHUNK0 = range(TABLE_COLS)
READ_COLS = 7            # CFTL_READ_COLS; the read's columns, in order:
R_SLOT, R_B0, R_NB, R_NC, R_KEY0, R_OUT0, R_CHUNK0 = range(READ_COLS)
_lib = None

_c_int, _c_p, _c_f = ctypes.c_int, ctypes.c_void_p, ctypes.c_float

# symbol -> argtypes; must match include/ext/clipfsar_timeline.h (tests/test_timeline_abi.py cross-checks against the header text)
SIGNATURES = {
    "cftl_version": [],
    "cftl_abi_version": [],
    "cftl_fold": [_c_p] * 11 + [_c_int] * 8 + [_c_f, _c_p],
    "cftl_read": [_c_p] * 11 + [_c_int] * 7 + [_c_p],
}


def lib():
    """Load (once) and return the ctypes handle.  Raises when the library is not built."""
    global _lib
    if _lib is None:
        _lib = _cabi.load(LIB_PATH, SIGNATURES, "cftl_", ABI_VERSION, "the timeline")
    return _lib


_check = _cabi.checker(lib, "cftl_")
_shape = _cabi.shape_checker("timeline_hip")
_dev, _stream = hip._dev, hip._stream

Table = _cabi.Table


def read_uploader(device, max_rows, depth=4):
    return TableUploader(device, max_rows, depth, cols=READ_COLS)


def _state(peak, at, above, marks, gens):
    """the state planes' shape checks -> (max_streams, B, cap) and, made only when asked, the five device pointers"""
    if peak.dim() != 3:
        raise RuntimeError("clip_fsar_amd.timeline_hip: peak must be [max_streams, B, cap], got shape %s" % (tuple(peak.shape),))
    M, B, cap = peak.shape
    for t, name in ((at, "at"), (above, "above"), (marks, "marks")):
        _shape(t, (M, B, cap), name)
    _shape(gens, (cap,), "gens")
    return (M, B, cap), lambda: (_dev(peak, torch.float32, "peak"), _dev(at, torch.int32, "at"), _dev(above, torch.int32, "above"),
                                 _dev(marks, torch.int32, "marks"), _dev(gens, torch.int32, "gens"))


def fold(scores, peak, at, above, marks, gens, keys, table, first, span, level=None):
    """scores [NOUT] flat (row i of the table owns a row-major [NW, NC] block at OUT0), peak fp32 / at / above / marks int32
    [max_streams, B, cap], gens [cap] int32, keys [NKEYS] int32, first: a Table of one column -- its .host [S] int32 on the host, its
    .dev their device copy --, each row's first window number: per (row, column j), with key = keys[KEY0 + j], the row's windows are
    folded into the cells [slot, (w // span) % B, key] (clip_fsar_amd.timeline: the rule).  level: None or a finite number.  scores is
    only read.  One launch."""
    (M, B, cap), state = _state(peak, at, above, marks, gens)
    if scores.dim() != 1 or keys.dim() != 1:
        raise RuntimeError("clip_fsar_amd.timeline_hip: scores and keys must be flat, got %s and %s" % (tuple(scores.shape),
                                                                                                       tuple(keys.shape)))
    S = table.S if isinstance(table, Table) else None            # (a table that is none is refused below)
    if S is not None and (not isinstance(first, Table) or first.host.is_cuda or first.host.dtype != torch.int32
                          or tuple(first.host.shape) != (S,) or not first.host.is_contiguous() or tuple(first.dev.shape) != (S,)
                          or first.S != S):
        raise RuntimeError("clip_fsar_amd.timeline_hip: first must be a Table of [S = %d] int32 host values and their device copy" % S)
    th, td, S = _cabi.table_args(table, TABLE_COLS, "timeline_hip")
    state = state()
    x = _dev(scores, torch.float32, "scores")
    if scores.shape[0] == 0:                       # no windows at all: an empty tensor has no address; the table is still validated, and
        x = state[0]                               # nothing is launched, so the stand-in is never dereferenced
    _check(lib().cftl_fold(x, *state, _dev(keys, torch.int32, "keys"), th, td, ctypes.c_void_p(first.host.data_ptr()),
                           _dev(first.dev, torch.int32, "first"), S, scores.shape[0], keys.shape[0], M, B, cap, int(span),
                           int(level is not None), 0.0 if level is None else float(level), _stream()), "cftl_fold")


def read(peak, at, above, marks, gens, keys, out_peak, out_at, out_above, table, span):
    """the state planes (as fold takes them), keys [NKEYS] int32 and the 7-column table -> out_peak fp32 / out_at / out_above int32
    [NOUT] flat: row r's row-major [NB, NC] block at its OUT0 holds, for bucket B0 + i and column j, the cell's values when it is live
    for that bucket, (-inf, -1, 0) when it is not and (NaN, -1, 0) when its key lies outside the store.  The state is only read.
    One launch."""
    (M, B, cap), state = _state(peak, at, above, marks, gens)
    if out_peak.dim() != 1 or keys.dim() != 1:
        raise RuntimeError("clip_fsar_amd.timeline_hip: out_peak and keys must be flat, got %s and %s" % (tuple(out_peak.shape),
                                                                                                         tuple(keys.shape)))
    _shape(out_at, tuple(out_peak.shape), "out_at")
    _shape(out_above, tuple(out_peak.shape), "out_above")
    th, td, S = _cabi.table_args(table, READ_COLS, "timeline_hip")
    state = state()
    outs = (_dev(out_peak, torch.float32, "out_peak"), _dev(out_at, torch.int32, "out_at"), _dev(out_above, torch.int32, "out_above"))
    if out_peak.shape[0] == 0:                     # no bucket at all: the table is still validated, nothing is launched
        outs = (state[0], state[1], state[2])
    _check(lib().cftl_read(*state, _dev(keys, torch.int32, "keys"), *outs, th, td, S, out_peak.shape[0], keys.shape[0], M, B, cap,
                           int(span), _stream()), "cftl_read")
