"""ctypes binding of libclipfsar_contest.so (C ABI declared in include/ext/clipfsar_contest.h): the contest of
clip_fsar_amd.pool.StreamPool(events=EventRule(...), contest=Contest(...)) -- every window's row ranked on the device, the leading classes
kept, every other candidate demoted to -inf ahead of the detector (clip_fsar_amd.contest states the rule).

A library and a signature table of their own, like clip_fsar_amd.events_hip: contiguous HIP device tensors only (no CPU path), launches on
the current stream of the operands' device, a non-zero return code raises with the library's message.  The descriptor table is
class_smooth_hip's -- the same six columns, planned by class_smooth_hip.plan_rows, uploaded by its table_uploader -- and so are the key
lists: a pool that smooths by class, normalises, contests and detects plans and uploads once per push.
"""
from __future__ import annotations

import ctypes
import os

import torch  # noqa: F401  (imported first so that torch's HIP runtime is the one the library binds to)

from . import _cabi, hip
from .class_smooth_hip import plan_rows, table_uploader  # noqa: F401  (one planner and one table layout for the libraries over it)

ABI_VERSION = 1          # CFCT_ABI_VERSION of include/ext/clipfsar_contest.h this file's SIGNATURES were written against
LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libclipfsar_contest.so")
MAX_STREAMS = 65536      # CFCT_MAX_STREAMS
TABLE_COLS = 6           # CFCT_TABLE_COLS; the columns, in order:
SLOT, NW, OUT0, NC, KEY0, CHUNK0 = range(TABLE_COLS)
NONE = 0x7FFFFFFF        # CFCT_NONE: the padding of a leader list
_lib = None

_c_int, _c_p, _c_f = ctypes.c_int, ctypes.c_void_p, ctypes.c_float

# symbol -> argtypes; must match include/ext/clipfsar_contest.h (tests/test_contest_abi.py cross-checks against the header text)
SIGNATURES = {
    "cfct_version": [],
    "cfct_abi_version": [],
    "cfct_workspace_words": [_c_int],
    "cfct_contest": [_c_p] * 8 + [_c_int] * 6 + [_c_f, _c_p],
}


def lib():
    """Load (once) and return the ctypes handle.  Raises when the library is not built."""
    global _lib
    if _lib is None:
        _lib = _cabi.load(LIB_PATH, SIGNATURES, "cfct_", ABI_VERSION, "the contest")
    return _lib


_check = _cabi.checker(lib, "cfct_")
_shape = _cabi.shape_checker("contest_hip")
_dev, _stream = hip._dev, hip._stream

Table = _cabi.Table


def workspace_words(n_out):
    """uint32 elements (held as int32) of contest's `work` for a plane of n_out scores"""
    n = lib().cfct_workspace_words(int(n_out))
    if n < 0:
        raise RuntimeError("clip_fsar_amd.contest_hip: no workspace for n_out=%r (below 0)" % (n_out,))
    return n


def contest(scores, keys, out, leaders, n_leaders, work, table, cap, top, margin=None):
    """scores [NOUT] flat (row i of the table owns a row-major [NW, NC] block at OUT0), keys [NKEYS] int32 or None (every column
    competes; cap is then ignored) -> out [NOUT]: the scores' bits, every candidate that is not one of its window's leaders -inf; and,
    when given (both or neither), leaders [sum NW, top] int32 -- the leaders' columns ascending, NONE-padded -- and n_leaders [sum NW]
    int32, rows in table order then window order.  work: int32, at least workspace_words(NOUT).  out must not overlap scores.
    NOUT == 0: nothing is launched.  One launch."""
    if scores.dim() != 1 or work.dim() != 1 or (keys is not None and keys.dim() != 1):
        raise RuntimeError("clip_fsar_amd.contest_hip: scores, keys and work must be flat, got %s, %s and %s" % (
            tuple(scores.shape), None if keys is None else tuple(keys.shape), tuple(work.shape)))
    n_out = scores.shape[0]
    _shape(out, (n_out,), "out")
    if (leaders is None) != (n_leaders is None):
        raise RuntimeError("clip_fsar_amd.contest_hip: leaders and n_leaders go together")
    if isinstance(top, bool) or not isinstance(top, int) or top < 1:
        raise RuntimeError("clip_fsar_amd.contest_hip: top must be an integer >= 1, got %r" % (top,))
    host = getattr(table, "host", None)            # the sizes against the host rows, before any pointer is taken (table_args checks the table below)
    if isinstance(host, torch.Tensor) and host.dim() == 2 and host.shape[1] == TABLE_COLS and host.shape[0]:
        if leaders is not None:
            rows = int(host[:, NW].clamp(min=0).sum())
            if leaders.dim() != 2 or leaders.shape[1] != top or leaders.shape[0] != rows:
                raise RuntimeError("clip_fsar_amd.contest_hip: leaders has shape %s, expected [sum NW = %d, top = %d]" % (
                    tuple(leaders.shape), rows, top))
            _shape(n_leaders, (rows,), "n_leaders")
    if work.shape[0] < workspace_words(n_out):
        raise RuntimeError("clip_fsar_amd.contest_hip: work holds %d words, a plane of %d scores needs %d" % (
            work.shape[0], n_out, workspace_words(n_out)))
    th, td, S = _cabi.table_args(table, TABLE_COLS, "contest_hip")
    args = (_dev(scores, torch.float32, "scores"), None if keys is None else _dev(keys, torch.int32, "keys"),
            _dev(out, torch.float32, "out"), None if leaders is None else _dev(leaders, torch.int32, "leaders"),
            None if n_leaders is None else _dev(n_leaders, torch.int32, "n_leaders"), _dev(work, torch.int32, "work"))
    if n_out == 0:                                 # no windows at all: empty tensors have no address, and nothing would be launched
        return
    _check(lib().cfct_contest(*args, th, td, S, n_out, 0 if keys is None else keys.shape[0], int(cap), top, int(margin is not None),
                              0.0 if margin is None else float(margin), _stream()), "cfct_contest")
