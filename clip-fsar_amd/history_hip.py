"""ctypes binding of libclipfsar_history.so (C ABI declared in include/ext/clipfsar_history.h): the peak search of
clip_fsar_amd.pool.StreamPool(history=History(...)).search -- a score plane [windows, classes] over the windows the history store still
holds -> per class its best occurrences that do not overlap (clip_fsar_amd.history states the rule).

A library and a signature table of their own, like clip_fsar_amd.contest_hip: contiguous HIP device tensors only (no CPU path), launches
on the current stream of the operands' device, a non-zero return code raises with the library's message.  The descriptor table is
pool_hip's -- the same eight columns, uploaded by its TableUploader -- and it is the very table the gather of the searched windows was
given: a search plans and uploads once.
"""
from __future__ import annotations

import ctypes
import os

import torch  # noqa: F401  (imported first so that torch's HIP runtime is the one the library binds to)

from . import _cabi, hip
from .pool_hip import TableUploader  # noqa: F401  (one table layout and one uploader for the libraries over it)

ABI_VERSION = 1          # CFHS_ABI_VERSION of include/ext/clipfsar_history.h this file's SIGNATURES were written against
LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libclipfsar_history.so")
MAX_STREAMS = 65536      # CFHS_MAX_STREAMS
TABLE_COLS = 8           # CFHS_TABLE_COLS; the columns, in order:
SLOT, PUT_POS, N, FEAT_OFF, WIN_POS, NW, WIN_OFF, HAS_STATE = range(TABLE_COLS)
MAX_CLASSES = 64         # CFHS_MAX_CLASSES
MAX_TOP = 4096           # CFHS_MAX_TOP
MAX_SEPARATION = 4096    # CFHS_MAX_SEPARATION
MAX_PLANE = 1 << 30      # the scores of a plane, NW * K, at most (cfhs_workspace_words answers -1 beyond it)
NONE = 0x7FFFFFFF        # CFHS_NONE: an unused place of hit_rows
_lib = None

_c_int, _c_p, _c_f = ctypes.c_int, ctypes.c_void_p, ctypes.c_float

# symbol -> argtypes; must match include/ext/clipfsar_history.h (tests/test_history_abi.py cross-checks against the header text)
SIGNATURES = {
    "cfhs_version": [],
    "cfhs_abi_version": [],
    "cfhs_workspace_words": [_c_int, _c_int],
    "cfhs_peaks": [_c_p] * 8 + [_c_int] * 5 + [_c_f, _c_int, _c_p],
}


def lib():
    """Load (once) and return the ctypes handle.  Raises when the library is not built."""
    global _lib
    if _lib is None:
        _lib = _cabi.load(LIB_PATH, SIGNATURES, "cfhs_", ABI_VERSION, "the history search")
    return _lib


_check = _cabi.checker(lib, "cfhs_")
_shape = _cabi.shape_checker("history_hip")
_dev, _stream = hip._dev, hip._stream

Table = _cabi.Table


def workspace_words(n_windows, n_classes):
    """uint32 elements (held as int32) of peaks' `work` for a plane of n_windows x n_classes scores"""
    n = lib().cfhs_workspace_words(int(n_windows), int(n_classes))
    if n < 0:
        raise RuntimeError("clip_fsar_amd.history_hip: no workspace for a plane of %r windows x %r classes (a negative count, no class, "
                           "or more than 2^30 scores)" % (n_windows, n_classes))
    return n


def peaks(scores, work, hit_rows, hit_scores, n_hits, n_peaks, table, separation, min_score, top):
    """scores [NW, K] fp32, the plane whose rows WIN_OFF .. WIN_OFF + NW - 1 belong to table row r -> hit_rows [K, top] int32: per class
    the plane rows of its `top` highest peaks in ascending order, NONE behind them; hit_scores [K, top] fp32: the plane's bits there,
    0 behind them; n_hits [K] int32 and n_peaks [K] int32: the places filled and the peaks before `top` cut them.  work: int32, at
    least workspace_words(NW, K), overlapping nothing else.  min_score: None or a number that is not NaN.  NW == 0: nothing is launched
    and the outputs stay as they are.  Two launches."""
    if scores.dim() != 2 or work.dim() != 1:
        raise RuntimeError("clip_fsar_amd.history_hip: scores must be [NW, K] and work flat, got %s and %s" % (
            tuple(scores.shape), tuple(work.shape)))
    n_windows, K = scores.shape
    for name, v, lo, hi in (("top", top, 1, MAX_TOP), ("separation", separation, 0, MAX_SEPARATION)):
        if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
            raise RuntimeError("clip_fsar_amd.history_hip: %s must be an integer in [%d, %d], got %r" % (name, lo, hi, v))
    if not 1 <= K <= MAX_CLASSES:
        raise RuntimeError("clip_fsar_amd.history_hip: scores has K = %d columns, the search takes 1 .. %d classes" % (K, MAX_CLASSES))
    if min_score is not None and min_score != min_score:
        raise RuntimeError("clip_fsar_amd.history_hip: min_score is NaN")
    _shape(hit_rows, (K, top), "hit_rows")
    _shape(hit_scores, (K, top), "hit_scores")
    _shape(n_hits, (K,), "n_hits")
    _shape(n_peaks, (K,), "n_peaks")
    if work.shape[0] < workspace_words(n_windows, K):
        raise RuntimeError("clip_fsar_amd.history_hip: work holds %d words, a plane of %d x %d scores needs %d" % (
            work.shape[0], n_windows, K, workspace_words(n_windows, K)))
    th, td, S = _cabi.table_args(table, TABLE_COLS, "history_hip")
    args = (_dev(scores, torch.float32, "scores"), _dev(work, torch.int32, "work"), _dev(hit_rows, torch.int32, "hit_rows"),
            _dev(hit_scores, torch.float32, "hit_scores"), _dev(n_hits, torch.int32, "n_hits"), _dev(n_peaks, torch.int32, "n_peaks"))
    if n_windows == 0:                             # no windows at all: empty tensors have no address, and nothing would be launched
        return
    _check(lib().cfhs_peaks(*args, th, td, S, n_windows, K, separation, int(min_score is not None),
                            0.0 if min_score is None else float(min_score), top, _stream()), "cfhs_peaks")
