"""ctypes binding of libclipfsar_tempo.so (C ABI declared in include/ext/clipfsar_tempo.h): the tempo windows of
clip_fsar_amd.pool.StreamPool(rates=...) -- the gather of every window of a push at R frame rates out of the pool's ring, over the pool's
own descriptor table (pool_hip.Table, pool_hip's eight columns), and the reduction of the R scores of a (window, class) cell to their
maximum and the index of the tempo that gave it.

A library and a signature table of their own, like clip_fsar_amd.pool_hip: contiguous HIP device tensors only (no CPU path), launches on
the current stream of the operands' device, a non-zero return code raises with the library's message.  The rates travel as a small host
array that the library validates and hands to its kernel by value.
"""
from __future__ import annotations

import ctypes
import os

import torch  # noqa: F401  (imported first so that torch's HIP runtime is the one the library binds to)

from . import _cabi, hip
from .pool_hip import TABLE_COLS

ABI_VERSION = 1          # CFTP_ABI_VERSION of include/ext/clipfsar_tempo.h this file's SIGNATURES were written against
LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libclipfsar_tempo.so")
MAX_RATES = 8            # CFTP_MAX_RATES
_lib = None

_c_int, _c_p = ctypes.c_int, ctypes.c_void_p

# symbol -> argtypes; must match include/ext/clipfsar_tempo.h (tests/test_tempo_abi.py cross-checks against the header text)
SIGNATURES = {
    "cftp_version": [],
    "cftp_abi_version": [],
    "cftp_window_sequences": [_c_p] * 4 + [_c_int] * 9 + [_c_p, _c_int, _c_p],
    "cftp_reduce": [_c_p] * 3 + [_c_int] * 3 + [_c_p],
}


def lib():
    """Load (once) and return the ctypes handle.  Raises when the library is not built."""
    global _lib
    if _lib is None:
        _lib = _cabi.load(LIB_PATH, SIGNATURES, "cftp_", ABI_VERSION, "tempo windows")
    return _lib


_check = _cabi.checker(lib, "cftp_")
_shape = _cabi.shape_checker("tempo_hip")
_dev, _stream = hip._dev, hip._stream

Table = _cabi.Table


def window_sequences(ring, X, table, n_windows, w0, w1, T, stride, rates):
    """ring [max_streams, cap, E] -> X [(w1 - w0) * R, T, E] (at least: a larger X is written in its first rows): the R = len(rates)
    tempos of the windows w0 .. w1 - 1 of the table's packed window list of n_windows windows, rows ordered (window, tempo).  The table
    is the one a pool with rate = rates[-1] uploads."""
    M, cap, E = ring.shape
    R = len(rates)
    if X.dim() != 3 or X.shape[0] < (w1 - w0) * R or tuple(X.shape[1:]) != (T, E):
        raise RuntimeError("clip_fsar_amd.tempo_hip: X has shape %s, expected [>= %d, %d, %d]" % (tuple(X.shape), (w1 - w0) * R, T, E))
    th, td, S = _cabi.table_args(table, TABLE_COLS, "tempo_hip")
    host = (ctypes.c_int32 * max(1, R))(*[int(r) for r in rates])
    _check(lib().cftp_window_sequences(_dev(ring, torch.float32, "ring"), _dev(X, torch.float32, "X"), th, td, S, int(n_windows), int(w0),
                                       int(w1), int(T), E, M, cap, int(stride), ctypes.cast(host, _c_p), R, _stream()),
           "cftp_window_sequences")


def reduce(scores, out, tempo, R):
    """scores [NW * R, C] fp32, rows ordered (window, tempo) -> out [NW, C] fp32, tempo [NW, C] int32: per cell the largest of the R
    scores and the lowest index that holds it; when one of them is NaN, the first NaN and its index
    (clip_fsar_amd.pool.reference_reduce restates the rule).  out and tempo are buffers of their own.  One launch."""
    rows, C = scores.shape
    R = int(R)
    if R < 1 or rows % R:
        raise RuntimeError("clip_fsar_amd.tempo_hip: scores has shape %s, its rows are no multiple of R = %d" % (tuple(scores.shape), R))
    NW = rows // R
    _shape(out, (NW, C), "out")
    _shape(tempo, (NW, C), "tempo")
    _check(lib().cftp_reduce(_dev(scores, torch.float32, "scores"), _dev(out, torch.float32, "out"), _dev(tempo, torch.int32, "tempo"),
                             NW, R, C, _stream()), "cftp_reduce")
