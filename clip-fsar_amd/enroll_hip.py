"""ctypes binding of libclipfsar_enroll.so (C ABI declared in include/clipfsar_enroll.h): the support sequences of windows that lie in a
stream pool's ring -- T ring rows and the class's text row each -- for clip_fsar_amd.pool.StreamPool.enroll / enroll_windows.

A library and a signature table of their own, like clip_fsar_amd.groups_hip: contiguous HIP device tensors only (no CPU path), launches on
the current stream of the operands' device, a non-zero return code raises with the library's message.

The enrolment list, one row per output sequence, travels twice, as the pool's table does (include/clipfsar_enroll.h): the library validates
the host rows and the kernel reads the device copy.  pool_hip.TableUploader makes both, here with this library's row layout.
"""
from __future__ import annotations

import ctypes
import os

import torch  # noqa: F401  (imported first so that torch's HIP runtime is the one the library binds to)

from . import _cabi, hip
from .pool_hip import MAX_T, TableUploader  # noqa: F401  (the windows are the pool's: CFSP_MAX_T)

ABI_VERSION = 1          # CFEN_ABI_VERSION of include/clipfsar_enroll.h this file's SIGNATURES were written against
LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libclipfsar_enroll.so")
TABLE_COLS = 4           # CFEN_TABLE_COLS; the columns, in order:
SLOT, POS, CLS, PAD = range(TABLE_COLS)
_lib = None

_c_int, _c_p = ctypes.c_int, ctypes.c_void_p

# symbol -> argtypes; must match include/clipfsar_enroll.h (tests/test_build_recipe.py cross-checks against the header text)
SIGNATURES = {
    "cfen_version": [],
    "cfen_abi_version": [],
    "cfen_ring_sequences": [_c_p] * 4 + [_c_int] * 7 + [_c_p] * 2,
}


def lib():
    """Load (once) and return the ctypes handle.  Raises when the library is not built."""
    global _lib
    if _lib is None:
        _lib = _cabi.load(LIB_PATH, SIGNATURES, "cfen_", ABI_VERSION, "enrolment")
    return _lib


_check = _cabi.checker(lib, "cfen_")
_shape = _cabi.shape_checker("enroll_hip")
_dev, _stream = hip._dev, hip._stream


def table_rows(slots, positions, classes):
    """the enrolment list of sequences (ring slot, ring position of the first frame, text row), in output order"""
    return [[int(s), int(p), int(c), 0] for s, p, c in zip(slots, positions, classes)]


def table_uploader(device, max_rows, depth=4):
    """pool_hip.TableUploader with this library's row layout"""
    return TableUploader(device, max_rows, depth=depth, cols=TABLE_COLS)


def _table(t):
    return _cabi.table_args(t, TABLE_COLS, "enroll_hip")


def ring_sequences(ring, text, table, X0, rate=1):
    """ring [max_streams, cap, E], text [n_cls, E], table: a row (SLOT, POS, CLS, 0) per sequence -> X0 [n, T+1, E]:
    X0[i, j] = ring[SLOT_i, (POS_i + j * rate) mod cap] for j < T, X0[i, T] = text[CLS_i] -- gallery_hip.support_sequences' layout."""
    M, cap, E = ring.shape
    _shape(text, (text.shape[0], E), "text")
    if X0.dim() != 3 or X0.shape[1] < 2:
        raise RuntimeError("clip_fsar_amd.enroll_hip: X0 has shape %s, expected [n, T+1, E]" % (tuple(X0.shape),))
    th, td, n = _table(table)
    _shape(X0, (n, X0.shape[1], E), "X0")
    _check(lib().cfen_ring_sequences(_dev(ring, torch.float32, "ring"), _dev(text, torch.float32, "text"), th, td, n, X0.shape[1] - 1, E, M,
                                     cap, int(rate), text.shape[0], _dev(X0, torch.float32, "X0"), _stream()), "cfen_ring_sequences")
