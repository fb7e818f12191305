"""ctypes binding of libclipfsar_live.so (C ABI declared in include/clipfsar_live.h): the kernels of clip_fsar_amd.live_gallery.LiveGallery
-- cos_sim + OTAM against the slots of a prototype store named by a column list, the running class sums that take further shots, and the
norms of updated slots.

A library and a signature table of their own, like clip_fsar_amd.pool_hip: contiguous HIP device tensors only (no CPU path), launches on
the current stream of the operands' device, a non-zero return code raises with the library's message.

The descriptor table of the updates travels twice, as the pool's does (include/clipfsar_live.h): the library validates the host rows and
the kernels read the device copy.  pool_hip.TableUploader makes both, here with this library's row layout.
"""
from __future__ import annotations

import ctypes
import os

import torch  # noqa: F401  (imported first so that torch's HIP runtime is the one the library binds to)

from . import _cabi, hip
from .pool_hip import TableUploader

ABI_VERSION = 1          # CFSL_ABI_VERSION of include/clipfsar_live.h this file's SIGNATURES were written against
LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libclipfsar_live.so")
MAX_T = 32               # CFSL_MAX_T
MAX_ROWS = 65536         # CFSL_MAX_ROWS
TABLE_COLS = 4           # CFSL_TABLE_COLS; the columns, in order:
SLOT, OFF, N, PRIOR = range(TABLE_COLS)
_lib = None

_c_int, _c_p, _c_f = ctypes.c_int, ctypes.c_void_p, ctypes.c_float

# symbol -> argtypes; must match include/clipfsar_live.h (tests/test_build_recipe.py cross-checks against the header text)
SIGNATURES = {
    "cfsl_version": [],
    "cfsl_abi_version": [],
    "cfsl_otam_indexed": [_c_p] * 6 + [_c_int] * 5 + [_c_f, _c_int, _c_p],
    "cfsl_accumulate": [_c_p] * 5 + [_c_int] * 7 + [_c_p],
    "cfsl_slot_norms": [_c_p] * 4 + [_c_int] * 4 + [_c_p],
}


def lib():
    """Load (once) and return the ctypes handle.  Raises when the library is not built."""
    global _lib
    if _lib is None:
        _lib = _cabi.load(LIB_PATH, SIGNATURES, "cfsl_", ABI_VERSION, "the live gallery")
    return _lib


_check = _cabi.checker(lib, "cfsl_")
_shape = _cabi.shape_checker("live_hip")
_dev, _stream = hip._dev, hip._stream


def table_uploader(device, max_rows, depth=4):
    """pool_hip.TableUploader with this library's row layout"""
    return TableUploader(device, max_rows, depth=depth, cols=TABLE_COLS)


def _table(t):
    return _cabi.table_args(t, TABLE_COLS, "live_hip")


def otam_indexed(Xq, qn, P_store, pn_store, cols, logits, lbda=0.5, single_direct=False):
    """Xq [NQ, T, E], qn [NQ*T], P_store [cap, T, E], pn_store [cap*T], cols [C] int32 (device) -> logits [NQ, C]: what
    gallery_hip.otam_gallery gives on P_store[cols], bit for bit; a slot outside [0, cap) gives a column of NaN."""
    NQ, T, E = Xq.shape
    cap = P_store.shape[0]
    if cols.dim() != 1:
        raise RuntimeError("clip_fsar_amd.live_hip: cols has shape %s, expected [C]" % (tuple(cols.shape),))
    C = cols.shape[0]
    _shape(P_store, (cap, T, E), "P_store")
    _shape(qn, (NQ * T,), "qn")
    _shape(pn_store, (cap * T,), "pn_store")
    _shape(logits, (NQ, C), "logits")
    _check(lib().cfsl_otam_indexed(_dev(Xq, torch.float32, "Xq"), _dev(qn, torch.float32, "qn"), _dev(P_store, torch.float32, "P_store"),
                                   _dev(pn_store, torch.float32, "pn_store"), _dev(cols, torch.int32, "cols"),
                                   _dev(logits, torch.float32, "logits"), NQ, C, cap, T, E, float(lbda), int(bool(single_direct)),
                                   _stream()), "cfsl_otam_indexed")


def accumulate(X, sums, means, table, by_slot):
    """X [Nv, L, E]: the table's runs of videos into sums [cap, L, E] (rows 0 .. rows_kept-1), their means into means -- [cap, rows_kept, E]
    at the rows' slots with by_slot, else [S, rows_kept, E] in table order.  Rows: (slot, run offset, videos in the run, videos already
    in the slot's sum)."""
    Nv, L, E = X.shape
    cap = sums.shape[0]
    _shape(sums, (cap, L, E), "sums")
    S = getattr(table, "S", -1)
    if means.dim() != 3 or means.shape[0] != (cap if by_slot else S) or means.shape[2] != E:
        raise RuntimeError("clip_fsar_amd.live_hip: means must be [%d, rows_kept, %d], got %s" % (cap if by_slot else S, E,
                                                                                                 tuple(means.shape)))
    th, td, S = _table(table)
    _check(lib().cfsl_accumulate(_dev(X, torch.float32, "X"), _dev(sums, torch.float32, "sums"), _dev(means, torch.float32, "means"), th, td,
                                 S, Nv, L, E, cap, means.shape[1], int(bool(by_slot)), _stream()), "cfsl_accumulate")


def slot_norms(P_store, pn_store, table):
    """pn_store[slot * T + t] = |P_store[slot, t]| for the slots of the table's rows: gallery_hip.row_norms' bits on those rows"""
    cap, T, E = P_store.shape
    _shape(pn_store, (cap * T,), "pn_store")
    th, td, S = _table(table)
    _check(lib().cfsl_slot_norms(_dev(P_store, torch.float32, "P_store"), _dev(pn_store, torch.float32, "pn_store"), th, td, S, cap, T, E,
                                 _stream()), "cfsl_slot_norms")
