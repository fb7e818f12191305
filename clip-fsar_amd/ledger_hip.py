"""ctypes binding of libclipfsar_ledger.so (C ABI declared in include/ext/clipfsar_ledger.h): the per-shot store of
clip_fsar_amd.live_gallery.LiveGallery(ledger=ShotLedger(...)) -- a call's addends into store slots (put), the touched classes' sums and
means again from the addends that remain (resum: cfsl_accumulate's bits on the same addends), and the leave-one-out agreement of every
shot with the rest of its class (fit).  clip_fsar_amd.ledger states the bookkeeping and restates fit on the host.

A library and a signature table of their own, like clip_fsar_amd.history_hip: contiguous HIP device tensors only (no CPU path), launches
on the current stream of the operands' device, a non-zero return code raises with the library's message.  The descriptor table -- a row
(SLOT, FIRST, N) per touched class -- travels twice, as the live gallery's does: the library validates the host rows and the kernels
read the device copy.  pool_hip.TableUploader makes both, here with this library's row layout.
"""
from __future__ import annotations

import ctypes
import os

import torch  # noqa: F401  (imported first so that torch's HIP runtime is the one the library binds to)

from . import _cabi, hip
from .pool_hip import TableUploader

ABI_VERSION = 1          # CFLD_ABI_VERSION of include/ext/clipfsar_ledger.h this file's SIGNATURES were written against
LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libclipfsar_ledger.so")
MAX_ROWS = 65536         # CFLD_MAX_ROWS
MAX_T = 32               # CFLD_MAX_T
TABLE_COLS = 3           # CFLD_TABLE_COLS; the columns, in order:
SLOT, FIRST, N = range(TABLE_COLS)
_lib = None

_c_int, _c_p = ctypes.c_int, ctypes.c_void_p

# symbol -> argtypes; must match include/ext/clipfsar_ledger.h (tests/test_ledger_abi.py cross-checks against the header text)
SIGNATURES = {
    "cfld_version": [],
    "cfld_abi_version": [],
    "cfld_put": [_c_p] * 3 + [_c_int] * 5 + [_c_p],
    "cfld_resum": [_c_p] * 6 + [_c_int] * 8 + [_c_p],
    "cfld_fit": [_c_p] * 6 + [_c_int] * 8 + [_c_p],
}


def lib():
    """Load (once) and return the ctypes handle.  Raises when the library is not built."""
    global _lib
    if _lib is None:
        _lib = _cabi.load(LIB_PATH, SIGNATURES, "cfld_", ABI_VERSION, "the shot ledger")
    return _lib


_check = _cabi.checker(lib, "cfld_")
_shape = _cabi.shape_checker("ledger_hip")
_dev, _stream = hip._dev, hip._stream

Table = _cabi.Table


def table_uploader(device, max_rows, depth=4):
    """pool_hip.TableUploader with this library's row layout"""
    return TableUploader(device, max_rows, depth=depth, cols=TABLE_COLS)


def _table(t):
    return _cabi.table_args(t, TABLE_COLS, "ledger_hip")


def _list(t, name):
    if t.dim() != 1 or t.shape[0] < 1:
        raise RuntimeError("clip_fsar_amd.ledger_hip: %s has shape %s, expected a non-empty [n]" % (name, tuple(t.shape)))
    return t.shape[0]


def put(X, store, slots):
    """X [Nv, L, E]: the first rows_kept rows of video v into store[slots[v]]; store [shots, rows_kept, E], slots [Nv] int32 (device),
    all different.  A slot outside [0, shots) writes nothing.  index_copy_'s bits."""
    if X.dim() != 3 or store.dim() != 3:
        raise RuntimeError("clip_fsar_amd.ledger_hip: X must be [Nv, L, E] and store [shots, rows_kept, E], got %s and %s" % (
            tuple(X.shape), tuple(store.shape)))
    Nv, L, E = X.shape
    shots, rows_kept = store.shape[0], store.shape[1]
    _shape(store, (shots, rows_kept, E), "store")
    _shape(slots, (Nv,), "slots")
    _check(lib().cfld_put(_dev(X, torch.float32, "X"), _dev(store, torch.float32, "store"), _dev(slots, torch.int32, "slots"), Nv, L, E,
                          shots, rows_kept, _stream()), "cfld_put")


def resum(store, slot_list, sums, means, table, by_slot):
    """store [shots, rows_kept, E], slot_list [n] int32 (device): the table's classes (rows (class slot, first, n): the class's addends
    are store[slot_list[first : first + n]], in that order) into sums [cap, L, E] (rows 0 .. rows_kept-1) and their means into means --
    [cap, rows_kept, E] at the rows' slots with by_slot, else [S, rows_kept, E] in table order.  What live_hip.accumulate gives on the
    same addends with prior = 0, bit for bit."""
    if store.dim() != 3 or sums.dim() != 3:
        raise RuntimeError("clip_fsar_amd.ledger_hip: store must be [shots, rows_kept, E] and sums [cap, L, E], got %s and %s" % (
            tuple(store.shape), tuple(sums.shape)))
    shots, rows_kept, E = store.shape
    cap, L = sums.shape[0], sums.shape[1]
    _shape(sums, (cap, L, E), "sums")
    n = _list(slot_list, "slot_list")
    S = getattr(table, "S", -1)
    _shape(means, (cap if by_slot else S, rows_kept, E), "means")
    th, td, S = _table(table)
    _check(lib().cfld_resum(_dev(store, torch.float32, "store"), _dev(slot_list, torch.int32, "slot_list"), _dev(sums, torch.float32, "sums"),
                            _dev(means, torch.float32, "means"), th, td, S, n, shots, rows_kept, L, E, cap, int(bool(by_slot)), _stream()),
           "cfld_resum")


def fit(store, sums, slot_list, out, table, T):
    """out [n] fp32: for list position p of its table row (class slot, first, n), the mean over rows r < T of the cosine between
    x = store[slot_list[p]][r] and sums[class slot][r] - x; NaN for a class of one shot.  clip_fsar_amd.ledger.reference_fit restates it."""
    if store.dim() != 3 or sums.dim() != 3:
        raise RuntimeError("clip_fsar_amd.ledger_hip: store must be [shots, rows_kept, E] and sums [cap, L, E], got %s and %s" % (
            tuple(store.shape), tuple(sums.shape)))
    shots, rows_kept, E = store.shape
    cap, L = sums.shape[0], sums.shape[1]
    _shape(sums, (cap, L, E), "sums")
    n = _list(slot_list, "slot_list")
    _shape(out, (n,), "out")
    if isinstance(T, bool) or not isinstance(T, int) or not 1 <= T <= min(MAX_T, rows_kept):
        raise RuntimeError("clip_fsar_amd.ledger_hip: T must be an integer in [1, min(%d, rows_kept = %d)], got %r" % (MAX_T, rows_kept, T))
    th, td, S = _table(table)
    _check(lib().cfld_fit(_dev(store, torch.float32, "store"), _dev(sums, torch.float32, "sums"), _dev(slot_list, torch.int32, "slot_list"),
                          _dev(out, torch.float32, "out"), th, td, S, n, shots, rows_kept, L, T, E, cap, _stream()), "cfld_fit")
