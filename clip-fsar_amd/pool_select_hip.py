"""ctypes binding of libclipfsar_pool_select.so (C ABI declared in include/ext/clipfsar_pool_select.h): the selection of
clip_fsar_amd.pool.StreamPool(shortlist=...) -- cfsh_select's threshold select per session of a push, with the (session, class) pairs the
pool's state is not done with pinned into the list, and the commit that zeroes the marks of a pair that returns after a gap.

A library and a signature table of their own, like clip_fsar_amd.shortlist_hip: contiguous HIP device tensors only (no CPU path), launches
on the current stream of the operands' device, a non-zero return code raises with the library's message.  The group table, one row
(Q0, NQ, SLOT, TICK) per group, travels twice as the other tables do: the library validates the host rows and the kernel reads the device
copy (pool_hip.TableUploader, here with this library's four columns).
"""
from __future__ import annotations

import ctypes
import os

import torch  # noqa: F401  (imported first so that torch's HIP runtime is the one the library binds to)

from . import _cabi, hip
from .pool_hip import TableUploader

ABI_VERSION = 1          # CFPS_ABI_VERSION of include/ext/clipfsar_pool_select.h this file's SIGNATURES were written against
LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libclipfsar_pool_select.so")
MAX_KEEP = 4096          # CFPS_MAX_KEEP
MAX_GROUPS = 65536       # CFPS_MAX_GROUPS
MAX_STREAMS = 65536      # CFPS_MAX_STREAMS
MAX_HOLD = 1 << 20       # CFPS_MAX_HOLD
MAX_CELLS = (1 << 31) - 1            # max_streams * cap: the kernel's cell index has 32 bits
NONE = 0x7fffffff        # CFPS_NONE: sel_cols of a place without a column (its sel_slots is -1, its sel_pin 0)
PIN_EVENT, PIN_HOLD = 1, 2           # CFPS_PIN_EVENT, CFPS_PIN_HOLD: the bits of sel_pin
TABLE_COLS = 4           # CFPS_TABLE_COLS; the columns, in order:
Q0, NQ, SLOT, TICK = range(TABLE_COLS)
_lib = None

_c_int, _c_p = ctypes.c_int, ctypes.c_void_p

# symbol -> argtypes; must match include/ext/clipfsar_pool_select.h (tests/test_pool_select_abi.py cross-checks against the header text)
SIGNATURES = {
    "cfps_version": [],
    "cfps_abi_version": [],
    "cfps_workspace_floats": [_c_int, _c_int],
    "cfps_select_pinned": [_c_p] * 11 + [_c_int] * 7 + [_c_p] * 6,
}


def lib():
    """Load (once) and return the ctypes handle.  Raises when the library is not built."""
    global _lib
    if _lib is None:
        _lib = _cabi.load(LIB_PATH, SIGNATURES, "cfps_", ABI_VERSION, "the pool's pinned selection")
    return _lib


_check = _cabi.checker(lib, "cfps_")
_shape = _cabi.shape_checker("pool_select_hip")
_dev, _stream = hip._dev, hip._stream

Table = _cabi.Table


def table_rows(counts, slots, ticks):
    """the group table of counts[i] consecutive windows of the session in slots[i] at its scoring push number ticks[i]: rows of
    (Q0, NQ, SLOT, TICK), and the number of windows"""
    rows, q = [], 0
    for n, slot, tick in zip(counts, slots, ticks):
        rows.append([q, int(n), int(slot), int(tick)])
        q += int(n)
    return rows, q


def table_uploader(device, max_rows, depth=4):
    """pool_hip.TableUploader with this library's row layout"""
    return TableUploader(device, max_rows, depth=depth, cols=TABLE_COLS)


def workspace_floats(G, NC):
    """floats of select_pinned's `work` for G groups over NC columns"""
    n = lib().cfps_workspace_floats(int(G), int(NC))
    if n < 0:
        raise RuntimeError("clip_fsar_amd.pool_select_hip: no workspace for G=%d groups x NC=%d columns (1 <= G <= %d, NC >= 1, "
                           "G * NC < 2^31)" % (G, NC, MAX_GROUPS))
    return n


def select_pinned(S, cols, gens, ev_streak, ev_marks, seen, merit, smooth_marks, base_marks, table, keep, hold, sel_cols, sel_slots,
                  sel_pin, n_pins, work):
    """S [NQ, NC], cols [NC] int32, gens [cap] int32, the planes [max_streams, cap] int32 (ev_streak and ev_marks both None or both
    given; smooth_marks and base_marks may each be None), table: a row (Q0, NQ, SLOT, TICK) per group -> sel_cols, sel_slots, sel_pin
    [G, K] int32, K = min(keep, NC), n_pins [G] int32: per group every pinned column and the best of the others (the K best pins when
    there are more than K), in ascending column order, their slots cols[column] and their PIN_* bits; places without a column hold NONE,
    -1 and 0 (clip_fsar_amd.shortlist.reference_select_pinned restates the rule).  The same launch commits: of a kept pair not seen at
    tick - 1 the marks are zeroed in the planes given, its seen becomes the tick, and its merit too when it is not pinned.  work: at
    least workspace_floats(G, NC) floats.  One launch."""
    NQ_, NC = S.shape
    K = min(int(keep), NC)
    M, cap = seen.shape
    _shape(cols, (NC,), "cols")
    _shape(gens, (cap,), "gens")
    _shape(merit, (M, cap), "merit")
    for t, name in ((ev_streak, "ev_streak"), (ev_marks, "ev_marks"), (smooth_marks, "smooth_marks"), (base_marks, "base_marks")):
        if t is not None:
            _shape(t, (M, cap), name)
    G = table.S if isinstance(table, Table) else 0
    _shape(sel_cols, (G, K), "sel_cols")
    _shape(sel_slots, (G, K), "sel_slots")
    _shape(sel_pin, (G, K), "sel_pin")
    _shape(n_pins, (G,), "n_pins")
    if work.dim() != 1 or work.shape[0] < G * NC:
        raise RuntimeError("clip_fsar_amd.pool_select_hip: work has shape %s, expected [>= %d]" % (tuple(work.shape), G * NC))
    th, td, G = _cabi.table_args(table, TABLE_COLS, "pool_select_hip")
    plane = lambda t, name: None if t is None else _dev(t, torch.int32, name)
    _check(lib().cfps_select_pinned(_dev(S, torch.float32, "S"), _dev(cols, torch.int32, "cols"), _dev(gens, torch.int32, "gens"),
                                    plane(ev_streak, "ev_streak"), plane(ev_marks, "ev_marks"), _dev(seen, torch.int32, "seen"),
                                    _dev(merit, torch.int32, "merit"), plane(smooth_marks, "smooth_marks"),
                                    plane(base_marks, "base_marks"), th, td, G, NQ_, NC, int(keep), int(hold), M, cap,
                                    _dev(sel_cols, torch.int32, "sel_cols"), _dev(sel_slots, torch.int32, "sel_slots"),
                                    _dev(sel_pin, torch.int32, "sel_pin"), _dev(n_pins, torch.int32, "n_pins"),
                                    _dev(work, torch.float32, "work"), _stream()), "cfps_select_pinned")
