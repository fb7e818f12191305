"""ctypes binding of libclipfsar_evidence.so (C ABI declared in include/ext/clipfsar_evidence.h): the event evidence of
clip_fsar_amd.pool.StreamPool(events=..., evidence=Evidence(...)) -- the T ring rows of the window behind an event record, copied into a
slot of a device store by the push that detected it, over the detector's records while they are still on the device
(clip_fsar_amd.events_hip.detect's events and n_events) and a descriptor table of its own, a row per row of the detector's table.

A library and a signature table of their own, like clip_fsar_amd.tempo_hip: contiguous HIP device tensors only (no CPU path), launches on
the current stream of the operands' device, a non-zero return code raises with the library's message.  The rates travel as a small host
array that the library validates and hands to its kernel by value.  clip_fsar_amd.evidence.reference_capture restates the rule.
"""
from __future__ import annotations

import ctypes
import os

import torch  # noqa: F401  (imported first so that torch's HIP runtime is the one the library binds to)

from . import _cabi, hip
from .events_hip import EVENT_COLS
from .pool_hip import TableUploader

ABI_VERSION = 1          # CFED_ABI_VERSION of include/ext/clipfsar_evidence.h this file's SIGNATURES were written against
LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libclipfsar_evidence.so")
MAX_STREAMS = 65536      # CFED_MAX_STREAMS
MAX_RATES = 8            # CFED_MAX_RATES
CHUNK = 256              # CFED_CHUNK: records per step of the placement pass
TABLE_COLS = 6           # CFED_TABLE_COLS; the columns, in order:
SLOT, POS0, NW, KEEP0, OUT0, NC = range(TABLE_COLS)
KIND_ONSET, KIND_OFFSET = 1, 2                   # bits of `kinds`
NOT_CAPTURED, LEFT_RING, NO_ROOM = -1, -2, -3    # where[i, 0] of a record without a slot
WORK_COLS = 3            # CFED_WORK_COLS
_lib = None

_c_int, _c_p = ctypes.c_int, ctypes.c_void_p

# symbol -> argtypes; must match include/ext/clipfsar_evidence.h (tests/test_evidence_abi.py cross-checks against the header text)
SIGNATURES = {
    "cfed_version": [],
    "cfed_abi_version": [],
    "cfed_workspace_ints": [_c_int],
    "cfed_capture": [_c_p] * 10 + [_c_int] * 9 + [_c_p, _c_int, _c_int, _c_p],
}


def lib():
    """Load (once) and return the ctypes handle.  Raises when the library is not built."""
    global _lib
    if _lib is None:
        _lib = _cabi.load(LIB_PATH, SIGNATURES, "cfed_", ABI_VERSION, "event evidence")
    return _lib


_check = _cabi.checker(lib, "cfed_")
_shape = _cabi.shape_checker("evidence_hip")
_dev, _stream = hip._dev, hip._stream

Table = _cabi.Table


def table_uploader(device, max_rows, depth=4):
    return TableUploader(device, max_rows, depth, cols=TABLE_COLS)


def workspace_ints(capacity):
    """int32 elements of capture's `work` for a store of `capacity` slots"""
    n = lib().cfed_workspace_ints(int(capacity))
    if n < 0:
        raise RuntimeError("clip_fsar_amd.evidence_hip: no workspace for capacity=%r (below 1, or 2^31 ints and more)" % (capacity,))
    return n


def capture(ring, events, n_events, tempo, store, head, where, work, table, kinds, stride, rate, rates=None):
    """ring [max_streams, cap, E] fp32, events [max_events, 5] int32 and n_events [1] int32 as events_hip.detect leaves them, tempo: the
    push's session-major tempo plane (int32, any shape, read flat) together with rates, or None without -> store [capacity, T, E] fp32
    receives the windows of the qualifying records in the slots head, head + 1, .. (mod capacity), head [1] int32 advances, and
    where [max_events, 2] int32 receives per record (slot, tempo index) or (NOT_CAPTURED | LEFT_RING | NO_ROOM, 0).  work: int32, at
    least workspace_ints(capacity).  table: TABLE_COLS columns, a row per row of the detector's table.  Two launches."""
    M, cap, E = ring.shape
    if store.dim() != 3 or store.shape[2] != E:
        raise RuntimeError("clip_fsar_amd.evidence_hip: store has shape %s, expected [capacity, T, %d]" % (tuple(store.shape), E))
    capacity, T, _ = store.shape
    if events.dim() != 2 or events.shape[1] != EVENT_COLS or events.shape[0] < 1:
        raise RuntimeError("clip_fsar_amd.evidence_hip: events has shape %s, expected [max_events >= 1, %d]" % (tuple(events.shape), EVENT_COLS))
    _shape(n_events, (1,), "n_events")
    _shape(head, (1,), "head")
    _shape(where, (events.shape[0], 2), "where")
    if work.dim() != 1 or work.shape[0] < workspace_ints(capacity):
        raise RuntimeError("clip_fsar_amd.evidence_hip: work has shape %s, a store of %d slots needs %d ints" % (
            tuple(work.shape), capacity, workspace_ints(capacity)))
    if (tempo is None) != (rates is None):
        raise RuntimeError("clip_fsar_amd.evidence_hip: tempo and rates go together, got tempo %s and rates %r" % (
            "None" if tempo is None else "given", rates))
    R = 0 if rates is None else len(rates)
    host = (ctypes.c_int32 * max(1, R))(*[int(r) for r in (rates or ())])
    th, td, S = _cabi.table_args(table, TABLE_COLS, "evidence_hip")
    _check(lib().cfed_capture(_dev(ring, torch.float32, "ring"), _dev(events, torch.int32, "events"), _dev(n_events, torch.int32, "n_events"),
                              None if tempo is None else _dev(tempo, torch.int32, "tempo"), _dev(store, torch.float32, "store"),
                              _dev(head, torch.int32, "head"), _dev(where, torch.int32, "where"), _dev(work, torch.int32, "work"), th, td, S,
                              M, cap, events.shape[0], int(kinds), T, E, int(stride), int(rate), ctypes.cast(host, _c_p), R, capacity,
                              _stream()), "cfed_capture")
