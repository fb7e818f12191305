"""ctypes binding of libclipfsar_class_smooth.so (C ABI declared in include/ext/clipfsar_class_smooth.h): the smoothing recurrence of
clip_fsar_amd.pool.StreamPool(smooth_by="class"), whose state is keyed by (session slot, class store slot) and guarded by the store slots'
generations (clip_fsar_amd.live_gallery.LiveGallery.slot_generations).

A library and a signature table of their own, like clip_fsar_amd.pool_hip: contiguous HIP device tensors only (no CPU path), launches on
the current stream of the operands' device, a non-zero return code raises with the library's message.  The descriptor table travels
twice, as pool_hip's (table_uploader: pool_hip.TableUploader at this table's width).
"""
from __future__ import annotations

import collections
import ctypes
import os

import torch  # noqa: F401  (imported first so that torch's HIP runtime is the one the library binds to)

from . import _cabi, hip
from .pool_hip import TableUploader

ABI_VERSION = 1          # CFCS_ABI_VERSION of include/ext/clipfsar_class_smooth.h this file's SIGNATURES were written against
LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libclipfsar_class_smooth.so")
MAX_STREAMS = 65536      # CFCS_MAX_STREAMS
CHUNK = 256              # CFCS_CHUNK: columns per workgroup
MAX_CELLS = (1 << 31) - 1            # max_streams * cap: the kernel's cell index has 32 bits
TABLE_COLS = 6           # CFCS_TABLE_COLS; the columns, in order:
SLOT, NW, OUT0, NC, KEY0, CHUNK0 = range(TABLE_COLS)
_lib = None

_c_int, _c_p, _c_f = ctypes.c_int, ctypes.c_void_p, ctypes.c_float

# symbol -> argtypes; must match include/ext/clipfsar_class_smooth.h (tests/test_class_smooth_abi.py cross-checks against the header text)
SIGNATURES = {
    "cfcs_version": [],
    "cfcs_abi_version": [],
    "cfcs_smooth_classes": [_c_p] * 8 + [_c_int] * 5 + [_c_f, _c_p],
}


def lib():
    """Load (once) and return the ctypes handle.  Raises when the library is not built."""
    global _lib
    if _lib is None:
        _lib = _cabi.load(LIB_PATH, SIGNATURES, "cfcs_", ABI_VERSION, "per-class smoothing")
    return _lib


_check = _cabi.checker(lib, "cfcs_")
_shape = _cabi.shape_checker("class_smooth_hip")
_dev, _stream = hip._dev, hip._stream


def table_uploader(device, max_rows, depth=4):
    return TableUploader(device, max_rows, depth, cols=TABLE_COLS)


Table = _cabi.Table
SmoothPlan = collections.namedtuple("SmoothPlan", "rows keys every n_out n_chunks")


def plan_rows(slots, n_windows, lists, n_every):
    """The host plan of one launch (pure).  Per session of the push: its slot, its windows, and its list of store slots -- or None: the
    "every class" list, of n_every store slots, which the planner never looks into.  -> SmoothPlan(rows: the descriptor table; keys: the
    sessions' own lists one after the other, equal lists once; every: whether a session points at the "every class" list -- the device
    keys are then that list FIRST (keys[0 .. n_every), once however many sessions point at it) and `keys` behind it; n_out: floats of
    the flat logits; n_chunks: the grid).  A session's block is [n_windows, its width], row-major, the blocks in the order given.  The
    work is O(sessions + the own lists' lengths): a push without lists uploads no key at all."""
    every = any(own is None for own in lists)
    if every and n_every < 1:
        raise ValueError("clip_fsar_amd.class_smooth_hip: the \"every class\" list is empty")
    rows, keys, where = [], [], {}
    first = int(n_every) if every else 0           # where the own lists start
    n_out = n_chunks = 0
    for slot, nW, own in zip(slots, n_windows, lists):
        if own is None:
            key0, NC = 0, int(n_every)
        else:
            seg = tuple(own)
            if not seg:
                raise ValueError("clip_fsar_amd.class_smooth_hip: a session's list of store slots is empty")
            if seg not in where:
                where[seg] = first + len(keys)
                keys.extend(seg)
            key0, NC = where[seg], len(seg)
        rows.append([int(slot), int(nW), n_out, NC, key0, n_chunks])
        n_out += int(nW) * NC
        n_chunks += -(-NC // CHUNK)
    return SmoothPlan(rows, keys, every, n_out, n_chunks)


def smooth_classes(logits, state, marks, gens, keys, out, table, alpha):
    """logits [NOUT] flat (row i of the table owns a row-major [NW, NC] block at OUT0), state [max_streams, cap] fp32, marks
    [max_streams, cap] int32, gens [cap] int32, keys [NKEYS] int32 -> out [NOUT]: per (row, column j), with key = keys[KEY0 + j], the
    recurrence y_k = fmaf(alpha, y_{k-1}, (1 - alpha) * x_k) over the row's windows, continued from state[slot, key] when
    marks[slot, key] == gens[key] and started (y_0 = x_0) otherwise; state and marks receive the last y and the generation.  out may
    be logits.  One launch."""
    M, cap = state.shape
    _shape(marks, (M, cap), "marks")
    _shape(gens, (cap,), "gens")
    _shape(out, tuple(logits.shape), "out")
    if logits.dim() != 1 or keys.dim() != 1:
        raise RuntimeError("clip_fsar_amd.class_smooth_hip: logits and keys must be flat, got %s and %s" % (tuple(logits.shape),
                                                                                                           tuple(keys.shape)))
    th, td, S = _cabi.table_args(table, TABLE_COLS, "class_smooth_hip")
    x, y = _dev(logits, torch.float32, "logits"), _dev(out, torch.float32, "out")
    if logits.shape[0] == 0:                       # no windows at all: an empty tensor has no address; the table is still validated, and
        x = y = _dev(state, torch.float32, "state")                        # nothing is launched, so the stand-in is never dereferenced
    _check(lib().cfcs_smooth_classes(x, _dev(state, torch.float32, "state"), _dev(marks, torch.int32, "marks"),
                                     _dev(gens, torch.int32, "gens"), _dev(keys, torch.int32, "keys"), y, th, td, S, logits.shape[0],
                                     keys.shape[0], M, cap, float(alpha), _stream()), "cfcs_smooth_classes")
