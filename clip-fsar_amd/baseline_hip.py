"""ctypes binding of libclipfsar_baseline.so (C ABI declared in include/ext/clipfsar_baseline.h): the adaptive baselines of
clip_fsar_amd.pool.StreamPool(baseline=Baseline(...)), a running mean and mean absolute deviation per (session slot, class store slot)
whose cells are guarded by the store slots' generations as clip_fsar_amd.class_smooth_hip's are, and the deviation of every score from
them.

A library and a signature table of their own, like clip_fsar_amd.events_hip: contiguous HIP device tensors only (no CPU path), launches
on the current stream of the operands' device, a non-zero return code raises with the library's message.  The descriptor table is
class_smooth_hip's -- the same six columns, planned by class_smooth_hip.plan_rows, uploaded by its table_uploader -- and so are the key
lists: a pool that smooths by class, keeps baselines and detects events plans and uploads once per push.
"""
from __future__ import annotations

import ctypes
import os

import torch  # noqa: F401  (imported first so that torch's HIP runtime is the one the library binds to)

from . import _cabi, hip
from .class_smooth_hip import plan_rows, table_uploader  # noqa: F401  (one planner and one table layout for the three libraries)

ABI_VERSION = 1          # CFBL_ABI_VERSION of include/ext/clipfsar_baseline.h this file's SIGNATURES were written against
LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libclipfsar_baseline.so")
MAX_STREAMS = 65536      # CFBL_MAX_STREAMS
CHUNK = 256              # CFBL_CHUNK: columns per workgroup
MAX_CELLS = (1 << 31) - 1            # max_streams * cap: the kernel's cell index has 32 bits
MAX_WARMUP = 1 << 20     # CFBL_MAX_WARMUP
TABLE_COLS = 6           # CFBL_TABLE_COLS; the columns, in order:
SLOT, NW, OUT0, NC, KEY0, CHUNK0 = range(TABLE_COLS)
_lib = None

_c_int, _c_p, _c_f = ctypes.c_int, ctypes.c_void_p, ctypes.c_float

# symbol -> argtypes; must match include/ext/clipfsar_baseline.h (tests/test_baseline_abi.py cross-checks against the header text)
SIGNATURES = {
    "cfbl_version": [],
    "cfbl_abi_version": [],
    "cfbl_normalize": [_c_p] * 10 + [_c_int] * 5 + [_c_f, _c_f, _c_int, _c_f, _c_f, _c_p],
}


def lib():
    """Load (once) and return the ctypes handle.  Raises when the library is not built."""
    global _lib
    if _lib is None:
        _lib = _cabi.load(LIB_PATH, SIGNATURES, "cfbl_", ABI_VERSION, "adaptive baselines")
    return _lib


_check = _cabi.checker(lib, "cfbl_")
_shape = _cabi.shape_checker("baseline_hip")
_dev, _stream = hip._dev, hip._stream

Table = _cabi.Table


def normalize(scores, mean, dev, count, marks, gens, keys, out, table, rate, warm_rate, warmup, gate, floor):
    """scores [NOUT] flat (row i of the table owns a row-major [NW, NC] block at OUT0), mean / dev [max_streams, cap] fp32, count / marks
    [max_streams, cap] int32, gens [cap] int32, keys [NKEYS] int32 -> out [NOUT]: per (row, column j), with key = keys[KEY0 + j], the
    deviation z of every window from the pair's running mean and mean absolute deviation (clip_fsar_amd.baseline: the recurrence),
    continued from the cell when marks[slot, key] == gens[key] and started otherwise; the cell advances and its mark receives the
    generation.  out may be scores.  One launch."""
    M, cap = mean.shape
    for t, name in ((dev, "dev"), (count, "count"), (marks, "marks")):
        _shape(t, (M, cap), name)
    _shape(gens, (cap,), "gens")
    _shape(out, tuple(scores.shape), "out")
    if scores.dim() != 1 or keys.dim() != 1:
        raise RuntimeError("clip_fsar_amd.baseline_hip: scores and keys must be flat, got %s and %s" % (tuple(scores.shape),
                                                                                                       tuple(keys.shape)))
    th, td, S = _cabi.table_args(table, TABLE_COLS, "baseline_hip")
    x, y = _dev(scores, torch.float32, "scores"), _dev(out, torch.float32, "out")
    if scores.shape[0] == 0:                       # no windows at all: an empty tensor has no address; the table is still validated, and
        x = y = _dev(mean, torch.float32, "mean")  # nothing is launched, so the stand-in is never dereferenced
    _check(lib().cfbl_normalize(x, _dev(mean, torch.float32, "mean"), _dev(dev, torch.float32, "dev"), _dev(count, torch.int32, "count"),
                                _dev(marks, torch.int32, "marks"), _dev(gens, torch.int32, "gens"), _dev(keys, torch.int32, "keys"), y,
                                th, td, S, scores.shape[0], keys.shape[0], M, cap, float(rate), float(warm_rate), int(warmup), float(gate),
                                float(floor), _stream()), "cfbl_normalize")
