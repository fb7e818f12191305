"""ctypes binding of libclipfsar_ingest.so (C ABI declared in include/clipfsar_ingest.h): the test-time frame transform over uint8 clips
of mixed geometry in one launch, the kernel under clip_fsar_amd.ingest.FrameIngest.

A library and a signature table of their own, like clip_fsar_amd.pool_hip: contiguous HIP device tensors only (no CPU path), the launch
goes to the current stream of the operands' device, a non-zero return code raises with the library's message.

The descriptor table travels twice, as the pool's does (include/clipfsar_ingest.h): the library validates the host rows and the kernel
reads the device copy.  pool_hip.TableUploader makes both, here with this library's row layout.
"""
from __future__ import annotations

import ctypes
import os

import torch  # noqa: F401  (imported first so that torch's HIP runtime is the one the library binds to)

from . import _cabi, hip
from .pool_hip import TableUploader

ABI_VERSION = 1          # CFSI_ABI_VERSION of include/clipfsar_ingest.h this file's SIGNATURES were written against
LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libclipfsar_ingest.so")
MAX_GROUPS = 65536       # CFSI_MAX_GROUPS
SRC_ALIGN = 16           # CFSI_SRC_ALIGN: the unit of the table's source offsets, in bytes
TABLE_COLS = 9           # CFSI_TABLE_COLS; the columns, in order:
SRC_OFF16, N, OUT_OFF, H, W, SCALE_H, SCALE_W, Y0, X0 = range(TABLE_COLS)
_lib = None

_c_int, _c_i64, _c_p = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p

# symbol -> argtypes; must match include/clipfsar_ingest.h (tests/test_build_recipe.py cross-checks against the header text)
SIGNATURES = {
    "cfsi_version": [],
    "cfsi_abi_version": [],
    "cfsi_transform_frames": [_c_p, _c_i64] + [_c_p] * 3 + [_c_int] * 3 + [_c_p] * 3,
}


def lib():
    """Load (once) and return the ctypes handle.  Raises when the library is not built."""
    global _lib
    if _lib is None:
        _lib = _cabi.load(LIB_PATH, SIGNATURES, "cfsi_", ABI_VERSION, "frame ingest")
    return _lib


_check = _cabi.checker(lib, "cfsi_")
_shape = _cabi.shape_checker("ingest_hip")
_dev, _stream = hip._dev, hip._stream


def table_uploader(device, max_rows, depth=4):
    """pool_hip.TableUploader with this library's row layout"""
    return TableUploader(device, max_rows, depth=depth, cols=TABLE_COLS)


def _table(t):
    return _cabi.table_args(t, TABLE_COLS, "ingest_hip")


def transform_frames(src, out, table, crop, mean, std):
    """src: uint8 device bytes (any shape, contiguous) holding the table's groups -> out [N, 3, crop, crop] fp32, N = the table's frames"""
    N = out.shape[0]
    _shape(out, (N, 3, int(crop), int(crop)), "out")
    th, td, S = _table(table)
    m = (ctypes.c_float * 3)(*[float(v) for v in mean])
    sd = (ctypes.c_float * 3)(*[float(v) for v in std])
    _check(lib().cfsi_transform_frames(_dev(src, torch.uint8, "src"), src.numel(), _dev(out, torch.float32, "out"), th, td, S, N, int(crop),
                                       ctypes.cast(m, ctypes.c_void_p), ctypes.cast(sd, ctypes.c_void_p), _stream()),
           "cfsi_transform_frames")
