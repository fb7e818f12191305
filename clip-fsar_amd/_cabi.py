"""What the ctypes bindings (hip, gallery_hip, gallery_text_hip, stream_hip, pool_hip, ingest_hip, live_hip, groups_hip, lastblock_hip, enroll_hip, live_text_hip and
the extension tier's class_smooth_hip, the add-on tier's events_hip and the plug-in tier's baseline_hip and shortlist_hip) share: loading a
C-ABI library against its signature table, the builders of their ``_check`` / ``_shape`` helpers, and the descriptor table that seven of
them pass (class_smooth_hip, events_hip, baseline_hip and shortlist_hip too).  Each binding keeps its own SIGNATURES, ABI_VERSION, LIB_PATH and ``lib()``."""
from __future__ import annotations

import collections
import ctypes
import os


def load(lib_path, signatures, prefix, abi_version, what):
    """CDLL(lib_path) with every name of ``signatures`` resolved (argtypes set, int return), ``<prefix>last_error`` typed, and the library's
    ``<prefix>abi_version()`` equal to ``abi_version``.  Raises when the library is not built (``what``: what has no fallback) or stale."""
    if not os.path.exists(lib_path):
        raise RuntimeError("clip_fsar_amd: %s is missing -- build it with `python clip-fsar_amd/build.py` (hipcc --offload-arch=gfx950).  "
                           "There is no CPU/PyTorch fallback for %s." % (lib_path, what))
    L = ctypes.CDLL(lib_path)
    for name, args in signatures.items():
        fn = getattr(L, name)
        fn.argtypes = args
        fn.restype = ctypes.c_int
    last_error = getattr(L, prefix + "last_error")
    last_error.restype = ctypes.c_char_p
    last_error.argtypes = []
    built = getattr(L, prefix + "abi_version")()
    if built != abi_version:
        raise RuntimeError("clip_fsar_amd: %s has ABI revision %d, this binding was written against %d -- rebuild it "
                           "(python clip-fsar_amd/build.py --force)" % (lib_path, built, abi_version))
    return L


def checker(lib, prefix):
    """_check(rc, what): a non-zero return code raises with the library's message"""
    def _check(rc, what):
        if rc != 0:
            raise RuntimeError("%s failed: %s" % (what, getattr(lib(), prefix + "last_error")().decode(errors="replace")))
    return _check


def shape_checker(module):
    """_shape(t, shape, name): a tensor of another shape raises"""
    def _shape(t, shape, name):
        if tuple(t.shape) != tuple(shape):
            raise RuntimeError("clip_fsar_amd.%s: %s has shape %s, expected %s" % (module, name, tuple(t.shape), tuple(shape)))
    return _shape


Table = collections.namedtuple("Table", "host dev S")          # host: pinned [S, cols] int32 rows; dev: their device copy


def table_args(t, cols, module):
    """(host pointer, device pointer, S) of a Table of ``cols`` values per row, as the table_host / table_dev / S arguments of a call"""
    import torch
    from .hip import _dev
    if not isinstance(t, Table) or t.host.is_cuda or t.host.dtype != torch.int32 or tuple(t.host.shape) != (t.S, cols) \
            or not t.host.is_contiguous() or tuple(t.dev.shape) != (t.S, cols):
        raise RuntimeError("clip_fsar_amd.%s: table must be a Table of [S, %d] int32 host rows and their device copy" % (module, cols))
    return ctypes.c_void_p(t.host.data_ptr()), _dev(t.dev, torch.int32, "table"), t.S
