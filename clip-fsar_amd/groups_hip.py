"""ctypes binding of libclipfsar_groups.so (C ABI declared in include/clipfsar_groups.h): cos_sim + OTAM and top-k of a ragged list of
groups -- each group of queries against its own list of store slots -- in one launch each (LiveGallery.classify_grouped, the per-session
class lists of StreamPool).

A library and a signature table of their own, like clip_fsar_amd.live_hip: contiguous HIP device tensors only (no CPU path), launches on
the current stream of the operands' device, a non-zero return code raises with the library's message.

The descriptor table, one row per group, travels twice, as the pool's does (include/clipfsar_groups.h): the library validates the host
rows and the kernels read the device copy.  pool_hip.TableUploader makes both, here with this library's row layout.
"""
from __future__ import annotations

import ctypes
import os

import torch  # noqa: F401  (imported first so that torch's HIP runtime is the one the library binds to)

from . import _cabi, hip
from .pool_hip import TableUploader

ABI_VERSION = 1          # CFGR_ABI_VERSION of include/clipfsar_groups.h this file's SIGNATURES were written against
LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libclipfsar_groups.so")
MAX_T = 32               # CFGR_MAX_T
MAX_GROUPS = 65536       # CFGR_MAX_GROUPS
TOPK_MAX = 16            # CFGR_TOPK_MAX
TABLE_COLS = 6           # CFGR_TABLE_COLS; the columns, in order:
Q0, NQ, C0, NC, TILE0, OUT0 = range(TABLE_COLS)
_lib = None

_c_int, _c_p, _c_f = ctypes.c_int, ctypes.c_void_p, ctypes.c_float

# symbol -> argtypes; must match include/clipfsar_groups.h (tests/test_build_recipe.py cross-checks against the header text)
SIGNATURES = {
    "cfgr_version": [],
    "cfgr_abi_version": [],
    "cfgr_otam_grouped": [_c_p] * 8 + [_c_int] * 7 + [_c_f, _c_int, _c_p],
    "cfgr_topk_grouped": [_c_p] * 3 + [_c_int] * 4 + [_c_p] * 3,
}


def lib():
    """Load (once) and return the ctypes handle.  Raises when the library is not built."""
    global _lib
    if _lib is None:
        _lib = _cabi.load(LIB_PATH, SIGNATURES, "cfgr_", ABI_VERSION, "grouped scoring")
    return _lib


_check = _cabi.checker(lib, "cfgr_")
_shape = _cabi.shape_checker("groups_hip")
_dev, _stream = hip._dev, hip._stream


def tile_videos(T):
    """QB: the videos along each side of a tile (tile_videos of csrc/otam_tile.h)"""
    return min(64 // T, 16)


def table_rows(counts, widths, T):
    """The descriptor table of groups of counts[i] queries against lists of widths[i] slots, packed in order: rows of
    (Q0, NQ, C0, NC, TILE0, OUT0), and the totals (NQ, NCOLS, tiles, NOUT)."""
    qb = tile_videos(T)
    rows, q, c, tiles, out = [], 0, 0, 0, 0
    for n, w in zip(counts, widths):
        rows.append([q, n, c, w, tiles, out])
        q, c, out = q + n, c + w, out + n * w
        tiles += -(-n // qb) * -(-w // qb)
    return rows, (q, c, tiles, out)


def table_uploader(device, max_rows, depth=4):
    """pool_hip.TableUploader with this library's row layout"""
    return TableUploader(device, max_rows, depth=depth, cols=TABLE_COLS)


def _table(t):
    return _cabi.table_args(t, TABLE_COLS, "groups_hip")


def otam_grouped(Xq, qn, P_store, pn_store, cols, logits, table, n_out, lbda=0.5, single_direct=False):
    """Xq [NQ, T, E], qn [NQ*T], P_store [cap, T, E], pn_store [cap*T], cols [NCOLS] int32 (device), table: a row per group -> logits
    [>= n_out] flat (its first n_out values are written): group g's [NQ_g, NC_g] block at OUT0_g holds what live_hip.otam_indexed gives
    for its queries and its part of cols, bit for bit."""
    NQ_, T, E = Xq.shape
    cap = P_store.shape[0]
    if cols.dim() != 1:
        raise RuntimeError("clip_fsar_amd.groups_hip: cols has shape %s, expected [NCOLS]" % (tuple(cols.shape),))
    if logits.dim() != 1 or logits.shape[0] < n_out:
        raise RuntimeError("clip_fsar_amd.groups_hip: logits has shape %s, expected [>= %d]" % (tuple(logits.shape), n_out))
    _shape(P_store, (cap, T, E), "P_store")
    _shape(qn, (NQ_ * T,), "qn")
    _shape(pn_store, (cap * T,), "pn_store")
    th, td, G = _table(table)
    _check(lib().cfgr_otam_grouped(_dev(Xq, torch.float32, "Xq"), _dev(qn, torch.float32, "qn"), _dev(P_store, torch.float32, "P_store"),
                                   _dev(pn_store, torch.float32, "pn_store"), _dev(cols, torch.int32, "cols"),
                                   _dev(logits, torch.float32, "logits"), th, td, G, NQ_, cols.shape[0], int(n_out), cap, T, E,
                                   float(lbda), int(bool(single_direct)), _stream()), "cfgr_otam_grouped")


def topk_grouped(logits, table, n_queries, n_out, k, values, index):
    """logits [>= n_out] flat as otam_grouped wrote it -> values [NQ, k] (descending), index [NQ, k] int32 into each query's own group's
    list; ties to the lower index."""
    if logits.dim() != 1 or logits.shape[0] < n_out:
        raise RuntimeError("clip_fsar_amd.groups_hip: logits has shape %s, expected [>= %d]" % (tuple(logits.shape), n_out))
    _shape(values, (n_queries, k), "values")
    _shape(index, (n_queries, k), "index")
    th, td, G = _table(table)
    _check(lib().cfgr_topk_grouped(_dev(logits, torch.float32, "logits"), th, td, G, int(n_queries), int(n_out), int(k),
                                   _dev(values, torch.float32, "values"), _dev(index, torch.int32, "index"), _stream()),
           "cfgr_topk_grouped")
