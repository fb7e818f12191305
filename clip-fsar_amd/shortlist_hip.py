"""ctypes binding of libclipfsar_shortlist.so (C ABI declared in include/ext/clipfsar_shortlist.h): the coarse stage of
clip_fsar_amd.shortlist.Shortlist -- one [E] row per sequence (the mean of its unit-normalised rows), the coarse scores of every
(query, class) pair as one exact-fp32 GEMM, and the selection that writes per-group slot lists on the device, where
clip_fsar_amd.groups_hip.otam_grouped reads them.

A library and a signature table of their own, like clip_fsar_amd.baseline_hip: contiguous HIP device tensors only (no CPU path), launches
on the current stream of the operands' device, a non-zero return code raises with the library's message.  The group table of select, one
row (Q0, NQ) per group, travels twice as the other tables do: the library validates the host rows and the kernel reads the device copy
(pool_hip.TableUploader, here with this library's two columns).
"""
from __future__ import annotations

import ctypes
import os

import torch  # noqa: F401  (imported first so that torch's HIP runtime is the one the library binds to)

from . import _cabi, hip
from .pool_hip import TableUploader

ABI_VERSION = 1          # CFSH_ABI_VERSION of include/ext/clipfsar_shortlist.h this file's SIGNATURES were written against
LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libclipfsar_shortlist.so")
MAX_T = 32               # CFSH_MAX_T
MAX_KEEP = 4096          # CFSH_MAX_KEEP
MAX_GROUPS = 65536       # CFSH_MAX_GROUPS
NONE = 0x7fffffff        # CFSH_NONE: sel_cols of a place without a column (its sel_slots is -1)
TINY = 1e-12             # CFSH_TINY
TABLE_COLS = 2           # CFSH_TABLE_COLS; the columns, in order:
Q0, NQ = range(TABLE_COLS)
_lib = None

_c_int, _c_p = ctypes.c_int, ctypes.c_void_p

# symbol -> argtypes; must match include/ext/clipfsar_shortlist.h (tests/test_shortlist_abi.py cross-checks against the header text)
SIGNATURES = {
    "cfsh_version": [],
    "cfsh_abi_version": [],
    "cfsh_mean_unit_rows": [_c_p] * 4 + [_c_int] * 4 + [_c_p],
    "cfsh_coarse_scores": [_c_p] * 4 + [_c_int] * 4 + [_c_p],
    "cfsh_workspace_floats": [_c_int, _c_int],
    "cfsh_select": [_c_p] * 4 + [_c_int] * 4 + [_c_p] * 4,
}


def lib():
    """Load (once) and return the ctypes handle.  Raises when the library is not built."""
    global _lib
    if _lib is None:
        _lib = _cabi.load(LIB_PATH, SIGNATURES, "cfsh_", ABI_VERSION, "the shortlist's coarse stage")
    return _lib


_check = _cabi.checker(lib, "cfsh_")
_shape = _cabi.shape_checker("shortlist_hip")
_dev, _stream = hip._dev, hip._stream

Table = _cabi.Table


def table_rows(counts):
    """the group table of counts[i] consecutive queries per group: rows of (Q0, NQ), and the number of queries"""
    rows, q = [], 0
    for n in counts:
        rows.append([q, n])
        q += n
    return rows, q


def table_uploader(device, max_rows, depth=4):
    """pool_hip.TableUploader with this library's row layout"""
    return TableUploader(device, max_rows, depth=depth, cols=TABLE_COLS)


def workspace_floats(G, NC):
    """floats of select's `work` for G groups over NC columns"""
    n = lib().cfsh_workspace_floats(int(G), int(NC))
    if n < 0:
        raise RuntimeError("clip_fsar_amd.shortlist_hip: no workspace for G=%d groups x NC=%d columns (1 <= G <= %d, NC >= 1, G * NC < 2^31)"
                           % (G, NC, MAX_GROUPS))
    return n


def mean_unit_rows(X, norms, slots, out):
    """X [cap, T, E], norms [cap * T], out [cap, E]: out[b] = the mean over t of X[b, t] / max(norms[b * T + t], TINY) for every block b
    of slots [n] int32 (device), or for every block when slots is None.  A slot outside [0, cap) writes nothing.  One launch."""
    cap, T, E = X.shape
    _shape(norms, (cap * T,), "norms")
    _shape(out, (cap, E), "out")
    if slots is not None and slots.dim() != 1:
        raise RuntimeError("clip_fsar_amd.shortlist_hip: slots has shape %s, expected [n]" % (tuple(slots.shape),))
    n = cap if slots is None else slots.shape[0]
    _check(lib().cfsh_mean_unit_rows(_dev(X, torch.float32, "X"), _dev(norms, torch.float32, "norms"),
                                     None if slots is None else _dev(slots, torch.int32, "slots"), _dev(out, torch.float32, "out"),
                                     n, cap, T, E, _stream()), "cfsh_mean_unit_rows")


def coarse_scores(U, C_store, cols, S):
    """U [NQ, E], C_store [cap, E], cols [NC] int32 (device) -> S [NQ, NC]: S[q, j] = <U[q], C_store[cols[j]]>; a slot outside [0, cap)
    gives a column of NaN.  One launch."""
    NQ_, E = U.shape
    cap = C_store.shape[0]
    _shape(C_store, (cap, E), "C_store")
    if cols.dim() != 1:
        raise RuntimeError("clip_fsar_amd.shortlist_hip: cols has shape %s, expected [NC]" % (tuple(cols.shape),))
    _shape(S, (NQ_, cols.shape[0]), "S")
    _check(lib().cfsh_coarse_scores(_dev(U, torch.float32, "U"), _dev(C_store, torch.float32, "C_store"), _dev(cols, torch.int32, "cols"),
                                    _dev(S, torch.float32, "S"), NQ_, cols.shape[0], cap, E, _stream()), "cfsh_coarse_scores")


def select(S, cols, table, keep, sel_cols, sel_slots, work):
    """S [NQ, NC], cols [NC] int32, table: a row (Q0, NQ) per group -> sel_cols, sel_slots [G, K] int32, K = min(keep, NC): per group
    the K columns with the best group score (the maximum over the group's queries), in ascending column order, and their slots
    cols[column]; places without a column hold NONE and -1 (clip_fsar_amd.shortlist.reference_select restates the rule).  work: at least
    workspace_floats(G, NC) floats.  One launch."""
    NQ_, NC = S.shape
    K = min(int(keep), NC)
    _shape(cols, (NC,), "cols")
    G = table.S if isinstance(table, Table) else 0
    _shape(sel_cols, (G, K), "sel_cols")
    _shape(sel_slots, (G, K), "sel_slots")
    if work.dim() != 1 or work.shape[0] < G * NC:
        raise RuntimeError("clip_fsar_amd.shortlist_hip: work has shape %s, expected [>= %d]" % (tuple(work.shape), G * NC))
    th, td, G = _cabi.table_args(table, TABLE_COLS, "shortlist_hip")
    _check(lib().cfsh_select(_dev(S, torch.float32, "S"), _dev(cols, torch.int32, "cols"), th, td, G, NQ_, NC, int(keep),
                             _dev(sel_cols, torch.int32, "sel_cols"), _dev(sel_slots, torch.int32, "sel_slots"),
                             _dev(work, torch.float32, "work"), _stream()), "cfsh_select")
