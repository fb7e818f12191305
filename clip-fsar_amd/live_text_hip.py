"""ctypes binding of libclipfsar_live_text.so (C ABI declared in include/clipfsar_live_text.h): the EVAL_TEXT / COMBINE eval branches of
a ragged list of groups -- each group of queries against its own list of slots of a text-row store, both softmaxes over that list -- in
one launch each (clip_fsar_amd.live_text_gallery.LiveTextGallery).

A library and a signature table of their own, like clip_fsar_amd.groups_hip: contiguous HIP device tensors only (no CPU path), launches
on the current stream of the operands' device, a non-zero return code raises with the library's message.

The descriptor table, one row per group, travels twice, as groups_hip's does: the library validates the host rows and the kernels read
the device copy.  pool_hip.TableUploader makes both, here with this library's row layout.
"""
from __future__ import annotations

import ctypes
import os

import torch  # noqa: F401  (imported first so that torch's HIP runtime is the one the library binds to)

from . import _cabi, hip
from .pool_hip import TableUploader

ABI_VERSION = 1          # CFLT_ABI_VERSION of include/clipfsar_live_text.h this file's SIGNATURES were written against
LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libclipfsar_live_text.so")
MAX_GROUPS = 65536       # CFLT_MAX_GROUPS
TILE = 64                # queries and classes along a tile
TABLE_COLS = 8           # CFLT_TABLE_COLS; the columns, in order:
Q0, NQ, C0, NC, TILE0, OUT0, PART0, PAD = range(TABLE_COLS)
_lib = None

_c_int, _c_p, _c_f = ctypes.c_int, ctypes.c_void_p, ctypes.c_float

# symbol -> argtypes; must match include/clipfsar_live_text.h (tests/test_build_recipe.py cross-checks against the header text)
SIGNATURES = {
    "cflt_version": [],
    "cflt_abi_version": [],
    "cflt_workspace_floats": [_c_p, _c_int],
    "cflt_text_logits_grouped": [_c_p] * 10 + [_c_int] * 7 + [_c_p],
    "cflt_text_softmax_grouped": [_c_p] * 5 + [_c_int] * 4 + [_c_p],
    "cflt_text_combine_grouped": [_c_p] * 6 + [_c_int] * 4 + [_c_f, _c_p],
}


def lib():
    """Load (once) and return the ctypes handle.  Raises when the library is not built."""
    global _lib
    if _lib is None:
        _lib = _cabi.load(LIB_PATH, SIGNATURES, "cflt_", ABI_VERSION, "grouped text scoring")
    return _lib


_check = _cabi.checker(lib, "cflt_")
_shape = _cabi.shape_checker("live_text_hip")
_dev, _stream = hip._dev, hip._stream


def table_rows(counts, widths):
    """The descriptor table of groups of counts[i] queries against lists of widths[i] slots, packed in order: rows of
    (Q0, NQ, C0, NC, TILE0, OUT0, PART0, 0), and the totals (NQ, NCOLS, tiles, NOUT, NPART)."""
    rows, q, c, tiles, out, part = [], 0, 0, 0, 0, 0
    for n, w in zip(counts, widths):
        rows.append([q, n, c, w, tiles, out, part, 0])
        ct = -(-w // TILE)
        q, c, out = q + n, c + w, out + n * w
        tiles += -(-n // TILE) * ct
        part += n * ct
    return rows, (q, c, tiles, out, part)


def n_partials(rows):
    """NPART of a table: the (max, sum) pairs its groups own"""
    return sum(r[NQ] * -(-r[NC] // TILE) for r in rows)


def table_uploader(device, max_rows, depth=4):
    """pool_hip.TableUploader with this library's row layout"""
    return TableUploader(device, max_rows, depth=depth, cols=TABLE_COLS)


def _table(t):
    return _cabi.table_args(t, TABLE_COLS, "live_text_hip")


def workspace_floats(table):
    """floats of the softmax-partials workspace of text_logits_grouped under `table`: 2 per (query, 64-class tile of its group)"""
    th, _, G = _table(table)
    n = lib().cflt_workspace_floats(th, G)
    if n < 0:
        raise RuntimeError("clip_fsar_amd.live_text_hip: no workspace for this table (a negative count, an empty list or beyond 2^31)")
    return n


def _aligned(t, name):
    if t.data_ptr() % 16:
        raise RuntimeError("clip_fsar_amd.live_text_hip: %s must start on a 16-byte boundary (float4 loads)" % name)


def _flat(t, n, name):
    if t.dim() != 1 or t.shape[0] < n:
        raise RuntimeError("clip_fsar_amd.live_text_hip: %s has shape %s, expected [>= %d]" % (name, tuple(t.shape), n))


def text_logits_grouped(emb, en, text_store, tn_store, cols, scale, logits, partials, table, n_out, n_part):
    """emb [NQ, E], en [NQ], text_store [cap, E], tn_store [cap], cols [NCOLS] int32 (device), scale [1] (device), table: a row per
    group -> logits [>= n_out] flat (its first n_out values are written): group g's [NQ_g, NC_g] block at OUT0_g holds what
    gallery_text_hip.text_logits gives for its queries against text_store[its part of cols], bit for bit; partials [>= 2 * n_part]."""
    NQ_, E = emb.shape
    cap = text_store.shape[0]
    if cols.dim() != 1:
        raise RuntimeError("clip_fsar_amd.live_text_hip: cols has shape %s, expected [NCOLS]" % (tuple(cols.shape),))
    _flat(logits, n_out, "logits")
    _flat(partials, 2 * n_part, "partials")
    _shape(text_store, (cap, E), "text_store")
    _shape(en, (NQ_,), "en")
    _shape(tn_store, (cap,), "tn_store")
    _shape(scale, (1,), "scale")
    p_emb, p_text = _dev(emb, torch.float32, "emb"), _dev(text_store, torch.float32, "text_store")
    _aligned(emb, "emb")
    _aligned(text_store, "text_store")
    th, td, G = _table(table)
    _check(lib().cflt_text_logits_grouped(p_emb, _dev(en, torch.float32, "en"), p_text, _dev(tn_store, torch.float32, "tn_store"),
                                          _dev(cols, torch.int32, "cols"), _dev(scale, torch.float32, "scale"),
                                          _dev(logits, torch.float32, "logits"), _dev(partials, torch.float32, "partials"), th, td, G,
                                          NQ_, cols.shape[0], int(n_out), int(n_part), cap, E, _stream()), "cflt_text_logits_grouped")


def text_softmax_grouped(logits, partials, probs, table, n_queries, n_out, n_part):
    """logits [>= n_out] + partials (from text_logits_grouped under the same table) -> probs [>= n_out]: every group's rows softmaxed
    over the group's own list (probs may be logits)."""
    _flat(logits, n_out, "logits")
    _flat(probs, n_out, "probs")
    _flat(partials, 2 * n_part, "partials")
    th, td, G = _table(table)
    _check(lib().cflt_text_softmax_grouped(_dev(logits, torch.float32, "logits"), _dev(partials, torch.float32, "partials"),
                                           _dev(probs, torch.float32, "probs"), th, td, G, int(n_queries), int(n_out), int(n_part),
                                           _stream()), "cflt_text_softmax_grouped")


def text_combine_grouped(logits, partials, visual, out, table, n_queries, n_out, n_part, coff):
    """logits [>= n_out] + partials, visual [>= n_out] (groups_hip.otam_grouped's logits for the same groups) -> out [>= n_out] =
    p^coff * softmax((8 + v) / 8)^(1 - coff), both softmaxes over each group's own list (out may be logits)."""
    _flat(logits, n_out, "logits")
    _flat(visual, n_out, "visual")
    _flat(out, n_out, "out")
    _flat(partials, 2 * n_part, "partials")
    th, td, G = _table(table)
    _check(lib().cflt_text_combine_grouped(_dev(logits, torch.float32, "logits"), _dev(partials, torch.float32, "partials"),
                                           _dev(visual, torch.float32, "visual"), _dev(out, torch.float32, "out"), th, td, G,
                                           int(n_queries), int(n_out), int(n_part), float(coff), _stream()), "cflt_text_combine_grouped")
