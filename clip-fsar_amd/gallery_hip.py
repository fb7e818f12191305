"""ctypes binding of libclipfsar_gallery.so (C ABI declared in include/clipfsar_gallery.h): the support gallery's kernels.

A library and a signature table of their own: ``hip.lib()`` resolves every name of ``hip.SIGNATURES`` against the product library,
which keeps exactly the entry points of include/clipfsar_hip.h.  Same conventions as clip_fsar_amd.hip: contiguous HIP device tensors
only (no CPU path), launches on the current stream of the operands' device, a non-zero return code raises with the library's message.
"""
from __future__ import annotations

import ctypes
import os

import torch  # noqa: F401  (imported first so that torch's HIP runtime is the one the library binds to)

from . import _cabi, hip

ABI_VERSION = 1          # CFSG_ABI_VERSION of include/clipfsar_gallery.h this file's SIGNATURES were written against
LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libclipfsar_gallery.so")
TOPK_MAX = 16
_lib = None

_c_int, _c_p, _c_f = ctypes.c_int, ctypes.c_void_p, ctypes.c_float

# symbol -> argtypes; must match include/clipfsar_gallery.h (tests/test_build_recipe.py cross-checks against the header text)
SIGNATURES = {
    "cfsg_version": [],
    "cfsg_abi_version": [],
    "cfsg_support_sequences": [_c_p, _c_p, _c_p, _c_p] + [_c_int] * 4 + [_c_p],
    "cfsg_segment_mean": [_c_p, _c_p, _c_p] + [_c_int] * 5 + [_c_p],
    "cfsg_row_norms": [_c_p, _c_p, _c_int, _c_int, _c_p],
    "cfsg_otam_gallery": [_c_p] * 6 + [_c_int] * 4 + [_c_f, _c_int, _c_p],
    "cfsg_topk": [_c_p, _c_p, _c_p, _c_int, _c_int, _c_int, _c_p],
}


def lib():
    """Load (once) and return the ctypes handle.  Raises when the library is not built."""
    global _lib
    if _lib is None:
        _lib = _cabi.load(LIB_PATH, SIGNATURES, "cfsg_", ABI_VERSION, "the gallery")
    return _lib


_check = _cabi.checker(lib, "cfsg_")
_shape = _cabi.shape_checker("gallery_hip")
_dev, _stream = hip._dev, hip._stream


def support_sequences(feats, text, cls_of_video, X):
    """feats [Nv, T, E], text [n_cls, E] fp32, cls_of_video [Nv] int32 -> X [Nv, T+1, E]: T frame rows, then the video's class text row."""
    Nv, T, E = feats.shape
    _shape(text, (text.shape[0], E), "text")
    _shape(cls_of_video, (Nv,), "cls_of_video")
    _shape(X, (Nv, T + 1, E), "X")
    _check(lib().cfsg_support_sequences(_dev(feats, torch.float32, "feats"), _dev(text, torch.float32, "text"),
                                        _dev(cls_of_video, torch.int32, "cls_of_video"), _dev(X, torch.float32, "X"), Nv, T, E,
                                        text.shape[0], _stream()), "cfsg_support_sequences")


def segment_mean(X, offsets, out):
    """X [Nv, L, E], offsets [C+1] int32 (device) -> out [C, rows_kept, E]: mean of rows 0 .. rows_kept-1 over each class's run of videos."""
    Nv, L, E = X.shape
    C = offsets.shape[0] - 1
    if out.dim() != 3 or out.shape[0] != C or out.shape[2] != E:
        raise RuntimeError("clip_fsar_amd.gallery_hip: out must be [%d, rows_kept, %d], got %s" % (C, E, tuple(out.shape)))
    _check(lib().cfsg_segment_mean(_dev(X, torch.float32, "X"), _dev(offsets, torch.int32, "offsets"), _dev(out, torch.float32, "out"),
                                   Nv, L, E, C, out.shape[1], _stream()), "cfsg_segment_mean")


def row_norms(X, n):
    """X [..., E] -> n [rows]: L2 norm of every row."""
    E = X.shape[-1]
    R = X.numel() // E
    _shape(n, (R,), "n")
    _check(lib().cfsg_row_norms(_dev(X, torch.float32, "X"), _dev(n, torch.float32, "n"), R, E, _stream()), "cfsg_row_norms")


def otam_gallery(Xq, qn, P, pn, logits, lbda=0.5, single_direct=False, dists_out=None):
    """Xq [NQ, T, E], qn [NQ*T], P [C, T, E], pn [C*T] -> logits [NQ, C] = -(OTAM(d) + OTAM(d^T)), d = 1 - cos_sim (eps 0.01 on the
    product of norms); dists_out (optional) [NQ, C, T, T]."""
    NQ, T, E = Xq.shape
    C = P.shape[0]
    _shape(P, (C, T, E), "P")
    _shape(qn, (NQ * T,), "qn")
    _shape(pn, (C * T,), "pn")
    _shape(logits, (NQ, C), "logits")
    if dists_out is not None:
        _shape(dists_out, (NQ, C, T, T), "dists_out")
    _check(lib().cfsg_otam_gallery(_dev(Xq, torch.float32, "Xq"), _dev(qn, torch.float32, "qn"), _dev(P, torch.float32, "P"),
                                   _dev(pn, torch.float32, "pn"), _dev(logits, torch.float32, "logits"),
                                   None if dists_out is None else _dev(dists_out, torch.float32, "dists_out"), NQ, C, T, E, float(lbda),
                                   int(bool(single_direct)), _stream()), "cfsg_otam_gallery")


def topk(logits, k, values, index):
    """logits [NQ, C] -> values [NQ, k] (descending), index [NQ, k] int32; ties to the lower class index."""
    NQ, C = logits.shape
    _shape(values, (NQ, k), "values")
    _shape(index, (NQ, k), "index")
    _check(lib().cfsg_topk(_dev(logits, torch.float32, "logits"), _dev(values, torch.float32, "values"), _dev(index, torch.int32, "index"),
                           NQ, C, int(k), _stream()), "cfsg_topk")
