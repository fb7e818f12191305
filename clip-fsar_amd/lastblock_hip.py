"""ctypes binding of libclipfsar_lastblock.so (C ABI and the algebra in include/clipfsar_lastblock.h): the class-token attention of the
last ViT block without its K | V projection -- key fold, class attend, value fold (HipViT, option fold_last_kv).

A library and a signature table of their own, like clip_fsar_amd.groups_hip: contiguous HIP device tensors only (no CPU path), launches
on the current stream of the operands' device, a non-zero return code raises with the library's message.
"""
from __future__ import annotations

import os

import torch  # noqa: F401  (imported first so that torch's HIP runtime is the one the library binds to)

import ctypes

from . import _cabi, hip

ABI_VERSION = 1          # CFLB_ABI_VERSION of include/clipfsar_lastblock.h this file's SIGNATURES were written against
LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libclipfsar_lastblock.so")
MAX_HEADS = 16           # CFLB_MAX_HEADS
FRAME_BATCH = 16         # CFLB_FRAME_BATCH
TOKEN_CHUNK = 32         # CFLB_TOKEN_CHUNK
BF16, F16 = 1, 2         # CFLB_BF16, CFLB_F16
_lib = None

_c_int, _c_p, _c_f = ctypes.c_int, ctypes.c_void_p, ctypes.c_float

# symbol -> argtypes; must match include/clipfsar_lastblock.h (tests/test_build_recipe.py cross-checks against the header text)
SIGNATURES = {
    "cflb_version": [],
    "cflb_abi_version": [],
    "cflb_key_fold": [_c_p, _c_int, _c_p, _c_p, _c_p, _c_int, _c_int, _c_int, _c_p],
    "cflb_class_attend": [_c_p, _c_p, _c_p, _c_p, _c_int, _c_p, _c_f, _c_p, _c_int, _c_int, _c_int, _c_int, _c_p],
    "cflb_value_fold": [_c_p, _c_p, _c_p, _c_p, _c_int, _c_int, _c_int, _c_int, _c_p],
}


def lib():
    """Load (once) and return the ctypes handle.  Raises when the library is not built."""
    global _lib
    if _lib is None:
        _lib = _cabi.load(LIB_PATH, SIGNATURES, "cflb_", ABI_VERSION, "the folded last-block attention")
    return _lib


_check = _cabi.checker(lib, "cflb_")
_shape = _cabi.shape_checker("lastblock_hip")
_dev, _stream = hip._dev, hip._stream


def _code(dtype):
    if dtype == torch.bfloat16:
        return BF16
    if dtype == torch.float16:
        return F16
    raise RuntimeError("clip_fsar_amd.lastblock_hip: q / oc must be bf16 or fp16, got %s" % dtype)


def key_weight(wk, heads):
    """Wk' [D, D] (rows [D:2D] of the LN-folded QKV weights, fp16) -> wk_t [heads, D, 64] with wk_t[h, k, j] = Wk'[64 h + j, k]: layout
    only, made once when the weights are loaded"""
    D = wk.shape[1]
    _shape(wk, (64 * heads, D), "wk")
    return wk.view(heads, 64, D).transpose(1, 2).contiguous()


def key_fold(q, wk_t, g, G):
    """q [F, D] (bf16 | fp16), wk_t [heads, D, 64] fp16 -> g [F, heads, D] fp16 = (1/8) Wk'_h^T q_h, G [F, heads] fp32 = its column sums"""
    F_, D = q.shape
    heads = wk_t.shape[0]
    _shape(wk_t, (heads, D, 64), "wk_t")
    _shape(g, (F_, heads, D), "g")
    _shape(G, (F_, heads), "G")
    _check(lib().cflb_key_fold(_dev(q, None, "q"), _code(q.dtype), _dev(wk_t, torch.float16, "wk_t"), _dev(g, torch.float16, "g"),
                               _dev(G, torch.float32, "G"), F_, D, heads, _stream()), "cflb_key_fold")


def class_attend(x, g, G, z, ntok, partial=None, rowstats=None, eps=1e-5):
    """x [>= F ntok, D] fp16 (the raw stream), g, G of key_fold, the rows' statistics as partial [>= F ntok, slots, 2] or rowstats
    [>= F ntok, 4] (exactly one) -> z [F, heads, D] fp32"""
    F_, heads, D = g.shape
    M = F_ * ntok
    if x.dim() != 2 or x.shape[1] != D or x.shape[0] < M:
        raise RuntimeError("clip_fsar_amd.lastblock_hip: x has shape %s, expected [>= %d, %d]" % (tuple(x.shape), M, D))
    _shape(G, (F_, heads), "G")
    _shape(z, (F_, heads, D), "z")
    slots = 0
    if partial is not None:
        if partial.dim() != 3 or partial.shape[0] < M or partial.shape[2] != 2:
            raise RuntimeError("clip_fsar_amd.lastblock_hip: partial has shape %s, expected [>= %d, slots, 2]" % (tuple(partial.shape), M))
        slots = partial.shape[1]
    if rowstats is not None and (rowstats.dim() != 2 or rowstats.shape[0] < M or rowstats.shape[1] != 4):
        raise RuntimeError("clip_fsar_amd.lastblock_hip: rowstats has shape %s, expected [>= %d, 4]" % (tuple(rowstats.shape), M))
    _check(lib().cflb_class_attend(_dev(x, torch.float16, "x"), _dev(g, torch.float16, "g"), _dev(G, torch.float32, "G"),
                                   hip._opt(partial, torch.float32, "partial"), slots, hip._opt(rowstats, torch.float32, "rowstats"),
                                   float(eps), _dev(z, torch.float32, "z"), F_, int(ntok), D, heads, _stream()), "cflb_class_attend")


def value_fold(z, wv, d_v, oc):
    """z [F, heads, D] fp32, wv [D, D] fp16 (Wv'), d_v [D] fp32 -> oc [F, D] (bf16 | fp16) = Wv'_h z_h + d_v per head"""
    F_, heads, D = z.shape
    _shape(wv, (D, D), "wv")
    _shape(d_v, (D,), "d_v")
    _shape(oc, (F_, D), "oc")
    _check(lib().cflb_value_fold(_dev(z, torch.float32, "z"), _dev(wv, torch.float16, "wv"), _dev(d_v, torch.float32, "d_v"),
                                 _dev(oc, None, "oc"), _code(oc.dtype), F_, D, heads, _stream()), "cflb_value_fold")
