"""ctypes binding of libclipfsar_gallery_text.so (C ABI declared in include/clipfsar_gallery_text.h): the EVAL_TEXT / COMBINE kernels of the
support gallery.

A library and a signature table of their own, like clip_fsar_amd.gallery_hip: contiguous HIP device tensors only (no CPU path), launches on
the current stream of the operands' device, a non-zero return code raises with the library's message.
"""
from __future__ import annotations

import ctypes
import os

import torch  # noqa: F401  (imported first so that torch's HIP runtime is the one the library binds to)

from . import _cabi, hip

ABI_VERSION = 1          # CFGT_ABI_VERSION of include/clipfsar_gallery_text.h this file's SIGNATURES were written against
LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libclipfsar_gallery_text.so")
_lib = None

_c_int, _c_p, _c_f = ctypes.c_int, ctypes.c_void_p, ctypes.c_float

# symbol -> argtypes; must match include/clipfsar_gallery_text.h (tests/test_build_recipe.py cross-checks against the header text)
SIGNATURES = {
    "cfgt_version": [],
    "cfgt_abi_version": [],
    "cfgt_workspace_floats": [_c_int, _c_int],
    "cfgt_frame_mean": [_c_p, _c_p, _c_int, _c_int, _c_int, _c_p],
    "cfgt_text_logits": [_c_p] * 7 + [_c_int] * 3 + [_c_p],
    "cfgt_text_softmax": [_c_p] * 3 + [_c_int] * 2 + [_c_p],
    "cfgt_text_combine": [_c_p] * 4 + [_c_int] * 2 + [_c_f, _c_p],
}


def lib():
    """Load (once) and return the ctypes handle.  Raises when the library is not built."""
    global _lib
    if _lib is None:
        _lib = _cabi.load(LIB_PATH, SIGNATURES, "cfgt_", ABI_VERSION, "the text gallery")
    return _lib


_check = _cabi.checker(lib, "cfgt_")
_shape = _cabi.shape_checker("gallery_text_hip")
_dev, _stream = hip._dev, hip._stream


def _aligned(t, name):
    if t.data_ptr() % 16:
        raise RuntimeError("clip_fsar_amd.gallery_text_hip: %s must start on a 16-byte boundary (float4 loads)" % name)


def workspace_floats(NQ, C):
    """floats of the softmax-partials workspace of text_logits for NQ queries x C classes"""
    n = lib().cfgt_workspace_floats(int(NQ), int(C))
    if n < 0:
        raise RuntimeError("clip_fsar_amd.gallery_text_hip: no workspace for NQ=%d C=%d" % (NQ, C))
    return n


def _check_partials(partials, NQ, C):
    if partials.dim() != 1 or partials.numel() < workspace_floats(NQ, C):
        raise RuntimeError("clip_fsar_amd.gallery_text_hip: partials must be 1-D with at least %d floats" % workspace_floats(NQ, C))


def frame_mean(feats, out):
    """feats [N, T, E] -> out [N, E]: the mean over T (summed in t order, then / T)."""
    N, T, E = feats.shape
    _shape(out, (N, E), "out")
    _check(lib().cfgt_frame_mean(_dev(feats, torch.float32, "feats"), _dev(out, torch.float32, "out"), N, T, E, _stream()), "cfgt_frame_mean")


def text_logits(emb, en, text, tn, scale, logits, partials):
    """emb [NQ, E], en [NQ], text [C, E], tn [C], scale [1] (device) -> logits [NQ, C] = scale * (dot / en / tn), partials
    [workspace_floats(NQ, C)] (at least) = per-(query, 64-class tile) softmax statistics."""
    NQ, E = emb.shape
    C = text.shape[0]
    _shape(text, (C, E), "text")
    _shape(en, (NQ,), "en")
    _shape(tn, (C,), "tn")
    _shape(scale, (1,), "scale")
    _shape(logits, (NQ, C), "logits")
    _check_partials(partials, NQ, C)
    p_emb, p_text = _dev(emb, torch.float32, "emb"), _dev(text, torch.float32, "text")
    _aligned(emb, "emb")
    _aligned(text, "text")
    _check(lib().cfgt_text_logits(p_emb, _dev(en, torch.float32, "en"), p_text, _dev(tn, torch.float32, "tn"),
                                  _dev(scale, torch.float32, "scale"), _dev(logits, torch.float32, "logits"),
                                  _dev(partials, torch.float32, "partials"), NQ, C, E, _stream()), "cfgt_text_logits")


def text_softmax(logits, partials, probs):
    """logits [NQ, C] + partials (from text_logits) -> probs [NQ, C] = the softmax over the C classes (probs may be logits)."""
    NQ, C = logits.shape
    _shape(probs, (NQ, C), "probs")
    _check_partials(partials, NQ, C)
    _check(lib().cfgt_text_softmax(_dev(logits, torch.float32, "logits"), _dev(partials, torch.float32, "partials"),
                                   _dev(probs, torch.float32, "probs"), NQ, C, _stream()), "cfgt_text_softmax")


def text_combine(logits, partials, visual, out, coff):
    """logits [NQ, C] + partials (from text_logits), visual [NQ, C] (OTAM logits) -> out [NQ, C] = p^coff * softmax((8 + v) / 8)^(1 - coff)
    (out may be logits)."""
    NQ, C = logits.shape
    _shape(visual, (NQ, C), "visual")
    _shape(out, (NQ, C), "out")
    _check_partials(partials, NQ, C)
    _check(lib().cfgt_text_combine(_dev(logits, torch.float32, "logits"), _dev(partials, torch.float32, "partials"),
                                   _dev(visual, torch.float32, "visual"), _dev(out, torch.float32, "out"), NQ, C, float(coff), _stream()),
           "cfgt_text_combine")
