"""ctypes binding of libclipfsar_stream.so (C ABI declared in include/clipfsar_stream.h): the ring, gather and smoothing kernels of
clip_fsar_amd.stream.WindowStream.

A library and a signature table of their own, like clip_fsar_amd.gallery_hip: contiguous HIP device tensors only (no CPU path), launches on
the current stream of the operands' device, a non-zero return code raises with the library's message.
"""
from __future__ import annotations

import ctypes
import os

import torch  # noqa: F401  (imported first so that torch's HIP runtime is the one the library binds to)

from . import _cabi, hip

ABI_VERSION = 1          # CFSS_ABI_VERSION of include/clipfsar_stream.h this file's SIGNATURES were written against
LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libclipfsar_stream.so")
MAX_T = 32               # CFSS_MAX_T
_lib = None

_c_int, _c_p, _c_f, _c_i64 = ctypes.c_int, ctypes.c_void_p, ctypes.c_float, ctypes.c_int64

# symbol -> argtypes; must match include/clipfsar_stream.h (tests/test_build_recipe.py cross-checks against the header text)
SIGNATURES = {
    "cfss_version": [],
    "cfss_abi_version": [],
    "cfss_ring_put": [_c_p, _c_p] + [_c_int] * 4 + [_c_i64, _c_p],
    "cfss_window_sequences": [_c_p, _c_p] + [_c_int] * 7 + [_c_i64, _c_i64, _c_p],
    "cfss_smooth_logits": [_c_p] * 3 + [_c_int] * 3 + [_c_f, _c_i64, _c_p],
}


def lib():
    """Load (once) and return the ctypes handle.  Raises when the library is not built."""
    global _lib
    if _lib is None:
        _lib = _cabi.load(LIB_PATH, SIGNATURES, "cfss_", ABI_VERSION, "window streams")
    return _lib


_check = _cabi.checker(lib, "cfss_")
_shape = _cabi.shape_checker("stream_hip")
_dev, _stream = hip._dev, hip._stream


def ring_put(feats, ring, first_frame):
    """feats [B, n, E] -> ring [B, cap, E]: ring[b, (first_frame + i) mod cap] = feats[b, i]; n <= cap."""
    B, n, E = feats.shape
    _shape(ring, (B, ring.shape[1], E), "ring")
    _check(lib().cfss_ring_put(_dev(feats, torch.float32, "feats"), _dev(ring, torch.float32, "ring"), B, n, E, ring.shape[1],
                               int(first_frame), _stream()), "cfss_ring_put")


def window_sequences(ring, X, n_windows, T, stride, rate, first_window, frames_pushed):
    """ring [B, cap, E] -> X [B * n_windows, T, E] (at least: a larger X is written in its first rows): window first_window + w of stream b
    = frames (first_window + w) * stride + j * rate.  Raises when a frame is not pushed yet or already overwritten."""
    B, cap, E = ring.shape
    if X.dim() != 3 or X.shape[0] < B * n_windows or tuple(X.shape[1:]) != (T, E):
        raise RuntimeError("clip_fsar_amd.stream_hip: X has shape %s, expected [>= %d, %d, %d]" % (tuple(X.shape), B * n_windows, T, E))
    _check(lib().cfss_window_sequences(_dev(ring, torch.float32, "ring"), _dev(X, torch.float32, "X"), B, int(n_windows), int(T), E, cap,
                                       int(stride), int(rate), int(first_window), int(frames_pushed), _stream()), "cfss_window_sequences")


def smooth_logits(logits, state, out, alpha, windows_seen):
    """logits [B, nW, C] (windows windows_seen ...), state [B, C] (y of the window before; not read when windows_seen == 0; receives the
    last y) -> out [B, nW, C]: y_0 = x_0, y_k = fmaf(alpha, y_{k-1}, (1 - alpha) * x_k).  out may be logits."""
    B, nW, C = logits.shape
    _shape(state, (B, C), "state")
    _shape(out, (B, nW, C), "out")
    _check(lib().cfss_smooth_logits(_dev(logits, torch.float32, "logits"), _dev(state, torch.float32, "state"),
                                    _dev(out, torch.float32, "out"), B, nW, C, float(alpha), int(windows_seen), _stream()),
           "cfss_smooth_logits")
