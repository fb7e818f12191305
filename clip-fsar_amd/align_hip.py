"""ctypes binding of libclipfsar_align.so (C ABI declared in include/ext/clipfsar_align.h): the OTAM soft alignment behind a score -- per
(query, store slot) pair the T x T cosine distances, the logit and the gradient of the soft-min DP with respect to the distances
(clip_fsar_amd.align.Aligner, StreamPool.explain).

A library and a signature table of their own, like clip_fsar_amd.pool_select_hip: contiguous HIP device tensors only (no CPU path), the
launch on the current stream of the operands' device, a non-zero return code raises with the library's message.  The pair lists are
device tensors: nothing of a call is read on the host.
"""
from __future__ import annotations

import ctypes
import os

import torch  # noqa: F401  (imported first so that torch's HIP runtime is the one the library binds to)

from . import _cabi, hip

ABI_VERSION = 1          # CFAL_ABI_VERSION of include/ext/clipfsar_align.h this file's SIGNATURES were written against
LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libclipfsar_align.so")
MAX_T = 32               # CFAL_MAX_T
MIN_E = 4                # CFAL_MIN_E
MAX_E = 8192             # CFAL_MAX_E
_lib = None

_c_int, _c_p, _c_float = ctypes.c_int, ctypes.c_void_p, ctypes.c_float

# symbol -> argtypes; must match include/ext/clipfsar_align.h (tests/test_align_abi.py cross-checks against the header text)
SIGNATURES = {
    "cfal_version": [],
    "cfal_abi_version": [],
    "cfal_align": [_c_p] * 6 + [_c_int] * 5 + [_c_float, _c_int] + [_c_p] * 4,
}


def lib():
    """Load (once) and return the ctypes handle.  Raises when the library is not built."""
    global _lib
    if _lib is None:
        _lib = _cabi.load(LIB_PATH, SIGNATURES, "cfal_", ABI_VERSION, "the OTAM alignment")
    return _lib


_check = _cabi.checker(lib, "cfal_")
_shape = _cabi.shape_checker("align_hip")
_dev, _stream = hip._dev, hip._stream


def align(Xq, qn, P, pn, pair_q, pair_slot, lam, single_direct, plan, dists, logits):
    """Xq [NQ, T, E], qn [NQ * T], P [cap, T, E], pn [cap * T] fp32; pair_q, pair_slot [NP] int32 (device): pair i is query pair_q[i]
    against store slot pair_slot[i] -> plan [NP, T, T], dists [NP, T, T] (or None), logits [NP] fp32: the pair's soft alignment
    G(D) + G(D^T)^T (G(D) with single_direct), its cosine distances D and its logit -(F(D) + F(D^T)); a pair whose query or slot lies
    outside the inputs is never dereferenced and NaN in every output (clip_fsar_amd.align.reference_alignment restates the arithmetic).
    One launch."""
    NQ, T, E = Xq.shape
    cap = P.shape[0]
    NP = pair_q.shape[0]
    _shape(P, (cap, T, E), "P")
    _shape(qn, (NQ * T,), "qn")
    _shape(pn, (cap * T,), "pn")
    _shape(pair_q, (NP,), "pair_q")
    _shape(pair_slot, (NP,), "pair_slot")
    _shape(plan, (NP, T, T), "plan")
    if dists is not None:
        _shape(dists, (NP, T, T), "dists")
    _shape(logits, (NP,), "logits")
    f32, i32 = torch.float32, torch.int32
    _check(lib().cfal_align(_dev(Xq, f32, "Xq"), _dev(qn, f32, "qn"), _dev(P, f32, "P"), _dev(pn, f32, "pn"), _dev(pair_q, i32, "pair_q"),
                            _dev(pair_slot, i32, "pair_slot"), NP, NQ, cap, T, E, float(lam), int(bool(single_direct)),
                            _dev(plan, f32, "plan"), None if dists is None else _dev(dists, f32, "dists"), _dev(logits, f32, "logits"),
                            _stream()), "cfal_align")
