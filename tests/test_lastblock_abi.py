"""CPU: the last-block library (libclipfsar_lastblock.so, include/clipfsar_lastblock.h) validates its arguments without a GPU and its wrappers
reject misuse.  Its exports, kernels and place in the build are checked with every library's in tests/test_build_recipe.py."""
import ctypes
import os
import re

import pytest

from _abi import _prototypes, check_abi_at_load, check_exports, lib_row

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "clipfsar_lastblock.h")


@pytest.fixture(scope="module")
def llib():
    import __graft_entry__ as ge
    ge.build()                                    # builds every library (no-op when up to date)
    from clip_fsar_amd import lastblock_hip
    return lastblock_hip.lib()


def test_header_exported_exactly_and_arity_matches(llib):
    check_exports(lib_row("lastblock"))                 # the checks every library gets; below, what is particular to this one
    from clip_fsar_amd import lastblock_hip as lb
    protos = _prototypes(HEADER, "cflb_")
    assert protos["cflb_key_fold"] == 9 and protos["cflb_class_attend"] == 13 and protos["cflb_value_fold"] == 9
    text = open(HEADER).read()
    assert int(re.search(r"#define CFLB_MAX_HEADS (\d+)", text).group(1)) == lb.MAX_HEADS == 16
    assert int(re.search(r"#define CFLB_FRAME_BATCH (\d+)", text).group(1)) == lb.FRAME_BATCH
    assert int(re.search(r"#define CFLB_TOKEN_CHUNK (\d+)", text).group(1)) == lb.TOKEN_CHUNK
    assert int(re.search(r"#define CFLB_BF16 (\d+)", text).group(1)) == lb.BF16
    assert int(re.search(r"#define CFLB_F16 (\d+)", text).group(1)) == lb.F16


def test_abi_version_is_checked_at_load(llib, monkeypatch):
    check_abi_at_load(lib_row("lastblock"), monkeypatch)


# ------------------------------------------------------------------ argument validation, without a GPU
def test_argument_validation_without_gpu(llib):
    p = ctypes.c_void_p(4096)                     # never dereferenced: every call below fails validation before any device work
    err = llib.cflb_last_error

    # key_fold(q, dtype, wk_t, g, G, F, D, heads, stream)
    def key(q=p, dtype=1, wk_t=p, g=p, G=p, F=3, D=768, heads=12):
        return llib.cflb_key_fold(q, dtype, wk_t, g, G, F, D, heads, None)

    # class_attend(x, g, G, partial, slots, rowstats, eps, z, F, ntok, D, heads, stream)
    def attend(x=p, g=p, G=p, partial=p, slots=12, rowstats=None, eps=1e-5, z=p, F=3, ntok=197, D=768, heads=12):
        return llib.cflb_class_attend(x, g, G, partial, slots, rowstats, eps, z, F, ntok, D, heads, None)

    # value_fold(z, wv, d_v, oc, dtype, F, D, heads, stream)
    def value(z=p, wv=p, d_v=p, oc=p, dtype=1, F=3, D=768, heads=12):
        return llib.cflb_value_fold(z, wv, d_v, oc, dtype, F, D, heads, None)

    for call, ptrs in ((key, ("q", "wk_t", "g", "G")), (attend, ("x", "g", "G", "z")), (value, ("z", "wv", "d_v", "oc"))):
        for name in ptrs:
            assert call(**{name: None}) != 0 and b"null pointer" in err(), (call.__name__, name)
        for kw in ({"D": 704}, {"D": 768, "heads": 11}, {"D": 1088, "heads": 17}, {"D": 0, "heads": 0}, {"F": 0}, {"F": -1}):
            assert call(**kw) != 0 and b"bad shape" in err(), (call.__name__, kw)
    for call in (key, value):
        for dtype in (0, 3):
            assert call(dtype=dtype) != 0 and b"bad dtype" in err(), (call.__name__, dtype)
    assert key(q=ctypes.c_void_p(4104)) != 0 and b"16-byte aligned" in err()
    assert value(wv=ctypes.c_void_p(4100)) != 0 and b"16-byte aligned" in err()
    for ntok in (0, -5):
        assert attend(ntok=ntok) != 0 and b"ntok >= 1" in err(), ntok
    assert attend(F=1 << 20, ntok=1 << 12) != 0 and b"below 2^31" in err()
    assert attend(partial=p, rowstats=p) != 0 and b"exactly one" in err()          # both statistics forms
    assert attend(partial=None, rowstats=None, slots=0) != 0 and b"exactly one" in err()          # neither
    for slots in (0, 17, -1):
        assert attend(slots=slots) != 0 and b"slots" in err(), slots
    assert attend(partial=None, rowstats=p, slots=12) != 0 and b"slots" in err()
    assert attend(eps=0.0) != 0 and b"eps" in err()
    assert attend(x=ctypes.c_void_p(4104)) != 0 and b"16-byte aligned" in err()


def test_python_wrappers_reject_cpu_tensors_and_bad_shapes(llib):
    import torch
    from clip_fsar_amd import lastblock_hip as lb
    F_, H, D, N = 2, 2, 128, 5
    q, wk = torch.zeros(F_, D, dtype=torch.bfloat16), torch.zeros(D, D, dtype=torch.float16)
    g, G, z = torch.zeros(F_, H, D, dtype=torch.float16), torch.zeros(F_, H), torch.zeros(F_, H, D)
    x, rs = torch.zeros(F_ * N, D, dtype=torch.float16), torch.zeros(F_ * N, 4)
    wk_t = lb.key_weight(wk, H)
    assert tuple(wk_t.shape) == (H, D, 64) and wk_t.is_contiguous()
    w = torch.arange(D * D, dtype=torch.float32).reshape(D, D)
    assert torch.equal(lb.key_weight(w, H)[1, 7, 5], w[64 + 5, 7])
    with pytest.raises(RuntimeError, match="HIP device tensor"):
        lb.key_fold(q, wk_t, g, G)
    with pytest.raises(RuntimeError, match="shape"):
        lb.key_fold(q, wk_t, g[:, :1], G)
    with pytest.raises(RuntimeError, match="HIP device tensor"):
        lb.class_attend(x, g, G, z, N, rowstats=rs)
    with pytest.raises(RuntimeError, match="x has shape"):
        lb.class_attend(x[:-1], g, G, z, N, rowstats=rs)
    with pytest.raises(RuntimeError, match="rowstats has shape"):
        lb.class_attend(x, g, G, z, N, rowstats=rs[:, :3])
    with pytest.raises(RuntimeError, match="partial has shape"):
        lb.class_attend(x, g, G, z, N, partial=torch.zeros(F_ * N, 2, 3))
    with pytest.raises(RuntimeError, match="HIP device tensor"):
        lb.value_fold(z, wk, torch.zeros(D), torch.zeros(F_, D, dtype=torch.bfloat16))
    with pytest.raises(RuntimeError, match="bf16 or fp16"):
        lb._code(torch.float32)


def test_the_option_is_a_constructor_argument_of_the_bf16_mode():
    from clip_fsar_amd.engine import HipViT
    assert HipViT.OPTIONS["fold_last_kv"] is True
    src = open(os.path.join(ROOT, "clip-fsar_amd", "engine.py")).read()
    assert 'precision == "bf16"' in src[src.index("self.fold_last_kv = "):][:200]
