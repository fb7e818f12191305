"""CPU: the text half of the support gallery (libclipfsar_gallery_text.so, include/clipfsar_gallery_text.h) sizes its workspace and validates
arguments without a GPU; TextGallery resolves its mode from the head's flags as the head does.  Its exports, kernels and place in the build
are checked with every library's in tests/test_build_recipe.py."""
import ctypes
from types import SimpleNamespace as NS

import pytest

from _abi import check_exports, lib_row


@pytest.fixture(scope="module")
def tlib():
    import __graft_entry__ as ge
    ge.build()                                    # builds every library (no-op when up to date)
    from clip_fsar_amd import gallery_text_hip
    return gallery_text_hip.lib()


def test_header_exported_exactly_and_arity_matches(tlib):
    check_exports(lib_row("gallery_text"))


def test_workspace_size(tlib):
    assert tlib.cfgt_workspace_floats(10, 64) == 20
    assert tlib.cfgt_workspace_floats(10, 65) == 40
    assert tlib.cfgt_workspace_floats(4096, 10000) == 4096 * 157 * 2
    assert tlib.cfgt_workspace_floats(0, 5) == -1 and tlib.cfgt_workspace_floats(5, 0) == -1
    assert tlib.cfgt_workspace_floats(2 ** 30, 2 ** 20) == -1


def test_argument_validation_without_gpu(tlib):
    p = ctypes.c_void_p(4096)                     # never dereferenced: every call below fails validation before any device work
    L = tlib
    assert L.cfgt_frame_mean(None, p, 4, 8, 64, None) != 0 and b"null" in L.cfgt_last_error()
    for N, T, E in ((0, 8, 64), (4, 0, 64), (4, -1, 64), (4, 1025, 64), (4, 8, 0)):
        assert L.cfgt_frame_mean(p, p, N, T, E, None) != 0, (N, T, E)
        assert b"bad shape" in L.cfgt_last_error()
    assert L.cfgt_text_logits(p, p, p, p, None, p, p, 4, 4, 64, None) != 0 and b"null" in L.cfgt_last_error()
    assert L.cfgt_text_logits(p, p, p, p, p, p, None, 4, 4, 64, None) != 0 and b"null" in L.cfgt_last_error()
    for NQ, C, E in ((0, 4, 64), (4, 0, 64), (4, 4, 66), (4, 4, 0), (4, 4, 8196)):
        assert L.cfgt_text_logits(p, p, p, p, p, p, p, NQ, C, E, None) != 0, (NQ, C, E)
        assert b"bad shape" in L.cfgt_last_error()
    assert L.cfgt_text_logits(ctypes.c_void_p(4100), p, p, p, p, p, p, 4, 4, 64, None) != 0 and b"aligned" in L.cfgt_last_error()
    assert L.cfgt_text_logits(p, p, p, p, p, p, p, 65536 * 64, 4, 64, None) != 0 and b"too large" in L.cfgt_last_error()
    assert L.cfgt_text_softmax(p, None, p, 4, 4, None) != 0 and b"null" in L.cfgt_last_error()
    assert L.cfgt_text_softmax(p, p, p, 4, 0, None) != 0 and b"bad shape" in L.cfgt_last_error()
    assert L.cfgt_text_combine(p, p, None, p, 4, 4, 0.9, None) != 0 and b"null" in L.cfgt_last_error()
    assert L.cfgt_text_combine(p, p, p, p, 0, 4, 0.9, None) != 0 and b"bad shape" in L.cfgt_last_error()
    for coff in (float("nan"), float("inf"), -float("inf")):
        assert L.cfgt_text_combine(p, p, p, p, 4, 4, coff, None) != 0 and b"finite" in L.cfgt_last_error()


def test_python_wrappers_reject_cpu_tensors(tlib):
    import torch
    from clip_fsar_amd import gallery_text_hip as gt
    with pytest.raises(RuntimeError, match="HIP device tensor"):
        gt.frame_mean(torch.zeros(2, 4, 8), torch.zeros(2, 8))
    with pytest.raises(RuntimeError, match="shape"):
        gt.frame_mean(torch.zeros(2, 4, 8), torch.zeros(2, 9))


# ------------------------------------------------------------------ mode resolution (no GPU: a stub head)
def _stub_head(**train):
    engine = NS(arch={"embed": 8})
    return NS(args=NS(TRAIN=NS(**train), DATA=NS(NUM_INPUT_FRAMES=4)), _get_engine=lambda dev: engine, _engine_key=("stub",),
              arch_name="stub", precision="fp32", depth=1)


def test_text_gallery_mode_resolution():
    from clip_fsar_amd.text_gallery import TextGallery, resolve_mode, text_coff
    with pytest.raises(ValueError, match="neither"):
        TextGallery(_stub_head(), "cpu")
    with pytest.raises(ValueError, match="contradicts"):
        TextGallery(_stub_head(EVAL_TEXT=True), "cpu", mode="combine")
    with pytest.raises(ValueError, match="contradicts"):
        TextGallery(_stub_head(COMBINE=True), "cpu", mode="eval_text")
    with pytest.raises(ValueError, match="mode must be"):
        TextGallery(_stub_head(), "cpu", mode="otam")
    assert TextGallery(_stub_head(EVAL_TEXT=True, COMBINE=True), "cpu").mode == "eval_text"        # the head's precedence
    assert TextGallery(_stub_head(EVAL_TEXT=True, COMBINE=True), "cpu", mode="eval_text").mode == "eval_text"
    assert TextGallery(_stub_head(COMBINE=True), "cpu").mode == "combine"
    assert TextGallery(_stub_head(), "cpu", mode="combine").mode == "combine"            # explicit mode on a default-branch head
    assert TextGallery(_stub_head(EVAL_TEXT=False, COMBINE=False), "cpu", mode="eval_text").mode == "eval_text"
    assert resolve_mode(NS(TRAIN=NS(COMBINE=1))) == "combine"
    assert text_coff(NS(TRAIN=NS())) == 0.9 and text_coff(NS(TRAIN=NS(TEXT_COFF=0))) == 0.9
    assert text_coff(NS(TRAIN=NS(TEXT_COFF=0.5))) == 0.5
    g = TextGallery(_stub_head(COMBINE=True, TEXT_COFF=0.5), "cpu")
    assert g.fingerprint()["mode"] == "combine" and g.fingerprint()["text_coff"] == 0.5 and len(g) == 0


def test_combine_gallery_refuses_text_only_classes():
    from clip_fsar_amd.text_gallery import TextGallery
    g = TextGallery(_stub_head(COMBINE=True), "cpu")
    with pytest.raises(ValueError, match="COMBINE"):
        g.add_text_classes([1, 2])


def test_support_gallery_points_to_text_gallery():
    from clip_fsar_amd.gallery import SupportGallery
    for flag in ("EVAL_TEXT", "COMBINE"):
        with pytest.raises(NotImplementedError, match="TextGallery"):
            SupportGallery(_stub_head(**{flag: True}), "cpu")
