"""CPU: the support-gallery library (libclipfsar_gallery.so, include/clipfsar_gallery.h) validates arguments without a GPU and its wrappers
reject misuse; its exports, kernels and place in the build are checked with every library's in tests/test_build_recipe.py."""
import ctypes

import pytest

from _abi import check_exports, lib_row


@pytest.fixture(scope="module")
def glib():
    import __graft_entry__ as ge
    ge.build()                                    # builds every library (no-op when up to date)
    from clip_fsar_amd import gallery_hip
    return gallery_hip.lib()


def test_gallery_header_exported_exactly_and_arity_matches(glib):
    check_exports(lib_row("gallery"))


def test_argument_validation_without_gpu(glib):
    p = ctypes.c_void_p(4096)                     # never dereferenced: every call below fails validation before any device work
    assert glib.cfsg_otam_gallery(None, p, p, p, p, None, 4, 4, 8, 64, 0.5, 0, None) != 0
    assert b"null" in glib.cfsg_last_error()
    for NQ, C, T, E in ((0, 4, 8, 64), (4, 0, 8, 64), (4, 4, 33, 64), (4, 4, 8, 66), (4, 4, 0, 64), (4, 4, 8, 0)):
        assert glib.cfsg_otam_gallery(p, p, p, p, p, None, NQ, C, T, E, 0.5, 0, None) != 0, (NQ, C, T, E)
        assert b"bad shape" in glib.cfsg_last_error()
    assert glib.cfsg_otam_gallery(p, p, p, p, p, None, 4, 4, 8, 64, 0.0, 0, None) != 0
    assert b"lambda" in glib.cfsg_last_error()
    assert glib.cfsg_topk(p, p, p, 4, 10, 17, None) != 0 and b"bad shape" in glib.cfsg_last_error()
    assert glib.cfsg_topk(p, p, p, 4, 10, 11, None) != 0
    assert glib.cfsg_topk(p, p, p, 4, 70000, 5, None) != 0
    assert glib.cfsg_topk(None, p, p, 4, 10, 5, None) != 0 and b"null" in glib.cfsg_last_error()
    assert glib.cfsg_support_sequences(p, p, None, p, 3, 8, 64, 5, None) != 0 and b"null" in glib.cfsg_last_error()
    assert glib.cfsg_support_sequences(p, p, p, p, 0, 8, 64, 5, None) != 0
    assert glib.cfsg_segment_mean(p, p, p, 3, 9, 64, 2, 10, None) != 0 and b"bad shape" in glib.cfsg_last_error()   # rows_kept > L
    assert glib.cfsg_segment_mean(p, None, p, 3, 9, 64, 2, 8, None) != 0
    assert glib.cfsg_row_norms(p, p, 0, 64, None) != 0 and glib.cfsg_row_norms(None, p, 4, 64, None) != 0


def test_python_wrappers_reject_cpu_tensors(glib):
    import torch
    from clip_fsar_amd import gallery_hip
    with pytest.raises(RuntimeError, match="HIP device tensor"):
        gallery_hip.row_norms(torch.zeros(4, 8), torch.zeros(4))


def test_gallery_refuses_text_modes_without_gpu():
    from types import SimpleNamespace as NS
    from clip_fsar_amd.gallery import SupportGallery
    for flag in ("EVAL_TEXT", "COMBINE"):
        head = NS(args=NS(TRAIN=NS(**{flag: True}), DATA=NS(NUM_INPUT_FRAMES=8)))
        with pytest.raises(NotImplementedError, match=flag):
            SupportGallery(head, "cuda")
