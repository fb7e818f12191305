"""CPU: the support-gallery library (libclipfsar_gallery.so, include/clipfsar_gallery.h) builds beside the product library, exports exactly its
header, validates arguments without a GPU, keeps its hot kernel out of scratch; the product library keeps exactly its 48 entry points."""
import ctypes
import json
import os

import pytest

from _abi import _exported, _other_reports, _prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "clipfsar_gallery.h")
HIP_HEADER = os.path.join(ROOT, "include", "clipfsar_hip.h")


@pytest.fixture(scope="module")
def glib():
    import __graft_entry__ as ge
    ge.build()                                    # builds both libraries (no-op when up to date)
    from clip_fsar_amd import gallery_hip
    return gallery_hip.lib()


def test_gallery_header_exported_exactly_and_arity_matches(glib):
    from clip_fsar_amd import gallery_hip
    protos = _prototypes(HEADER, "cfsg_")
    assert len(protos) == 8, protos
    assert _exported(gallery_hip.LIB_PATH) == set(protos), sorted(_exported(gallery_hip.LIB_PATH) ^ set(protos))
    for name, nargs in protos.items():
        if name == "cfsg_last_error":
            continue
        assert name in gallery_hip.SIGNATURES, name
        assert len(gallery_hip.SIGNATURES[name]) == nargs, (name, len(gallery_hip.SIGNATURES[name]), nargs)
    assert set(gallery_hip.SIGNATURES) | {"cfsg_last_error"} == set(protos)
    assert glib.cfsg_abi_version() == gallery_hip.ABI_VERSION and glib.cfsg_version() >= 100


def test_product_library_still_exports_exactly_its_48_symbols(glib):
    from clip_fsar_amd import hip
    if os.environ.get("CFSAR_DEV", "0") == "1":
        pytest.skip("developer build")
    protos = _prototypes(HIP_HEADER, "cfsar_")
    assert len(protos) == 48
    ours = _exported(hip.LIB_PATH)
    assert ours == set(protos), sorted(ours ^ set(protos))
    assert not any(s.startswith("cfsg_") for s in ours)
    assert not any(n.startswith("cfsg_") for n in hip.SIGNATURES)


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


def test_gallery_kernels_use_no_scratch_and_stay_out_of_the_product_report(glib):
    from clip_fsar_amd import build as b
    if not os.path.exists(b.SIDE_LIBS["gallery"].usage):
        b.build_side("gallery", force=True, verbose=False)
    usage = json.load(open(b.SIDE_LIBS["gallery"].usage))
    otam = [n for n in usage if "otam_gallery_kernel" in n]
    assert len(otam) == 3, sorted(usage)                  # T = 8, T = 16, run-time T
    for n, u in usage.items():
        assert u.get("scratch", 0) == 0, (n, u)
    assert b.SIDE_LIBS["gallery"].source not in b.SOURCES and b.SIDE_LIBS["gallery"].usage != b.USAGE
    for other in _other_reports("gallery"):
        if os.path.exists(other):
            assert not any("otam_gallery_kernel" in n for n in json.load(open(other))) and not set(usage) & set(json.load(open(other))), other


def test_gallery_refuses_text_modes_without_gpu():
    from types import SimpleNamespace as NS
    from clip_fsar_amd.gallery import SupportGallery
    for flag in ("EVAL_TEXT", "COMBINE"):
        head = NS(args=NS(TRAIN=NS(**{flag: True}), DATA=NS(NUM_INPUT_FRAMES=8)))
        with pytest.raises(NotImplementedError, match=flag):
            SupportGallery(head, "cuda")
