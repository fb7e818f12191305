"""CPU: the text half of the support gallery (libclipfsar_gallery_text.so, include/clipfsar_gallery_text.h) builds beside the other two
libraries, exports exactly its header, validates arguments without a GPU, keeps its kernels out of scratch; TextGallery resolves its mode
from the head's flags as the head does."""
import ctypes
import json
import os
import re
from types import SimpleNamespace as NS

import pytest

from _abi import _exported, _other_reports, _prototypes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "clipfsar_gallery_text.h")


@pytest.fixture(scope="module")
def tlib():
    import __graft_entry__ as ge
    ge.build()                                    # builds all three libraries (no-op when up to date)
    from clip_fsar_amd import gallery_text_hip
    return gallery_text_hip.lib()


def test_header_exported_exactly_and_arity_matches(tlib):
    from clip_fsar_amd import gallery_text_hip as gt
    protos = _prototypes(HEADER, "cfgt_")
    assert len(protos) == 8, protos
    assert _exported(gt.LIB_PATH) == set(protos), sorted(_exported(gt.LIB_PATH) ^ set(protos))
    for name, nargs in protos.items():
        if name == "cfgt_last_error":
            continue
        assert len(gt.SIGNATURES[name]) == nargs, (name, len(gt.SIGNATURES[name]), nargs)
    assert set(gt.SIGNATURES) | {"cfgt_last_error"} == set(protos)
    assert tlib.cfgt_abi_version() == gt.ABI_VERSION and tlib.cfgt_version() >= 100
    m = re.search(r"#define CFGT_ABI_VERSION (\d+)", open(HEADER).read())
    assert int(m.group(1)) == gt.ABI_VERSION


def test_other_libraries_keep_their_export_sets(tlib):
    from clip_fsar_amd import gallery_hip, gallery_text_hip
    ours = _exported(gallery_text_hip.LIB_PATH)
    assert not any(s.startswith(("cfsg_", "cfsar_")) for s in ours)
    assert not any(s.startswith("cfgt_") for s in _exported(gallery_hip.LIB_PATH))


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


def test_kernels_use_no_scratch_and_stay_out_of_the_other_reports(tlib):
    from clip_fsar_amd import build as b
    if not os.path.exists(b.SIDE_LIBS["gallery_text"].usage):
        b.build_side("gallery_text", force=True, verbose=False)
    usage = json.load(open(b.SIDE_LIBS["gallery_text"].usage))
    names = sorted(usage)
    for k in ("frame_mean_kernel", "text_logits_kernel", "text_softmax_kernel", "text_combine_kernel"):
        assert sum(k in n for n in names) == 1, (k, names)
    for n, u in usage.items():
        assert u.get("scratch", 0) == 0, (n, u)
        assert "otam_gallery_kernel" not in n, n
    assert b.SIDE_LIBS["gallery_text"].source not in b.SOURCES
    for other in _other_reports("gallery_text"):
        if os.path.exists(other):
            assert not set(usage) & set(json.load(open(other)))


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
