"""What the ABI tests (test_abi, test_build_recipe, test_<side library>_abi) share: the prototypes a C header declares, the symbols a built
library exports, and LIBS, the one table of the eleven libraries -- the product library and every name of build.SIDE_LIBS, in build order.
tests/test_build_recipe.py runs its checks over every row (check_exports and check_abi_at_load are here because the per-library files
call them for their own row too); a new library is one name in build.SIDE_LIBS and one row here."""
import collections
import importlib
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

#   name:    "product", or the library's name in build.SIDE_LIBS
#   module:  its ctypes binding in clip_fsar_amd
#   prefix:  what every exported symbol starts with, and no symbol of another library
#   header:  its C ABI under include/
#   exports: the exact set of exported names (prefix + each word)
#   kernels: {fragment of a kernel's name: how many kernels of the resource report carry it}; total: the number of kernels in that report.
#            The product library's report is checked by tests/test_abi.py (scratch budgets), so its row lists none.
Lib = collections.namedtuple("Lib", "name module prefix header exports kernels total")


def _row(name, module, prefix, header, exports, kernels=None, total=None):
    return Lib(name, module, prefix, header, frozenset(prefix + e for e in exports.split()), kernels, total)


LIBS = [
    _row("product", "hip", "cfsar_", "clipfsar_hip.h",
         "version abi_version last_error attnpool_attend attnpool_tokens avgpool2x2_nhwc build_sequences class_text_logits cls_rows cls_rows_ex "
         "combine_logits conv3x3_nhwc copy_rows_strided cos_otam_logits embed_finish_pair embed_tokens episode_top1 f16_pair_to_f32 "
         "frame_col_means frame_gemm gather_rows gemm gemm_ex gemm_lnfold gemm_lnfold_heads gemm_lnfold_hp gemm_lnfold_partials "
         "gemm_residual_stats gemm_residual_stats_heads gemm_residual_wide im2col3x3_nhwc im2col_patches im2col_patches_split layernorm "
         "layernorm_ex ln_stats_finalize nchw_to_nhwc patch_embed preprocess_frames prototypes row_stats seq_attention stem_conv3x3_s2 "
         "text_match_probs vit_attention vit_attention_cls vit_attention_means vit_attention_pair"),
    _row("gallery", "gallery_hip", "cfsg_", "clipfsar_gallery.h",
         "version abi_version last_error otam_gallery topk row_norms segment_mean support_sequences",
         {"otam_gallery_kernel": 3, "topk_kernel": 1, "row_norms_kernel": 1, "segment_mean_kernel": 1, "support_sequences_kernel": 1}, 7),
    _row("gallery_text", "gallery_text_hip", "cfgt_", "clipfsar_gallery_text.h",
         "version abi_version last_error workspace_floats frame_mean text_logits text_softmax text_combine",
         {"frame_mean_kernel": 1, "text_logits_kernel": 1, "text_softmax_kernel": 1, "text_combine_kernel": 1}, 4),
    _row("stream", "stream_hip", "cfss_", "clipfsar_stream.h",
         "version abi_version last_error ring_put window_sequences smooth_logits",
         {"ring_put_kernel": 2, "window_sequences_kernel": 2, "smooth_logits_kernel": 1}, 5),          # 16-byte and 4-byte forms
    _row("pool", "pool_hip", "cfsp_", "clipfsar_pool.h",
         "version abi_version last_error ring_put window_sequences smooth_logits",
         {"pool_ring_put_kernel": 2, "pool_window_sequences_kernel": 2, "pool_smooth_logits_kernel": 1}, 5),
    _row("ingest", "ingest_hip", "cfsi_", "clipfsar_ingest.h",
         "version abi_version last_error transform_frames",
         {"ingest_transform_kernel": 2}, 2),                                                            # 16-byte and 4-byte stores
    _row("live", "live_hip", "cfsl_", "clipfsar_live.h",
         "version abi_version last_error otam_indexed accumulate slot_norms",
         {"otam_indexed_kernel": 3, "slot_norms_kernel": 1, "accumulate_kernel": 1}, 5),              # T = 8, T = 16, run-time T
    _row("groups", "groups_hip", "cfgr_", "clipfsar_groups.h",
         "version abi_version last_error otam_grouped topk_grouped",
         {"otam_grouped_kernel": 3, "topk_grouped_kernel": 1}, 4),
    _row("lastblock", "lastblock_hip", "cflb_", "clipfsar_lastblock.h",
         "version abi_version last_error key_fold class_attend value_fold",
         {"key_fold_kernel": 2, "value_fold_kernel": 2, "class_attend_kernel": 3}, 7),                # bf16 / fp16; up to 2, 12 and 16 heads
    _row("enroll", "enroll_hip", "cfen_", "clipfsar_enroll.h",
         "version abi_version last_error ring_sequences",
         {"ring_sequences_kernel": 2}, 2),                                                              # 16-byte and 4-byte pieces
    _row("live_text", "live_text_hip", "cflt_", "clipfsar_live_text.h",
         "version abi_version last_error workspace_floats text_logits_grouped text_softmax_grouped text_combine_grouped",
         {"text_logits_grouped_kernel": 1, "text_softmax_grouped_kernel": 1, "text_combine_grouped_kernel": 1}, 3),
]
SIDE = LIBS[1:]


def lib_row(name):
    return next(row for row in LIBS if row.name == name)


def _binding(row):
    return importlib.import_module("clip_fsar_amd." + row.module)


def _prototypes(path, prefix):
    """{entry point: number of arguments} of the `int` / `const char*` prototypes named <prefix>... in the header at path"""
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    protos = {}
    for m in re.finditer(r"(?:int|const char\*)\s*(%s\w+)\s*\(([^;]*?)\)\s*;" % prefix, text, flags=re.S):
        args = m.group(2).strip()
        protos[m.group(1)] = 0 if args in ("", "void") else len([a for a in args.split(",") if a.strip()])
    return protos


def _exported(lib_path):
    """the dynamic symbols a library defines (`nm -D`), without the linker's and the HIP runtime's own"""
    out = subprocess.run(["nm", "-D", "--defined-only", lib_path], stdout=subprocess.PIPE, text=True, check=True).stdout
    syms = {l.split()[-1] for l in out.splitlines() if l.strip()}
    return {s for s in syms if not s.startswith(("__hip", "_init", "_fini", "__bss", "_edata", "_end"))}


def check_exports(row):
    """header prototypes, `nm -D` exports and SIGNATURES (plus last_error) are the row's pinned set, with matching arities and ABI revision"""
    mod = _binding(row)
    L = mod.lib()
    header = os.path.join(ROOT, "include", row.header)
    protos = _prototypes(header, row.prefix)
    last_error = row.prefix + "last_error"
    assert set(protos) == row.exports, (row.name, sorted(set(protos) ^ row.exports))
    exported = _exported(mod.LIB_PATH)
    if row.name == "product" and os.environ.get("CFSAR_DEV", "0") == "1":         # a developer build exports its debug hooks too
        assert row.exports <= exported, (row.name, sorted(row.exports - exported))
    else:
        assert exported == row.exports, (row.name, sorted(exported ^ row.exports))
        assert not any("debug" in s for s in exported), row.name
    assert set(mod.SIGNATURES) | {last_error} == row.exports, (row.name, sorted((set(mod.SIGNATURES) | {last_error}) ^ row.exports))
    for name, args in mod.SIGNATURES.items():
        assert hasattr(L, name), (row.name, name)
        assert len(args) == protos[name], (row.name, name, len(args), protos[name])
    assert protos[last_error] == 0 and isinstance(getattr(L, last_error)(), bytes), row.name
    define = re.search(r"#define %sABI_VERSION (\d+)" % row.prefix.upper(), open(header).read())
    assert getattr(L, row.prefix + "abi_version")() == mod.ABI_VERSION == int(define.group(1)), row.name
    assert getattr(L, row.prefix + "version")() >= 100, row.name


def check_abi_at_load(row, monkeypatch):
    """a binding written against another ABI revision, and one whose library is absent, raise at lib()"""
    mod = _binding(row)
    mod.lib()
    monkeypatch.setattr(mod, "_lib", None)
    monkeypatch.setattr(mod, "ABI_VERSION", mod.ABI_VERSION + 1)
    with pytest.raises(RuntimeError, match="ABI revision"):
        mod.lib()
    monkeypatch.setattr(mod, "LIB_PATH", mod.LIB_PATH + ".absent")
    with pytest.raises(RuntimeError, match="no CPU/PyTorch fallback"):
        mod.lib()
