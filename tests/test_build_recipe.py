"""CPU: every library and its place in the build, checked once over the table of tests/_abi.py (the product library and the ten side
libraries): what each exports, that its binding checks the ABI revision at load, that the symbol prefixes and the resource reports stay
apart, the one registry of build.py, which libraries an edited file makes stale, and the headers that hold the one copy of the code two
libraries share.  What is particular to one library stays in its own test_<name>_abi.py."""
import itertools
import json
import os
import re

import pytest

from _abi import LIBS, SIDE, _binding, _exported, check_abi_at_load, check_exports
from clip_fsar_amd import build as b

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = "product"
NAMES = [row.name for row in SIDE]
by_name = pytest.mark.parametrize("row", LIBS, ids=[row.name for row in LIBS])
side_by_name = pytest.mark.parametrize("row", SIDE, ids=NAMES)


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as ge
    ge.build()                                    # builds all eleven libraries (no-op when up to date)


# ------------------------------------------------------------------ 1. exports
def test_the_table_pins_eleven_export_sets():
    assert [len(row.exports) for row in LIBS] == [48, 8, 8, 6, 6, 4, 6, 5, 6, 4, 7]
    assert len({row.module for row in LIBS}) == len({row.header for row in LIBS}) == 11
    for row in LIBS:
        assert row.exports >= {row.prefix + e for e in ("version", "abi_version", "last_error")}, row.name


@by_name
def test_header_exports_and_signatures_are_the_pinned_set(row):
    check_exports(row)


# ------------------------------------------------------------------ 2. the ABI revision at load
@side_by_name
def test_abi_version_is_checked_at_load(row, monkeypatch):
    check_abi_at_load(row, monkeypatch)


# ------------------------------------------------------------------ 3. prefixes
def test_every_library_exports_its_own_prefix_and_no_other():
    for x, y in itertools.permutations(LIBS, 2):
        assert not x.prefix.startswith(y.prefix), (x.name, y.name)                # distinct, and none hides another
    for row in LIBS:
        mod = _binding(row)
        names = _exported(mod.LIB_PATH) | set(mod.SIGNATURES)
        assert names and all(s.startswith(row.prefix) for s in names), (row.name, sorted(names))
        for other in LIBS:
            if other is not row:
                assert not any(s.startswith(other.prefix) for s in names), (row.name, other.name)


# ------------------------------------------------------------------ 4. resource reports
def _report(name):
    """the parsed resource report of a library, built first when a fresh library has lost it"""
    path = b.USAGE if name == P else b.SIDE_LIBS[name].usage
    if not os.path.exists(path):
        b.build(force=True, verbose=False) if name == P else b.build_side(name, force=True, verbose=False)
    return json.load(open(path))


@side_by_name
def test_kernels_are_the_listed_ones_and_use_no_scratch(row):
    sl = b.SIDE_LIBS[row.name]
    usage = _report(row.name)
    names = sorted(usage)
    for fragment, count in row.kernels.items():
        assert sum(fragment in n for n in names) == count, (row.name, fragment, names)
    assert len(names) == row.total == sum(row.kernels.values()), (row.name, names)
    assert all(any(fragment in n for fragment in row.kernels) for n in names), (row.name, names)
    for n, u in usage.items():
        assert u.get("scratch", 0) == 0 and u.get("spills", 0) == 0, (row.name, n, u)
    assert sl.source == row.name + ".hip" and sl.source not in b.SOURCES, row.name
    assert sl.lib.endswith(os.sep + "libclipfsar_%s.so" % row.name) and sl.lib == _binding(row).LIB_PATH, row.name
    assert os.path.normpath(sl.usage).endswith(os.path.join("build", row.name, "resource_usage.json")), row.name


def test_the_resource_reports_stay_apart():
    paths = [b.USAGE] + [b.SIDE_LIBS[n].usage for n in NAMES]
    libs = [b.LIB] + [b.SIDE_LIBS[n].lib for n in NAMES]
    assert len(set(paths)) == len(set(libs)) == 11
    assert os.path.normpath(b.USAGE).endswith(os.path.join("clip-fsar_amd", "build", "resource_usage.json"))
    reports = {row.name: _report(row.name) for row in LIBS}
    for x, y in itertools.combinations(LIBS, 2):
        assert not set(reports[x.name]) & set(reports[y.name]), (x.name, y.name)
    # nor does a kernel of one side library sit in another report under another signature: no other report holds a kernel of that
    # identifier (the mangled name carries it behind its length), and where the bare fragment occurs in another side library's report it
    # is inside a longer fragment that library lists (stream's ring_put_kernel in pool's pool_ring_put_kernel)
    for x, y in itertools.permutations(LIBS, 2):
        for fragment in x.kernels or ():
            for n in reports[y.name]:
                assert "%d%s" % (len(fragment), fragment) not in n, (x.name, fragment, y.name, n)
                if y.kernels:
                    assert fragment not in n or any(fragment in g and g in n for g in y.kernels), (x.name, fragment, y.name, n)
    assert not any("otam_gallery_kernel" in n for n in reports[P])


# ------------------------------------------------------------------ 5. the registry
def test_one_registry_names_the_ten_side_libraries_in_build_order():
    assert list(b.SIDE_LIBS) == b.side_lib_names() == NAMES, sorted(set(b.SIDE_LIBS) ^ set(NAMES))
    assert NAMES == ["gallery", "gallery_text", "stream", "pool", "ingest", "live", "groups", "lastblock", "enroll", "live_text"]
    registries = [d for d in vars(b).values() if isinstance(d, dict) and d and all(isinstance(v, b.SideLib) for v in d.values())]
    assert len(registries) == 1 and registries[0] is b.SIDE_LIBS
    for call in (b._side_deps, b.build_side):
        with pytest.raises(KeyError):
            call("nobody")
    for name in NAMES:                            # the fixture ran build(): every library of the registry is there
        assert os.path.exists(b.SIDE_LIBS[name].lib), name
    assert os.path.exists(b.LIB)
    patterns = set(open(os.path.join(ROOT, ".gitignore")).read().split())
    assert {"*.so", "*.o", "build/"} <= patterns  # every library's products: lib*.so, build/<name>/


# ------------------------------------------------------------------ 6. staleness
#  edited file -> the stale ones of the product library and the ten; every file of csrc/ and every include/clipfsar_*.h has a row
ALL = {P} | set(NAMES)
OTAM = {"gallery", "live", "groups", "live_text"}                                 # the libraries whose source includes otam_tile.h
STALE = {
    "build.py": ALL,
    "common.h": ALL,
    "clipfsar_hip.h": ALL,                        # common.h includes it
    "clipfsar_hip_dev.h": set(),                  # the -DCFSAR_DEV hooks: read by developer builds alone, and _product_deps does not list it
    "side_lib.h": set(NAMES),
    "fp32_tile_gemm.h": OTAM | {"gallery_text"},
    "otam_tile.h": OTAM,                          # includes fp32_tile_gemm.h, otam_dp.h and side_lib.h
    "otam_dp.h": OTAM | {P},
    "topk_wave.h": {"gallery", "groups"},
    "text_softmax.h": {"gallery_text", "live_text"},
    "ring_rows.h": {"stream", "pool", "enroll"},
    "frame_transform.h": {P, "ingest"},
    "gemm_vit.h": {P},
    "gemm_vit_epi.h": {P},
}
for _s in b.SOURCES:
    STALE[_s] = {P}
for _n in NAMES:                                  # a library's source and its C header: that library alone ...
    STALE[_n + ".hip"] = STALE["clipfsar_%s.h" % _n] = {_n}
STALE["clipfsar_pool.h"] = {"pool", "enroll"}     # ... but the enrolment header takes CFSP_MAX_T from the pool's


def test_the_stale_matrix_has_every_file_and_exactly_the_libraries_it_reaches(monkeypatch):
    files = set(os.listdir(b.CSRC)) | {f for f in os.listdir(os.path.join(ROOT, "include")) if re.fullmatch(r"clipfsar_\w+\.h", f)}
    files.add("build.py")
    assert set(STALE) <= files, sorted(set(STALE) - files)                        # no row for a file that is gone
    monkeypatch.setattr(b.os.path, "exists", lambda p: True)
    for edited in sorted(files):
        monkeypatch.setattr(b.os.path, "getmtime", lambda p: 2.0 if p.endswith(os.sep + edited) else 1.0)   # newer than every library
        stale = {P} if b._stale(b.LIB, b._product_deps()) else set()
        stale |= {n for n in b.side_lib_names() if b._stale(b.SIDE_LIBS[n].lib, b._side_deps(n))}
        assert edited in STALE, "%s has no row in STALE; editing it makes %s stale" % (edited, sorted(stale))
        assert stale == STALE[edited], (edited, sorted(stale ^ STALE[edited]))


def test_the_product_library_does_not_depend_on_side_only_files():
    deps = b._product_deps()
    for f in [n + ".hip" for n in NAMES] + ["fp32_tile_gemm.h", "otam_tile.h", "ring_rows.h", "side_lib.h", "topk_wave.h", "text_softmax.h"]:
        assert os.path.join(b.CSRC, f) not in deps, f
    for f in ("otam_dp.h", "frame_transform.h", "common.h"):
        assert os.path.join(b.CSRC, f) in deps, f
    for f in set(os.listdir(b.CSRC)) & set(STALE):                                # and as the matrix has it
        assert (os.path.join(b.CSRC, f) in deps) == (P in STALE[f]), f
    assert os.path.join(b.CSRC, "frame_transform.h") in b._side_deps("ingest")


# ------------------------------------------------------------------ 7. code that two libraries share has one copy
def _src(name):
    return open(os.path.join(b.CSRC, name)).read()


def test_shared_code_has_one_copy():
    # one K loop: fp32_tile_gemm.h holds the MFMA; gallery_text.hip calls it through the identity map, the OTAM tile through a row source
    assert _src("fp32_tile_gemm.h").count("__builtin_amdgcn_mfma_f32_16x16x4f32") == 1
    assert "fp32_tile_gemm(" in _src("gallery_text.hip")
    # one OTAM tile body: otam_tile.h holds the K loop's call, the distance image and the DP fan-out; gallery.hip (dense rows: the identity
    # map, as fp32_tile_gemm's) and live.hip (looked-up rows) hold a row source and a wrapper kernel each
    tile = _src("otam_tile.h")
    assert tile.count("fp32_tile_gemm_rows(") == 1 and tile.count("otam_dp<TT>(") == 1 and tile.count("0.01f") == 1
    for src, rows in (("gallery.hip", "TileRows{"), ("live.hip", "LookedUpRow{")):
        text = _src(src)
        assert '#include "otam_tile.h"' in text and text.count("otam_tile<TT>(") == 1 and rows in text, src
        for body in ("__builtin_amdgcn_mfma", "fp32_tile_gemm_rows(", "otam_dp<", "0.01f", "tile_videos(", "extern __shared__"):
            assert body not in text, (src, body)
    # one smoothing recurrence and one set of copy-kernel limits: ring_rows.h
    ring = _src("ring_rows.h")
    assert ring.count("__fmaf_rn(") == 1 and ring.count("struct Piece") == 2                    # the template and its 16-byte form
    for src in ("stream.hip", "pool.hip"):
        text = _src(src)
        assert '#include "ring_rows.h"' in text and text.count("smooth_run(") == 1, src
        for body in ("__fmaf_rn", "struct Piece", "MAX_BLOCKS =", "MAX_ITEMS =", "bool vec_ok", "unsigned blocks_for"):
            assert body not in text, (src, body)
    # one "slot appears twice" scan: side_lib.h
    assert _src("side_lib.h").count("struct SlotBits") == 1
    for src in ("pool.hip", "live.hip"):
        text = _src(src)
        assert "SlotBits seen(" in text and "calloc" not in text and "thread_local" not in text, src
    # one frame transform: rowops.hip and ingest.hip compile the arithmetic from the one header
    for src in ("rowops.hip", "ingest.hip"):
        text = _src(src)
        assert '#include "frame_transform.h"' in text and "frame_transform_pixel(" in text and "inv255" not in text, src


def test_the_tile_body_and_the_slot_arithmetic_have_one_copy():
    from clip_fsar_amd import build as b
    src = lambda name: open(os.path.join(b.CSRC, name)).read()
    tile, groups, live = src("otam_tile.h"), src("groups.hip"), src("live.hip")
    assert tile.count("void otam_tile_at(") == 1 and tile.count("otam_tile_at<TT>(") == 1 and "blockIdx" in tile
    assert groups.count("otam_tile_at<TT>(") == 1 and '#include "otam_tile.h"' in groups and "LookedUpRow{" in groups
    for body in ("__builtin_amdgcn_mfma", "fp32_tile_gemm_rows(", "otam_dp<", "0.01f", "extern __shared__", "asm"):
        assert body not in groups, body
    assert tile.count("slot = cols[c0 + j]") == 1                                 # the slot arithmetic: otam_tile.h alone
    for text in (groups, live):
        assert "store_slot_row(" in text and "store_slot_norm(" in text and "cols[c0 + j]" not in text
    topk = src("topk_wave.h")
    assert topk.count("__shfl_xor(bv") == 1
    for text in (groups, src("gallery.hip")):
        assert text.count("topk_wave(") == 1 and "__shfl_xor" not in text


def test_the_softmax_code_has_one_copy():
    from clip_fsar_amd import build as b
    src = lambda name: open(os.path.join(b.CSRC, name)).read()
    shared, dense, grouped = src("text_softmax.h"), src("gallery_text.hip"), src("live_text.hip")
    for body in ("void merge_partials(", "void row_pass4(", "float block_max(", "float block_sum(", "void text_tile_epilogue(",
                 "void text_softmax_row(", "void text_combine_row("):
        assert shared.count(body) == 1, body
        assert body not in dense and body not in grouped, body
    for text in (dense, grouped):
        assert '#include "text_softmax.h"' in text
        assert text.count("text_tile_epilogue(") == 1 and text.count("text_softmax_row(") == 1 and text.count("text_combine_row(") == 1
        for body in ("powf(", "wave_max(", "wave_sum(", "fmaxf(", "merge_partials(", "__builtin_amdgcn_mfma"):
            assert body not in text, body
    assert src("fp32_tile_gemm.h").count("__builtin_amdgcn_mfma_f32_16x16x4f32") == 1
    assert "fp32_tile_gemm(" in dense and grouped.count("fp32_tile_gemm_rows(") == 1 and "LookedUpRow{" in grouped
    assert "store_slot_row(" in grouped and "store_slot_norm(" in grouped and "cols[c0" not in grouped     # the slot arithmetic: otam_tile.h
