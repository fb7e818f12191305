"""CPU: build.py's recipe for the seven libraries -- the one registry of side libraries, which library an edited file makes stale, and the
headers that hold the one copy of the code two libraries share.  What a library exports and what its kernels use stays in its own
test_<name>_abi.py."""
import os

from clip_fsar_amd import build as b

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["gallery", "gallery_text", "stream", "pool", "ingest", "live"]


def test_the_registry_names_six_side_libraries_with_products_of_their_own():
    assert list(b.SIDE_LIBS) == NAMES and b.side_lib_names() == NAMES
    libs = [b.LIB] + [b.SIDE_LIBS[n].lib for n in NAMES]
    reports = [b.USAGE] + [b.SIDE_LIBS[n].usage for n in NAMES]
    assert len(set(libs)) == 7 and len(set(reports)) == 7
    patterns = set(open(os.path.join(ROOT, ".gitignore")).read().split())
    assert {"*.so", "*.o", "build/"} <= patterns
    for n in NAMES:
        sl = b.SIDE_LIBS[n]
        assert sl.source == n + ".hip" and sl.source not in b.SOURCES
        assert sl.lib.endswith(os.sep + "libclipfsar_%s.so" % n)
        assert os.path.normpath(sl.usage).endswith(os.path.join("build", n, "resource_usage.json"))


#  edited file -> the stale ones of (product, gallery, gallery_text, stream, pool, ingest, live)
P, G, GT, S, PL, I, L = "product", *NAMES
STALE = {
    "tail.hip": {P},
    "rowops.hip": {P},
    "frame_transform.h": {P, I},
    "fp32_tile_gemm.h": {G, GT, L},
    "otam_dp.h": {P, G, L},
    "otam_tile.h": {G, L},                      # includes fp32_tile_gemm.h, otam_dp.h and side_lib.h; gallery.hip and live.hip include it
    "ring_rows.h": {S, PL},                     # stream.hip and pool.hip include it
    "side_lib.h": set(NAMES),
    "common.h": {P} | set(NAMES),
}
for _n in NAMES:                                # a library's source and its C header: that library alone
    STALE[_n + ".hip"] = STALE["clipfsar_%s.h" % _n] = {_n}


def test_an_edited_file_makes_exactly_the_libraries_that_reach_it_stale(monkeypatch):
    monkeypatch.setattr(b.os.path, "exists", lambda p: True)
    for edited, want in sorted(STALE.items()):
        monkeypatch.setattr(b.os.path, "getmtime", lambda p: 2.0 if p.endswith(os.sep + edited) else 1.0)   # newer than every library
        stale = (b._stale(b.LIB, b._product_deps()),) + tuple(b._stale(b.SIDE_LIBS[n].lib, b._side_deps(n)) for n in b.side_lib_names())
        assert stale == tuple(n in want for n in [P] + NAMES), edited


def test_the_product_library_does_not_depend_on_side_only_files():
    deps = b._product_deps()
    for f in [n + ".hip" for n in NAMES] + ["fp32_tile_gemm.h", "otam_tile.h", "ring_rows.h", "side_lib.h"]:
        assert os.path.join(b.CSRC, f) not in deps, f
    for f in ("otam_dp.h", "frame_transform.h", "common.h"):
        assert os.path.join(b.CSRC, f) in deps, f
    assert os.path.join(b.CSRC, "frame_transform.h") in b._side_deps("ingest")


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
