"""CPU: the still-frame gate (libclipfsar_still.so, include/ext/clipfsar_still.h, clip_fsar_amd.still_hip, clip_fsar_amd.still,
StreamPool(still=...)) -- the plug-in library's exports, ABI check at load, resource report and place in the build (one more name of the
open registry, build.PLUGIN_LIBS); every host validation of cfsk_changed, cfsk_pack and cfsk_expand without a GPU; reference_changed
and plan_still on hand-written cases; StillGate's refusals; every refusal of StreamPool(still=...) on stub heads."""
import ctypes
import json
import os
import re
from types import SimpleNamespace as NS

import pytest
import torch

import _abi
from _abi import check_abi_at_load, check_exports

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ext", "clipfsar_still.h")
# the compare, the pack and the expansion each in a 16-byte and a 4-byte form; the sum over a frame's chunks
KERNELS = {"still_changed_kernel": 2, "still_finish_kernel": 1, "still_pack_kernel": 2, "still_expand_kernel": 2}
ROW = _abi._row("still", "still_hip", "cfsk_", "ext/clipfsar_still.h", "version abi_version last_error workspace_ints changed pack expand",
                KERNELS, 7)
INF, NAN = float("inf"), float("nan")


@pytest.fixture(scope="module")
def clib():
    import __graft_entry__ as ge
    ge.build()                                    # builds every library (no-op when up to date)
    from clip_fsar_amd import still_hip
    return still_hip.lib()


# ------------------------------------------------------------------ the library and its place in the build
def test_header_exported_exactly_and_arity_matches(clib):
    check_exports(ROW)
    assert ROW.exports == {"cfsk_" + e for e in ("version", "abi_version", "last_error", "workspace_ints", "changed", "pack", "expand")}
    from clip_fsar_amd import still_hip as sk
    text = open(HEADER).read()
    define = lambda name: int(re.search(r"#define CFSK_%s \(?(-?\d+)\)?" % name, text).group(1))
    assert define("ABI_VERSION") == sk.ABI_VERSION == 1
    assert define("TABLE_COLS") == sk.TABLE_COLS == 4
    assert [define(n) for n in ("SLOT", "F0", "N", "LAST_POS")] == [sk.SLOT, sk.F0, sk.N, sk.LAST_POS] == list(range(4))
    assert define("MAX_STREAMS") == sk.MAX_STREAMS == 65536 and define("CHUNK") == sk.CHUNK == 8192
    assert [len(sk.SIGNATURES["cfsk_" + e]) for e in ("workspace_ints", "changed", "pack", "expand")] == [2, 12, 13, 14]
    # the workspace: an int per (frame, chunk)
    for n, L, want in ((1, 1, 1), (5, 8192, 5), (5, 8193, 10), (64, 150528, 64 * 19), (3, (1 << 31) - 1, 3 * (1 << 18)),
                       (0, 5, -1), (-1, 5, -1), (5, 0, -1), (5, 1 << 31, -1), (1 << 14, (1 << 31) - 1, -1)):
        assert clib.cfsk_workspace_ints(n, L) == want, (n, L)
    assert sk.workspace_ints(5, 8193) == 10
    with pytest.raises(RuntimeError, match="no workspace for N=0"):
        sk.workspace_ints(0, 5)
    for other in _abi.LIBS:                       # its prefix hides no other library's, and none hides it
        assert not other.prefix.startswith(ROW.prefix) and not ROW.prefix.startswith(other.prefix), other.name
    for prefix in ("cfcs_", "cfev_", "cfbl_", "cfsh_", "cfps_", "cfal_", "cftp_", "cfed_"):
        assert not prefix.startswith(ROW.prefix) and not ROW.prefix.startswith(prefix)


def test_abi_version_is_checked_at_load(clib, monkeypatch):
    check_abi_at_load(ROW, monkeypatch)


def test_the_kernels_are_the_listed_ones_and_use_no_scratch(clib):
    from clip_fsar_amd import build as b
    from clip_fsar_amd import still_hip as sk
    pl = b.PLUGIN_LIBS["still"]
    if not os.path.exists(pl.usage):
        b.build_plugin("still", force=True, verbose=False)
    usage = json.load(open(pl.usage))
    assert len(usage) == ROW.total == sum(KERNELS.values()), sorted(usage)
    for fragment, count in KERNELS.items():
        assert sum(fragment in n for n in usage) == count, (fragment, sorted(usage))
    for n, u in usage.items():
        assert u.get("scratch", 0) == 0 and u.get("spills", 0) == 0, (n, u)
    assert pl.lib == sk.LIB_PATH and pl.lib.endswith(os.sep + "libclipfsar_still.so") and os.path.exists(pl.lib)
    others = [b.USAGE] + [x.usage for reg in (b.SIDE_LIBS, b.EXT_LIBS, b.ADDON_LIBS) for x in reg.values()]
    others += [x.usage for n, x in b.PLUGIN_LIBS.items() if n != "still"]
    for path in others:                           # no other library's report names them, and they carry no other library's fragment
        if os.path.exists(path):
            assert not any(fragment in n for n in json.load(open(path)) for fragment in KERNELS), path
    import test_align_abi, test_baseline_abi, test_events_abi, test_evidence_abi, test_pool_select_abi, test_shortlist_abi, test_tempo_abi
    claimed = [f for row in _abi.SIDE for f in row.kernels]
    claimed += [f for mod in (test_align_abi, test_baseline_abi, test_events_abi, test_evidence_abi, test_pool_select_abi,
                              test_shortlist_abi, test_tempo_abi) for f in mod.KERNELS]
    for n in usage:
        assert not any(f in n for f in claimed), n
    # the conventions: the ring libraries' row pieces, the shared error plumbing and its own header -- nothing else of the project;
    # plain C++, integer counting without atomics, no allocation, no copy or wait of its own
    source = open(pl.source).read()
    assert re.findall(r'^#include [<"]([^>"]+)[>"]', source, flags=re.M) == ["math.h", "../csrc/ring_rows.h", "../csrc/side_lib.h",
                                                                            "../../include/ext/clipfsar_still.h"]
    for body in ("asm", "atomic", "malloc", "hipMalloc", "hipMemcpy", "hipMemset", "hipDeviceSynchronize", "hipStreamSynchronize"):
        assert body not in source, body
    for shared in ("Piece<VEC>", "vec_ok(", "blocks_for(", "MAX_ITEMS", "SIDE_REQUIRE(", "check_launch(", "SlotBits", "CFSK_LAST_POS"):
        assert shared in source, shared
    assert "__fsub_rn(" in source and "double" not in source.split("namespace {", 1)[1].split("// the host copy", 1)[0]
    assert "(size_t)i * L" in source and "(size_t)kept[r] * L" in source        # 64-bit element offsets: N * L passes 2^31


def test_still_is_a_name_of_the_open_registry_and_follows_the_recipe():
    from clip_fsar_amd import build as b
    assert "still" in b.PLUGIN_LIBS and "still" in b.plugin_lib_names()
    assert all("still" not in reg for reg in (b.SIDE_LIBS, b.EXT_LIBS, b.ADDON_LIBS))
    pl = b.PLUGIN_LIBS["still"]
    assert isinstance(pl, b.ExtLib)
    assert pl.source == os.path.join(b.EXT, "still.hip") and os.path.exists(pl.source)
    assert pl.header == HEADER and os.path.exists(pl.header)
    assert pl.lib == os.path.join(b.HERE, "libclipfsar_still.so")
    assert pl.usage == os.path.join(b.HERE, "build", "still", "resource_usage.json")
    deps = b._plugin_deps("still")
    assert sorted(deps) == sorted([pl.source, pl.header, os.path.abspath(b.__file__), os.path.join(b.CSRC, "ring_rows.h"),
                                   os.path.join(b.CSRC, "side_lib.h"), os.path.join(b.CSRC, "common.h"),
                                   os.path.join(ROOT, "include", "clipfsar_hip.h")])
    for call in (b.build_side, b._side_deps, b.build_ext, b._ext_deps, b.build_addon, b._addon_deps):       # the three closed registries
        with pytest.raises(KeyError):
            call("still")
    assert not os.path.exists(os.path.join(b.CSRC, "still.hip"))
    assert not any("clipfsar_still" in open(os.path.join(b.CSRC, f)).read() for f in os.listdir(b.CSRC))    # nothing of csrc/ knows it
    # the semantics are pure Python and torch on the CPU: no binding, no library
    sem = open(os.path.join(b.HERE, "still.py")).read()
    assert "still_hip" not in re.sub(r'""".*?"""', "", sem, flags=re.S) and "ctypes" not in sem and ".cuda" not in sem


def test_staleness_of_the_still_library_and_of_no_other(monkeypatch):
    from clip_fsar_amd import build as b
    from test_build_recipe import NAMES, STALE, P
    monkeypatch.setattr(b.os.path, "exists", lambda p: True)

    def stale_after(edited):
        monkeypatch.setattr(b.os.path, "getmtime", lambda p: 2.0 if p.endswith(os.sep + edited) else 1.0)
        old = {P} if b._stale(b.LIB, b._product_deps()) else set()
        old |= {n for n in NAMES if b._stale(b.SIDE_LIBS[n].lib, b._side_deps(n))}
        old |= {n for n in b.EXT_LIBS if b._stale(b.EXT_LIBS[n].lib, b._ext_deps(n))}
        old |= {n for n in b.ADDON_LIBS if b._stale(b.ADDON_LIBS[n].lib, b._addon_deps(n))}
        return old, {n for n in b.PLUGIN_LIBS if b._stale(b.PLUGIN_LIBS[n].lib, b._plugin_deps(n))}

    for edited in ("still.hip", "clipfsar_still.h"):                              # its own files: it alone
        assert stale_after(edited) == (set(), {"still"}), edited
    old, plugins = stale_after("ring_rows.h")                                     # the row pieces: the ring libraries and it
    assert STALE["ring_rows.h"] <= old and "still" in plugins and "align" not in plugins
    for edited in ("side_lib.h", "build.py", "common.h"):                         # what every library reaches
        old, plugins = stale_after(edited)
        assert STALE[edited] <= old and plugins == set(b.PLUGIN_LIBS), edited
    for edited in ("pool.hip", "clipfsar_pool.h", "clipfsar_tempo.h", "tempo.hip", "clipfsar_events.h", "evidence.hip", "select_keys.h",
                   "chunk_row.h", "otam_tile.h", "fp32_tile_gemm.h", "align.hip", "gemm.hip", "ingest.hip", "still.py", "still_hip.py"):
        assert "still" not in stale_after(edited)[1], edited
    assert stale_after("no_such_file.h") == (set(), set())


# ------------------------------------------------------------------ validation, without a GPU
def _tbl(rows):
    flat = [v for r in rows for v in r]
    return (ctypes.c_int32 * len(flat))(*flat)


def _ints(*v):
    return (ctypes.c_int32 * max(1, len(v)))(*v)


#        slot f0 n last_pos
GOOD = [[2, 0, 3, 5],
        [0, 3, 4, -1],
        [1, 7, 2, 0]]                             # N = 9; max_streams 4; cap 16 where a ring is involved


def _edit(row, col, value):
    rows = [list(r) for r in GOOD]
    rows[row][col] = value
    return _tbl(rows)


def _table_refusals(call, err, name, cap=None):
    """the refusals of the host table that the three entry points share, each naming the entry point and the offending value"""
    def refused(words, **kw):
        assert call(**kw) != 0
        assert err().startswith(name + b": ") and words in err(), (kw, err())

    for ms in (0, 1 << 20, -1):
        refused(b"max_streams=%d outside 1 .. 65536" % ms, ms=ms)
    for S in (0, 5, -1):
        refused(b"a table of S=%d rows for max_streams=4" % S, S=S)
    for slot in (-1, 4):
        refused(b"row 1 has slot %d outside 0 .. 3" % slot, table=_edit(1, 0, slot))
    refused(b"slot 2 appears twice in the table (row 2)", table=_edit(2, 0, 2))
    for n in (0, -2):
        refused(b"row 0 has n=%d frames, every row needs at least 1" % n, table=_edit(0, 2, n))
    refused(b"row 2 has f0=5, the prefix sum of the counts is 7", table=_edit(2, 1, 5))
    refused(b"row 1 has f0=0, the prefix sum of the counts is 3", table=_edit(1, 1, 0))
    refused(b"row 0 has last_pos=-2 outside -1 ..", table=_edit(0, 3, -2))
    if cap is not None:
        refused(b"row 2 has last_pos=16 outside -1 .. 15", table=_edit(2, 3, 16))
    refused(b"the table's n sum to 9, not to N=10", N=10)
    refused(b"the table's n sum to 5, not to N=9", table=_tbl([[0, 0, 5, -1]]), S=1)
    refused(b"the table's n sum to 7, not to N=9", S=2)


def test_changed_validation_without_gpu(clib):
    err, good = clib.cfsk_last_error, _tbl(GOOD)
    f, pv, c, w, td = (ctypes.c_void_p(a << 32) for a in (1, 2, 3, 4, 5))        # far apart, never dereferenced

    # changed(frames, prev, counts, work, table_host, table_dev, S, N, L, max_streams, tol, stream)
    def call(ptrs=None, table=good, S=3, N=9, L=100, ms=4, tol=0.0):
        a = list(ptrs or [f, pv, c, w])
        return clib.cfsk_changed(*a, table, td, S, N, L, ms, tol, None)

    for i in range(4):
        ptrs = [f, pv, c, w]
        ptrs[i] = None
        assert call(ptrs=ptrs) != 0 and b"cfsk_changed: null pointer" in err(), i
    assert call(table=None) != 0 and b"null pointer" in err()
    assert clib.cfsk_changed(f, pv, c, w, good, None, 3, 9, 100, 4, 0.0, None) != 0 and b"null pointer" in err()
    for kw in ({"N": 0}, {"N": -1}, {"L": 0}, {"L": -5}):
        assert call(**kw) != 0 and b"cfsk_changed: bad shape" in err(), kw
    assert call(L=1 << 31) != 0 and b"cfsk_changed: L=2147483648 elements per frame" in err()
    for tol in (-1.0, -1e-30, INF, -INF, NAN):
        assert call(tol=tol) != 0 and b"cfsk_changed: tol=" in err() and b"must be finite and >= 0" in err(), tol
    assert call(tol=-0.5) != 0 and b"tol=-0.5 " in err()
    _table_refusals(call, err, b"cfsk_changed")
    big = _tbl([[0, 0, 1 << 14, -1]])
    assert call(table=big, S=1, N=1 << 14, L=(1 << 31) - 1) != 0 and b"cfsk_changed: too large for one launch (N=16384 frames of 262144 chunks)" in err()
    # counts or work inside frames / prev, or inside each other
    at = lambda p, off: ctypes.c_void_p(p.value + off)
    for ptrs in ([f, pv, at(f, 8), w], [f, pv, at(pv, 4 * 100 * 4 - 4), w], [f, pv, c, at(f, 9 * 100 * 4 - 4)], [f, pv, c, at(pv, 0)],
                 [f, pv, c, at(c, 32)], [f, pv, at(f, -4), w]):
        assert call(ptrs=ptrs) != 0 and b"cfsk_changed: counts or work overlaps" in err() and b"of its own" in err(), ptrs


def test_pack_validation_without_gpu(clib):
    err, good = clib.cfsk_last_error, _tbl(GOOD)
    f, pk, pv, kd, td = (ctypes.c_void_p(a << 32) for a in (1, 2, 3, 4, 5))
    k3 = _ints(0, 4, 8)

    # pack(frames, packed, prev, kept_host, kept_dev, NK, table_host, table_dev, S, N, L, max_streams, stream)
    def call(ptrs=None, kept=k3, NK=3, table=good, S=3, N=9, L=100, ms=4, kdev=kd):
        a = list(ptrs or [f, pk, pv])
        return clib.cfsk_pack(*a, kept, kdev, NK, table, td, S, N, L, ms, None)

    for i in (0, 2):
        ptrs = [f, pk, pv]
        ptrs[i] = None
        assert call(ptrs=ptrs) != 0 and b"cfsk_pack: null pointer" in err(), i
    assert call(table=None) != 0 and b"cfsk_pack: null pointer" in err()
    # packed and kept are needed exactly when something is packed: 0 < NK < N
    for kw in ({"ptrs": [f, None, pv]}, {"kept": None}, {"kdev": None}):
        assert call(**kw) != 0 and b"cfsk_pack: null pointer (packed or kept, with NK=3 of N=9)" in err(), kw
    for kw in ({"N": 0}, {"L": 0}, {"N": -4}):
        assert call(**kw) != 0 and b"cfsk_pack: bad shape" in err(), kw
    assert call(L=1 << 31) != 0 and b"cfsk_pack: L=2147483648 elements per frame" in err()
    for NK in (-1, 10):
        assert call(NK=NK) != 0 and b"cfsk_pack: NK=%d kept frames outside 0 .. N=9" % NK in err(), NK
    _table_refusals(call, err, b"cfsk_pack")
    for bad, words in (((-1, 4, 8), b"kept[0]=-1 outside 0 .. 8"), ((0, 4, 9), b"kept[2]=9 outside 0 .. 8"),
                       ((0, 4, 4), b"kept[2]=4 after kept[1]=4, the list must be strictly ascending"),
                       ((5, 4, 8), b"kept[1]=4 after kept[0]=5")):
        assert call(kept=_ints(*bad)) != 0 and b"cfsk_pack: " + words in err(), bad
    at = lambda p, off: ctypes.c_void_p(p.value + off)
    assert call(ptrs=[f, pk, at(f, 9 * 100 * 4 - 4)]) != 0 and b"cfsk_pack: prev overlaps frames" in err()
    for ptrs in ([f, at(f, 16), pv], [f, at(pv, 4 * 100 * 4 - 4), pv], [f, at(f, -4), pv]):
        assert call(ptrs=ptrs) != 0 and b"cfsk_pack: packed overlaps frames or prev" in err(), ptrs
    big = _tbl([[0, 0, 1 << 14, -1]])
    assert call(kept=_ints(*range(1 << 13)), NK=1 << 13, table=big, S=1, N=1 << 14, L=(1 << 31) - 1, ms=1) != 0 \
        and b"cfsk_pack: too large for one launch (NK=8192 S=1 rows of 262144 chunks)" in err()


def test_expand_validation_without_gpu(clib):
    err, good = clib.cfsk_last_error, _tbl(GOOD)
    kf, ring, feats, sd, td = (ctypes.c_void_p(a << 32) for a in (1, 2, 3, 4, 5))
    src = _ints(0, 0, 1, 2, 2, 2, 3, -1, 4)      # row 1 (no frame before the push) starts kept; row 2's first frame reads the ring

    # expand(kept_feats, ring, feats, src_host, src_dev, NK, table_host, table_dev, S, N, E, max_streams, cap, stream)
    def call(ptrs=None, src=src, NK=5, table=good, S=3, N=9, E=64, ms=4, cap=16, sdev=sd):
        a = list(ptrs or [kf, ring, feats])
        return clib.cfsk_expand(*a, src, sdev, NK, table, td, S, N, E, ms, cap, None)

    for i in (1, 2):
        ptrs = [kf, ring, feats]
        ptrs[i] = None
        assert call(ptrs=ptrs) != 0 and b"cfsk_expand: null pointer" in err(), i
    for kw in ({"src": None}, {"sdev": None}, {"table": None}):
        assert call(**kw) != 0 and b"cfsk_expand: null pointer" in err(), kw
    assert call(ptrs=[None, ring, feats]) != 0 and b"cfsk_expand: null pointer (kept_feats, with NK=5)" in err()
    for kw in ({"N": 0}, {"E": 0}, {"cap": 0}, {"E": -1}):
        assert call(**kw) != 0 and b"cfsk_expand: bad shape" in err(), kw
    for NK in (-1, 10):
        assert call(NK=NK) != 0 and b"cfsk_expand: NK=%d kept frames outside 0 .. N=9" % NK in err(), NK
    _table_refusals(call, err, b"cfsk_expand", cap=16)
    # src: -1 .. NK - 1, and no -1 where the session has nothing in the ring
    assert call(src=_ints(0, 0, 1, 2, 2, 2, 3, -1, 5)) != 0 and b"cfsk_expand: src[8]=5 outside -1 .. NK-1=4" in err()
    assert call(src=_ints(0, -2, 1, 2, 2, 2, 3, -1, 4)) != 0 and b"cfsk_expand: src[1]=-2 outside -1 .. NK-1=4" in err()
    assert call(src=_ints(0, 0, 1, -1, 2, 2, 3, -1, 4)) != 0 \
        and b"cfsk_expand: src[3]=-1 in row 1, whose session has no frame before the push (last_pos=-1)" in err()
    assert call(src=_ints(0, 0, 1, 2, -1, 2, 3, -1, 4)) != 0 and b"src[4]=-1 in row 1" in err()
    assert call(E=1 << 22, cap=2047) != 0 and b"cfsk_expand: too large for one launch" in err()
    at = lambda p, off: ctypes.c_void_p(p.value + off)
    for ptrs in ([kf, ring, at(ring, 4 * 16 * 64 * 4 - 4)], [kf, ring, at(kf, 5 * 64 * 4 - 4)], [kf, ring, at(kf, -4)]):
        assert call(ptrs=ptrs) != 0 and b"cfsk_expand: feats overlaps kept_feats or the ring" in err(), ptrs


def test_python_wrappers_reject_cpu_tensors_and_bad_shapes(clib):
    from clip_fsar_amd import still_hip as sk
    host = torch.tensor(GOOD, dtype=torch.int32)
    table = sk.Table(host, host, 3)               # a device copy that is no device tensor
    i32 = dict(dtype=torch.int32)
    with pytest.raises(RuntimeError, match="HIP device tensor"):
        sk.changed(torch.zeros(9, 10), torch.zeros(4, 10), torch.zeros(9, **i32), torch.zeros(9, **i32), table, 0.0)
    with pytest.raises(RuntimeError, match="shape"):
        sk.changed(torch.zeros(9, 10), torch.zeros(4, 11), torch.zeros(9, **i32), torch.zeros(9, **i32), table, 0.0)
    with pytest.raises(RuntimeError, match="shape"):
        sk.changed(torch.zeros(9, 10), torch.zeros(4, 10), torch.zeros(8, **i32), torch.zeros(9, **i32), table, 0.0)
    with pytest.raises(RuntimeError, match=r"work has shape \(8,\), expected at least \[9\]"):
        sk.changed(torch.zeros(9, 10), torch.zeros(4, 10), torch.zeros(9, **i32), torch.zeros(8, **i32), table, 0.0)
    with pytest.raises(RuntimeError, match="Table"):
        sk.changed(torch.zeros(9, 10), torch.zeros(4, 10), torch.zeros(9, **i32), torch.zeros(9, **i32), sk.Table(host[:, :3], host, 3), 0.0)
    k = torch.tensor([0, 4, 8], **i32)
    with pytest.raises(RuntimeError, match="shape"):
        sk.pack(torch.zeros(9, 10), torch.zeros(2, 10), torch.zeros(4, 10), sk.List(k, k, 3), table)
    with pytest.raises(RuntimeError, match="kept must be a List of 3 int32"):
        sk.pack(torch.zeros(9, 10), torch.zeros(3, 10), torch.zeros(4, 10), sk.List(k.long(), k, 3), table)
    with pytest.raises(RuntimeError, match="HIP device tensor"):
        sk.pack(torch.zeros(9, 10), None, torch.zeros(4, 10), sk.List(None, None, 9), table)
    s = torch.zeros(9, **i32)
    with pytest.raises(RuntimeError, match="shape"):
        sk.expand(torch.zeros(5, 8), torch.zeros(4, 16, 7), torch.zeros(9, 8), sk.List(s, s, 9), table)
    with pytest.raises(RuntimeError, match="src must be a List of 9 int32"):
        sk.expand(torch.zeros(5, 8), torch.zeros(4, 16, 8), torch.zeros(9, 8), sk.List(s[:8], s[:8], 8), table)
    with pytest.raises(RuntimeError, match="HIP device tensor"):
        sk.expand(torch.zeros(5, 8), torch.zeros(4, 16, 8), torch.zeros(9, 8), sk.List(s, s, 9), table)


# ------------------------------------------------------------------ reference_changed on hand-written cases
def test_reference_changed_hand_cases():
    from clip_fsar_amd.still import reference_changed
    tol = 0.25                                    # exact in fp32, and so is every difference below
    prev = torch.tensor([[9.0] * 8, [1.0, 1.0, NAN, INF, -INF, 0.0, -0.0, 5.0]])
    #                      = tol     > tol   NaN vs NaN  inf - inf  -inf - -inf   -0 vs +0   +0 vs -0   equal
    x0 = torch.tensor([1.25, 1.2500001, NAN, INF, -INF, -0.0, 0.0, 5.0])
    x1 = torch.tensor([1.0, 1.0, 1.0, INF, INF, 0.25, -0.25, NAN])               # against x0: NaN on one side, inf vs -inf, a NaN arriving
    frames = torch.stack([x0, x1])
    got = reference_changed(frames, prev, [(1, 0, 2, 3)], tol)
    # x0 against prev[1]: 1.25 - 1 = tol exactly: NOT changed; 1.2500001 (the next fp32 above 1.25) - 1 > tol: changed; NaN against NaN,
    # inf - inf and -inf + inf: changed; the zeros of either sign: not; equal: not -> 4
    # x1 against x0: |1 - 1.25| = tol: not; 1 - 1.2500001: changed; 1 against NaN: changed; inf - inf: changed; inf - -inf = inf:
    # changed; 0.25 - -0 = tol and -0.25 - 0 = -tol: not; NaN against 5: changed -> 5
    want = 5
    assert got.dtype == torch.int32 and got.tolist() == [4, want]
    # tol = 0: only equal elements (and the zeros of either sign) are unchanged
    assert reference_changed(frames, prev, [(1, 0, 2, 3)], 0.0).tolist() == [5, 8]
    # no predecessor: -1, and prev is not read (a NaN store changes nothing); the second frame is compared with the first as before
    nanprev = torch.full((2, 8), NAN)
    assert reference_changed(frames, nanprev, [(1, 0, 2, -1)], tol).tolist() == [-1, want]
    # two sessions in one table, each frame against its own predecessor; trailing dimensions are flattened
    f = torch.zeros(4, 2, 2)
    f[1, 0, 0] = 1.0
    f[2] = 9.0
    f[3] = 9.0
    f[3, 1, 1] = 9.5
    p = torch.zeros(3, 2, 2)
    p[2] = 9.0
    assert reference_changed(f, p, [(0, 0, 2, 7), (2, 2, 2, 0)], 0.0).tolist() == [0, 1, 0, 1]
    assert reference_changed(f, p, [(0, 0, 2, 7), (1, 2, 2, 0)], 0.0).tolist() == [0, 1, 4, 1]
    assert reference_changed(f, p, [(0, 0, 2, -1), (1, 2, 2, -1)], 0.0).tolist() == [-1, 1, -1, 1]
    # tol is rounded to fp32 once: 0.1 as a double is below fp32(0.1), and a difference of exactly fp32(0.1) is not a change
    t32 = float(torch.tensor(0.1, dtype=torch.float32))
    assert t32 > 0.1
    assert reference_changed(torch.tensor([[t32]]), torch.zeros(1, 1), [(0, 0, 1, 0)], 0.1).tolist() == [0]


# ------------------------------------------------------------------ plan_still on hand-written cases
def test_plan_still_hand_cases():
    from clip_fsar_amd.still import StillGate, plan_still
    # one session, a run across a push boundary: the run carried in is continued, and carried out
    rows = [(0, 0, 5, 3)]
    kept, src, runs = plan_still([0, 0, 7, 0, 0], rows, [2], 0, None)
    assert (kept, src, runs) == ([2], [-1, -1, 0, 0, 0], [2])                     # the first two take the row before the push
    # max_run = 3 forces a keep every max_run + 1 frames of an unchanging stream, across pushes
    pattern, run = [], [1]
    for _ in range(3):
        kept, src, run = plan_still([0] * 5, rows, run, 0, 3)
        pattern += [i in kept for i in range(5)]
    assert pattern == [False, False, True, False, False, False, True, False, False, False, True, False, False, False, True]
    assert run == [0]
    kept, src, run = plan_still([0] * 5, rows, [3], 0, 3)
    assert kept == [0, 4] and src == [0, 0, 0, 0, 1] and run == [0]
    assert plan_still([0] * 5, rows, [0], 0, 1) == ([1, 3], [-1, 0, 0, 1, 1], [1])     # max_run = 1: every other frame
    # a push skipped whole: NK = 0, every src = -1, the runs grow by the counts
    rows2 = [(3, 0, 2, 0), (1, 2, 3, 9)]
    assert plan_still([0, 0, 0, 0, 0], rows2, [4, 0], 0, None) == ([], [-1] * 5, [6, 3])
    # count -1 (no predecessor) is kept whatever the limit, and resets the run
    assert plan_still([-1, 0, 0, -1, 0], rows2, [4, 7], 100, None) == ([0, 3], [0, 0, -1, 1, 1], [1, 1])
    # sessions are independent: src counts kept frames over the whole push, runs per session
    assert plan_still([5, 0, 0, 5, 5], rows2, [0, 0], 4, None) == ([0, 3, 4], [0, 0, -1, 1, 2], [1, 0])
    # limit = floor(changed * L): a count equal to it is still, one above is not
    assert plan_still([5, 4, 5, 4, 3], rows2, [0, 0], 4, None) == ([0, 2], [0, 0, 1, 1, 1], [1, 2])
    g = StillGate(changed=0.001)
    assert g.limit(150528) == 150 and g.limit(999) == 0 and g.limit(1000) == 1 and StillGate().limit(10 ** 9) == 0
    assert StillGate(changed=0.5).limit(75) == 37 and StillGate(changed=0.999999).limit(12) == 11
    # every frame kept: src is the identity
    assert plan_still([9] * 5, rows2, [3, 3], 0, 2) == ([0, 1, 2, 3, 4], [0, 1, 2, 3, 4], [0, 0])
    # counts may come as a tensor
    assert plan_still(torch.tensor([0, 3, 0], dtype=torch.int32), [(0, 0, 3, 1)], [0], 2, None) == ([1], [-1, 0, 0], [1])


# ------------------------------------------------------------------ StillGate
def test_still_gate_refusals():
    from clip_fsar_amd.still import StillGate
    g = StillGate()
    assert (g.pixel_tol, g.changed, g.max_run, g.tol) == (0.0, 0.0, None, 0.0)
    g = StillGate(pixel_tol=0.1, changed=0.25, max_run=7)
    assert (g.pixel_tol, g.changed, g.max_run) == (0.1, 0.25, 7) and g.tol == float(torch.tensor(0.1, dtype=torch.float32)) != 0.1
    assert repr(g) == "StillGate(pixel_tol=0.1, changed=0.25, max_run=7)"
    assert StillGate(1, 0, 1).pixel_tol == 1.0
    with pytest.raises(AttributeError):
        g.max_run = 3
    for bad in (-1e-9, -1.0, INF, -INF, NAN):
        with pytest.raises(ValueError, match="pixel_tol must be finite and >= 0"):
            StillGate(pixel_tol=bad)
    for bad in (-0.1, 1.0, 1.5, NAN, INF):
        with pytest.raises(ValueError, match=r"changed must be in \[0, 1\)"):
            StillGate(changed=bad)
    for bad in (0, -1):
        with pytest.raises(ValueError, match="max_run must be None or an integer >= 1"):
            StillGate(max_run=bad)
    for bad in (1.0, "3", True, False):
        with pytest.raises(TypeError, match="max_run must be None or an integer"):
            StillGate(max_run=bad)
    for name in ("pixel_tol", "changed"):          # bools are refused as numbers, and so is what is no number
        for bad in (True, False, "0.1", None, [0.1]):
            with pytest.raises(TypeError, match="%s must be a number" % name):
                StillGate(**{name: bad})


# ------------------------------------------------------------------ StreamPool's option, on stub heads
def _stub_head(T=4, **train):
    engine = NS(arch={"embed": 8})
    return NS(args=NS(TRAIN=NS(**train), DATA=NS(NUM_INPUT_FRAMES=T)), _get_engine=lambda dev: engine, _engine_key=("stub",),
              arch_name="stub", precision="fp32", depth=1)


def _live(capacity=4, ids=(0, 1, 2), T=4):
    from clip_fsar_amd import live_gallery as lg
    g = lg.LiveGallery(_stub_head(T), "cpu", capacity=capacity)
    if ids:
        g._install(lg.plan_add(g._book, list(ids)).book)       # registered on the host alone: nothing below reaches the device
    return g


def test_stream_pool_still_refusals_are_raised_before_the_device_is_touched():
    from clip_fsar_amd.pool import StreamPool
    from clip_fsar_amd.still import StillGate
    g = _live()
    gate = StillGate(pixel_tol=0.02, max_run=5)
    p = StreamPool(g, max_streams=3, stride=2, max_push=5, still=gate)
    q = StreamPool(g, max_streams=3, stride=2, max_push=5)
    assert p._still is gate and q._still is None and p.cap == q.cap and p._ring.shape == q._ring.shape
    with pytest.raises(TypeError):
        StreamPool(g, 3, 2, 1, 5, 0.0, None, "column", None, None, gate)            # keyword-only
    for bad in (True, 0.02, "gate", (0.0, 0.0, None), StillGate):
        with pytest.raises(TypeError, match="StreamPool: still must be a StillGate, got %s" % type(bad).__name__):
            StreamPool(g, still=bad)
    # a pool without the option has the keys it had, and no last_kept()
    hq = q.open()
    assert q.stats(hq) == {"frames": 0, "tower_frames": 0, "windows": 0}
    assert q.stats() == {"frames": 0, "tower_frames": 0, "windows": 0, "open": 1}
    with pytest.raises(ValueError, match="last_kept: the pool was built without still="):
        q.last_kept()
    # with it: "still_frames" in both, an empty last_kept() before the first pixel push
    h = p.open()
    assert p.stats(h) == {"frames": 0, "tower_frames": 0, "windows": 0, "still_frames": 0}
    assert p.stats() == {"frames": 0, "tower_frames": 0, "windows": 0, "still_frames": 0, "open": 1}
    assert p.last_kept() == {}
    # the gate's per-session state: made by open(), cleared by reset(), gone with close(); a reused slot starts without a predecessor
    assert p._sk_state[h] == [False, 0, 0]
    p._sk_state[h][:] = [True, 4, 9]
    p.reset(h)
    assert p._sk_state[h] == [False, 0, 0] and p.stats(h)["still_frames"] == 0
    p._sk_state[h][:] = [True, 4, 9]
    slot = p._sessions[h].slot
    p.close(h)
    assert h not in p._sk_state
    h2 = p.open()
    assert p._sessions[h2].slot == slot and p._sk_state[h2] == [False, 0, 0]
    with pytest.raises(ValueError, match="is not open"):
        p.stats(h)
    # pushes: the existing checks come first, and nothing is allocated by a refused push
    with pytest.raises(RuntimeError, match="HIP device tensor"):
        p.push_packed(torch.zeros(2, 3, 4, 4), [h2], [2])
    with pytest.raises(ValueError, match="counts sum to 3"):
        p.push_packed(torch.zeros(2, 3, 4, 4), [h2], [3])
    with pytest.raises(ValueError, match="is not open"):
        p.push_packed(torch.zeros(2, 3, 4, 4), [h], [2])
    assert p._sk_prev is None and p._sk_hw is None and p._sk_state[h2] == [False, 0, 0]
    # a feature push that is refused leaves the gate's state alone
    p._sk_state[h2][:] = [True, 2, 5]
    with pytest.raises(RuntimeError, match="HIP device tensor"):
        p.push_features_packed(torch.zeros(2, 8), [h2], [2])
    assert p._sk_state[h2] == [True, 2, 5]
    # composes with every other option of the constructor
    from clip_fsar_amd.baseline import Baseline
    from clip_fsar_amd.events import EventRule
    from clip_fsar_amd.evidence import Evidence
    r = StreamPool(g, smooth=0.5, smooth_by="class", events=EventRule(0.6, 0.4, 2, 2), baseline=Baseline(), rates=(1, 2),
                   evidence=Evidence(capacity=8), still=StillGate())
    assert set(r.stats()) == {"frames", "tower_frames", "windows", "events", "events_dropped", "evidence", "evidence_missed",
                              "still_frames", "open"}
