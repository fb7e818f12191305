"""CPU: the timeline (libclipfsar_timeline.so, include/ext/clipfsar_timeline.h, clip_fsar_amd.timeline_hip, clip_fsar_amd.timeline,
StreamPool(timeline=...)) -- the plug-in library's exports, ABI check at load, resource report and place in the build (one more name of
the open registry, build.PLUGIN_LIBS); the source's conventions; every host validation of cftl_fold and cftl_read without a GPU; the
binding's refusals; Timeline's errors; reference_fold and reference_read on hand-written rows; every refusal of
StreamPool(timeline=...), timeline() and recall() on stub heads."""
import ctypes
import json
import os
import re
import struct

import numpy as np
import pytest
import torch

import _abi
from _abi import check_abi_at_load, check_exports
from test_contest_abi import _live, _stub_head

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ext", "clipfsar_timeline.h")
KERNELS = {"timeline_fold_kernel": 1, "timeline_read_kernel": 1}
ROW = _abi._row("timeline", "timeline_hip", "cftl_", "ext/clipfsar_timeline.h", "version abi_version last_error fold read", KERNELS, 2)
INF, NAN = float("inf"), float("nan")
FMAX = float(np.finfo(np.float32).max)


@pytest.fixture(scope="module")
def clib():
    import __graft_entry__ as ge
    ge.build()                                    # builds every library (no-op when up to date)
    from clip_fsar_amd import timeline_hip
    return timeline_hip.lib()


def _bits(values):
    """fp32 bit patterns: NaN-proof, sign-of-zero-proof equality"""
    return [struct.pack("f", v) for v in values]


# ------------------------------------------------------------------ the library and its place in the build
def test_header_exported_exactly_and_arity_matches(clib):
    check_exports(ROW)
    assert ROW.exports == {"cftl_" + e for e in ("version", "abi_version", "last_error", "fold", "read")}
    from clip_fsar_amd import class_smooth_hip as ch
    from clip_fsar_amd import timeline as tm
    from clip_fsar_amd import timeline_hip as th
    text = open(HEADER).read()
    smooth = open(os.path.join(ROOT, "include", "ext", "clipfsar_class_smooth.h")).read()
    define = lambda name: int(re.search(r"#define CFTL_%s (\d+)" % name, text).group(1))
    for name in ("MAX_STREAMS", "CHUNK", "TABLE_COLS", "SLOT", "NW", "OUT0", "NC", "KEY0", "CHUNK0"):       # the fold's table is CFCS_*'s, redeclared
        assert define(name) == int(re.search(r"#define CFCS_%s (\d+)" % name, smooth).group(1)) == getattr(th, name) == getattr(ch, name), name
    for i, name in enumerate(("R_SLOT", "R_B0", "R_NB", "R_NC", "R_KEY0", "R_OUT0", "R_CHUNK0")):            # the read's is its own
        assert define(name) == getattr(th, name) == getattr(tm, name) == i, name
    assert define("READ_COLS") == th.READ_COLS == 7 and define("ABI_VERSION") == th.ABI_VERSION == 1
    assert define("MAX_SPAN") == th.MAX_SPAN == tm.MAX_SPAN == 1 << 20
    assert define("MAX_BUCKETS") == th.MAX_BUCKETS == tm.MAX_BUCKETS == 1 << 16
    assert th.plan_rows is ch.plan_rows and th.MAX_CELLS == (1 << 31) - 1 and tm.CHUNK == th.CHUNK
    assert [len(th.SIGNATURES["cftl_" + e]) for e in ("fold", "read")] == [21, 19]
    for other in _abi.LIBS:                       # its prefix hides no other library's, and none hides it
        assert not other.prefix.startswith(ROW.prefix) and not ROW.prefix.startswith(other.prefix), other.name
    for prefix in ("cfcs_", "cfev_", "cfbl_", "cfsh_", "cfps_", "cfal_", "cftp_", "cfed_", "cfsk_", "cfct_", "cfhs_", "cfld_"):
        assert not prefix.startswith(ROW.prefix) and not ROW.prefix.startswith(prefix)


def test_abi_version_is_checked_at_load(clib, monkeypatch):
    check_abi_at_load(ROW, monkeypatch)


def test_the_kernels_are_the_two_listed_and_use_no_scratch(clib):
    from clip_fsar_amd import build as b
    from clip_fsar_amd import timeline_hip as th
    pl = b.PLUGIN_LIBS["timeline"]
    if not os.path.exists(pl.usage):
        b.build_plugin("timeline", force=True, verbose=False)
    usage = json.load(open(pl.usage))
    assert len(usage) == ROW.total == sum(KERNELS.values()) == 2, sorted(usage)
    for fragment, count in KERNELS.items():
        assert sum(fragment in n for n in usage) == count, (fragment, sorted(usage))
    for n, u in usage.items():
        assert u.get("scratch", 0) == 0 and u.get("spills", 0) == 0, (n, u)
    assert pl.lib == th.LIB_PATH and pl.lib.endswith(os.sep + "libclipfsar_timeline.so") and os.path.exists(pl.lib)
    others = [b.USAGE] + [x.usage for reg in (b.SIDE_LIBS, b.EXT_LIBS, b.ADDON_LIBS) for x in reg.values()]
    others += [x.usage for n, x in b.PLUGIN_LIBS.items() if n != "timeline"]
    for path in others:                           # no other library's report names them, and they carry no other library's fragment
        if os.path.exists(path):
            assert not any(fragment in n for n in json.load(open(path)) for fragment in KERNELS), path
    import test_align_abi, test_baseline_abi, test_contest_abi, test_events_abi, test_evidence_abi, test_history_abi, test_ledger_abi
    import test_pool_select_abi, test_shortlist_abi, test_still_abi, test_tempo_abi
    claimed = [f for row in _abi.SIDE for f in row.kernels]
    claimed += [f for mod in (test_align_abi, test_baseline_abi, test_contest_abi, test_events_abi, test_evidence_abi, test_history_abi,
                              test_ledger_abi, test_pool_select_abi, test_shortlist_abi, test_still_abi, test_tempo_abi) for f in mod.KERNELS]
    for n in usage:
        assert not any(f in n for f in claimed), n


def test_the_source_follows_the_conventions():
    from clip_fsar_amd import build as b
    source = open(b.PLUGIN_LIBS["timeline"].source).read()
    # the shared error plumbing and its own header -- not chunk_row.h or ring_rows.h, whose includers are pinned
    assert re.findall(r'^#include [<"]([^>"]+)[>"]', source, flags=re.M) == ["../csrc/side_lib.h", "../../include/ext/clipfsar_timeline.h",
                                                                            "math.h"]
    # plain C++ for wave64: no assembly, no allocation, no stream, copy or wait of its own, no LDS, no shuffles; ONE launch per entry point
    for body in ("asm", "thread_local", "calloc", "malloc", "hipMalloc", "hipStreamCreate", "__builtin_amdgcn", "hipMemcpy", "hipMemset",
                 "hipDeviceSynchronize", "hipStreamSynchronize", "__shared__", "__shfl", "__syncthreads", "warpSize", "fmaf"):
        assert body not in source, body
    assert not re.findall(r"[Aa]tomic\w*\(", source)
    assert source.count("hipLaunchKernelGGL(") == 2 and "SIDE_REQUIRE(" in source and source.count("check_launch(") == 2
    assert source.count("__global__") == 2 and source.count("__launch_bounds__(CHUNK)") == 2
    # the rule is pure Python and numpy on the CPU: no binding, no library, no torch
    sem = open(os.path.join(b.HERE, "timeline.py")).read()
    code = re.sub(r'""".*?"""', "", sem, flags=re.S)
    assert "timeline_hip" not in code and "ctypes" not in sem and ".cuda" not in sem and "import torch" not in sem


def test_timeline_is_a_name_of_the_open_registry_and_of_no_other():
    from clip_fsar_amd import build as b
    assert "timeline" in b.PLUGIN_LIBS and "timeline" in b.plugin_lib_names()
    assert all("timeline" not in reg for reg in (b.SIDE_LIBS, b.EXT_LIBS, b.ADDON_LIBS))
    pl = b.PLUGIN_LIBS["timeline"]
    assert isinstance(pl, b.ExtLib)
    assert pl.source == os.path.join(b.EXT, "timeline.hip") and os.path.exists(pl.source)
    assert pl.header == HEADER and os.path.exists(pl.header)
    assert pl.lib == os.path.join(b.HERE, "libclipfsar_timeline.so")
    assert pl.usage == os.path.join(b.HERE, "build", "timeline", "resource_usage.json")
    deps = b._plugin_deps("timeline")
    assert sorted(deps) == sorted([pl.source, pl.header, os.path.abspath(b.__file__), os.path.join(b.CSRC, "side_lib.h"),
                                   os.path.join(b.CSRC, "common.h"), os.path.join(ROOT, "include", "clipfsar_hip.h")])
    for call in (b.build_side, b._side_deps, b.build_ext, b._ext_deps, b.build_addon, b._addon_deps):       # the three closed registries
        with pytest.raises(KeyError):
            call("timeline")
    assert not os.path.exists(os.path.join(b.CSRC, "timeline.hip"))
    assert not any("clipfsar_timeline" in open(os.path.join(b.CSRC, f)).read() for f in os.listdir(b.CSRC))   # nothing of csrc/ knows it
    assert not any(row.name == "timeline" for row in _abi.LIBS)
    text = open(b.__file__).read()
    assert "clip_fsar_amd.timeline" in text[text.index("# The plug-in tier"):text.index("PLUGIN_LIBS = {")]


def test_staleness_of_the_timeline_library_and_of_no_other(monkeypatch):
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

    for edited in ("timeline.hip", "clipfsar_timeline.h"):                        # its own files: it alone
        assert stale_after(edited) == (set(), {"timeline"}), edited
    for edited in ("side_lib.h", "build.py", "common.h"):                         # what every library reaches
        old, plugins = stale_after(edited)
        assert STALE[edited] <= old and plugins == set(b.PLUGIN_LIBS), edited
    for edited in ("pool.hip", "clipfsar_pool.h", "baseline.hip", "clipfsar_baseline.h", "class_smooth.hip", "clipfsar_class_smooth.h",
                   "history.hip", "clipfsar_history.h", "chunk_row.h", "ring_rows.h", "select_keys.h", "otam_tile.h", "gemm.hip",
                   "timeline.py", "timeline_hip.py", "pool.py"):
        assert "timeline" not in stale_after(edited)[1], edited
    assert stale_after("chunk_row.h")[1] == {"baseline"}                          # the header's includer stays the one it was
    assert stale_after("no_such_file.h") == (set(), set())


# ------------------------------------------------------------------ validation, without a GPU
def _tbl(rows):
    flat = [v for r in rows for v in r]
    return (ctypes.c_int32 * len(flat))(*flat)


#        slot nW out0 NC key0 chunk0
GOOD = [[2, 2, 0, 300, 0, 0],                    # two chunks of 256 columns
        [0, 0, 600, 3, 300, 2],                  # no windows
        [1, 5, 600, 256, 44, 3]]                 # a list that overlaps the first; NOUT = 600 + 1280, NKEYS = 303, max_streams 4, cap 300
FIRST = [7, 0, 3]
NOUT, NKEYS = 1880, 303


def _edit(good, row, col, value):
    rows = [list(r) for r in good]
    rows[row][col] = value
    return _tbl(rows)


def test_fold_validation_without_gpu(clib):
    p = ctypes.c_void_p(4096)                     # never dereferenced: every call below fails validation before any device work
    err, good, first = clib.cftl_last_error, _tbl(GOOD), _tbl([FIRST])
    # fold(scores, peak, at, above, marks, gens, keys, table_host, table_dev, first_host, first_dev,
    #      S, NOUT, NKEYS, max_streams, B, cap, span, has_level, level, stream)

    def call(t=good, f=first, S=3, nout=NOUT, nkeys=NKEYS, ms=4, B=5, cap=300, span=3, has_level=0, level=0.0):
        return clib.cftl_fold(p, p, p, p, p, p, p, t, p, f, p, S, nout, nkeys, ms, B, cap, span, has_level, level, None)

    for i in range(11):
        args = [p] * 7 + [good, p, first, p]
        args[i] = None
        assert clib.cftl_fold(*args, 3, NOUT, NKEYS, 4, 5, 300, 3, 0, 0.0, None) != 0 and b"cftl_fold: null pointer" in err(), i
    for level in (NAN, INF, -INF):
        assert call(has_level=1, level=level) != 0 and b"level=" in err() and b"finite" in err(), level
    for ms in (0, -1, 65537, 1 << 20):
        assert call(ms=ms) != 0 and b"max_streams" in err(), ms
    for S in (0, -2, 5):                          # no rows; more rows than slots
        assert call(S=S) != 0 and b"rows" in err(), S
    for cap in (0, -7):
        assert call(cap=cap) != 0 and b"cap=" in err(), cap
    for B in (0, -1, 65537):
        assert call(B=B) != 0 and b"B=%d buckets outside 1 .. 65536" % B in err(), B
    for span in (0, -1, (1 << 20) + 1):
        assert call(span=span) != 0 and b"span=%d outside 1 .. 1048576" % span in err(), span
    assert call(ms=4096, B=2048, cap=300) != 0 and b"too large" in err() and b"cells" in err()      # 2^31 cells and more
    assert call(ms=1 << 16, B=1 << 15, cap=1) != 0 and b"too large" in err()                        # exactly 2^31
    assert call(nout=-1) != 0 and b"bad shape" in err()
    assert call(nkeys=0) != 0 and b"bad shape" in err()

    def rejected(row, *words, **kw):
        assert call(**kw) != 0 and all(w in err() for w in words + (b"row %d" % row,)), (row, words, err())

    for slot in (-1, 4):
        rejected(1, b"slot", b"outside", t=_edit(GOOD, 1, 0, slot))
    rejected(2, b"appears twice", t=_edit(GOOD, 2, 0, 2))
    rejected(0, b"negative count", t=_edit(GOOD, 0, 1, -1))
    for NC in (0, -3):
        rejected(1, b"width", t=_edit(GOOD, 1, 3, NC))
    rejected(1, b"prefix sums", t=_edit(GOOD, 1, 2, 599))         # OUT0
    rejected(2, b"prefix sums", t=_edit(GOOD, 2, 2, 603))
    rejected(0, b"prefix sums", t=_edit(GOOD, 0, 2, 1))
    rejected(1, b"prefix sums", t=_edit(GOOD, 1, 5, 1))           # CHUNK0: the first row has two chunks
    rejected(2, b"prefix sums", t=_edit(GOOD, 2, 5, 2))
    rejected(2, b"keys[", t=_edit(GOOD, 2, 4, -1))                # KEY0 below 0, and the list's end beyond NKEYS
    rejected(2, b"keys[", t=_edit(GOOD, 2, 4, 48))
    rejected(0, b"keys[", t=_edit(GOOD, 0, 4, 4))
    rejected(0, b"keys[", nkeys=299)
    rejected(1, b"keys[", nkeys=302)
    for r in range(3):                            # first >= 0, a row without windows included
        rejected(r, b"negative first window (first=-1)", f=_edit([FIRST], 0, r, -1))
    rejected(2, b"window numbers stay below 2^31", f=_edit([FIRST], 0, 2, (1 << 31) - 5))       # first + NW = 2^31
    rejected(0, b"window numbers stay below 2^31", f=_edit([FIRST], 0, 0, (1 << 31) - 1))
    assert call(nout=NOUT + 1) != 0 and b"not to NOUT" in err()
    assert call(nout=NOUT - 1) != 0 and b"not to NOUT" in err()
    big = _tbl([[0, 40000, 0, 60000, 0, 0]])      # products beyond 2^31: 40 000 windows x 60 000 columns
    assert call(t=big, S=1, nout=0, nkeys=60000, cap=60000, B=1) != 0 and b"too large" in err() and b"row 0" in err()
    # a table without a window is valid and launches nothing; so are the parameters' edges
    empty, zero = _tbl([[3, 0, 0, 7, 0, 0]]), _tbl([[0]])
    assert call(t=empty, f=zero, S=1, nout=0, nkeys=7) == 0, err()
    assert call(t=empty, f=_tbl([[(1 << 31) - 1]]), S=1, nout=0, nkeys=7, span=1 << 20, B=1 << 16, cap=8, has_level=1, level=FMAX) == 0, err()
    assert call(t=empty, f=zero, S=1, nout=0, nkeys=7, span=1, B=1, has_level=0, level=NAN) == 0, err()     # no level: the value is not looked at


#         slot b0 nb NC key0 out0 chunk0
RGOOD = [[2, 4, 5, 300, 0, 0, 0],                # a full ring of 5 buckets, two chunks
         [0, 0, 0, 3, 300, 1500, 2],             # no buckets
         [2, 7, 1, 256, 44, 1500, 3]]            # the first row's slot again; NOUT = 1500 + 256
RNOUT = 1756


def test_read_validation_without_gpu(clib):
    p = ctypes.c_void_p(4096)
    err, good = clib.cftl_last_error, _tbl(RGOOD)
    # read(peak, at, above, marks, gens, keys, out_peak, out_at, out_above, table_host, table_dev, S, NOUT, NKEYS, max_streams, B, cap, span, stream)

    def call(t=good, S=3, nout=RNOUT, nkeys=NKEYS, ms=4, B=5, cap=300, span=3):
        return clib.cftl_read(p, p, p, p, p, p, p, p, p, t, p, S, nout, nkeys, ms, B, cap, span, None)

    for i in range(11):
        args = [p] * 9 + [good, p]
        args[i] = None
        assert clib.cftl_read(*args, 3, RNOUT, NKEYS, 4, 5, 300, 3, None) != 0 and b"cftl_read: null pointer" in err(), i
    for ms in (0, 65537):
        assert call(ms=ms) != 0 and b"max_streams" in err(), ms
    for S in (0, -1, 65537):
        assert call(S=S) != 0 and b"a table of S=%d rows (1 .. 65536)" % S in err(), S
    assert call(cap=0) != 0 and b"cap=" in err()
    for B in (0, 65537):
        assert call(B=B) != 0 and b"buckets outside" in err(), B
    for span in (0, (1 << 20) + 1):
        assert call(span=span) != 0 and b"span=" in err(), span
    assert call(ms=4096, B=2048, cap=300) != 0 and b"too large" in err()
    assert call(nout=-1) != 0 and b"bad shape" in err()
    assert call(nkeys=0) != 0 and b"bad shape" in err()

    def rejected(row, *words, **kw):
        assert call(**kw) != 0 and all(w in err() for w in words + (b"row %d" % row,)), (row, words, err())

    for slot in (-1, 4):
        rejected(1, b"slot", b"outside", t=_edit(RGOOD, 1, 0, slot))
    rejected(0, b"negative first bucket (B0=-1)", t=_edit(RGOOD, 0, 1, -1))
    for NB in (-1, 6):
        rejected(0, b"NB=%d buckets outside 0 .. B=5" % NB, t=_edit(RGOOD, 0, 2, NB))
    rejected(2, b"beyond the last one a window number below 2^31 reaches", t=_edit(RGOOD, 2, 1, ((1 << 31) - 1) // 3 + 1))
    for NC in (0, -3):
        rejected(1, b"width", t=_edit(RGOOD, 1, 3, NC))
    rejected(1, b"prefix sums", t=_edit(RGOOD, 1, 5, 1499))       # OUT0
    rejected(2, b"prefix sums", t=_edit(RGOOD, 2, 5, 1503))
    rejected(1, b"prefix sums", t=_edit(RGOOD, 1, 6, 1))          # CHUNK0
    rejected(2, b"keys[", t=_edit(RGOOD, 2, 4, -1))
    rejected(2, b"keys[", t=_edit(RGOOD, 2, 4, 48))
    rejected(1, b"keys[", nkeys=302)
    assert call(nout=RNOUT + 1) != 0 and b"not to NOUT" in err()
    # the last bucket a window number reaches is fine; a table without a bucket launches nothing; a slot may appear in every row
    assert call(t=_tbl([[3, ((1 << 31) - 1) // 3, 0, 7, 0, 0, 0]]), S=1, nout=0, nkeys=7) == 0, err()
    assert call(t=_tbl([[1, 0, 0, 7, 0, 0, 0], [1, 9, 0, 300, 3, 0, 1], [1, 0, 0, 1, 0, 0, 3]]), S=3, nout=0) == 0, err()
    assert call(t=_tbl([[0, 0, 0, 1, 0, 0, 0]] * 5), S=5, nout=0, ms=1) != 0 and b"prefix sums" in err()      # S may exceed max_streams


def test_python_wrapper_rejects_cpu_tensors_and_bad_shapes(clib):
    from clip_fsar_amd import timeline_hip as th
    host = torch.tensor(GOOD, dtype=torch.int32)
    table = th.Table(host, host, 3)
    first = th.Table(torch.tensor(FIRST, dtype=torch.int32), torch.tensor(FIRST, dtype=torch.int32), 3)
    i32 = dict(dtype=torch.int32)
    x, pk = torch.zeros(NOUT), torch.zeros(4, 5, 300)
    at, ab, mk = (torch.zeros(4, 5, 300, **i32) for _ in range(3))
    gens, keys = torch.ones(300, **i32), torch.zeros(NKEYS, **i32)
    good = [x, pk, at, ab, mk, gens, keys]
    with pytest.raises(RuntimeError, match="HIP device tensor"):
        th.fold(*good, table, first, 3, None)
    with pytest.raises(RuntimeError, match="HIP device tensor"):                 # an empty plane too
        th.fold(x[:0], *good[1:], th.Table(host[:1] * 0, host[:1], 1), th.Table(first.host[:1], first.dev[:1], 1), 3, None)
    for i, bad in ((0, x.view(2, -1)), (1, pk[0]), (2, at[:3]), (3, ab[:, :4]), (4, mk[:, :, :299]), (5, gens[:299]), (6, keys.view(1, -1))):
        args = list(good)
        args[i] = bad
        with pytest.raises(RuntimeError, match="shape|flat"):
            th.fold(*args, table, first, 3, None)
    with pytest.raises(RuntimeError, match="table must be a Table"):
        th.fold(*good, th.Table(host[:, :5], host[:, :5], 3), first, 3, None)
    for bad in (first.host, th.Table(first.host[:2], first.dev[:2], 2), th.Table(first.host.long(), first.dev, 3),
                th.Table(first.host.view(3, 1), first.dev, 3)):
        with pytest.raises(RuntimeError, match=r"first must be a Table of \[S = 3\] int32 host values"):
            th.fold(*good, table, bad, 3, None)
    # read
    rhost = torch.tensor(RGOOD, dtype=torch.int32)
    rtable = th.Table(rhost, rhost, 3)
    op, oa, ob = torch.zeros(RNOUT), torch.zeros(RNOUT, **i32), torch.zeros(RNOUT, **i32)
    rgood = [pk, at, ab, mk, gens, keys, op, oa, ob]
    with pytest.raises(RuntimeError, match="HIP device tensor"):
        th.read(*rgood, rtable, 3)
    for i, bad in ((0, pk.view(20, 300)), (1, at[:3]), (3, mk[:, :4]), (4, gens[:299]), (5, keys.view(1, -1)), (6, op.view(2, -1)),
                   (7, oa[:-1]), (8, ob[:-1])):
        args = list(rgood)
        args[i] = bad
        with pytest.raises(RuntimeError, match="shape|flat"):
            th.read(*args, rtable, 3)
    with pytest.raises(RuntimeError, match="table must be a Table"):
        th.read(*rgood, table, 3)                 # the fold's six columns
    for bad_dtype_at in (1, 2, 3):                # dtypes: an fp32 plane where an int32 one belongs
        args = list(rgood)
        args[bad_dtype_at] = pk
        with pytest.raises(RuntimeError, match="HIP device tensor|dtype"):
            th.read(*args, rtable, 3)


# ------------------------------------------------------------------ the option's type and the rule
def test_timeline_errors_name_the_field():
    from clip_fsar_amd.timeline import Timeline, held_buckets, read_rows
    t = Timeline()
    assert t == (16, 256, None, None) and t._fields == ("span", "buckets", "level", "of")
    assert Timeline(1, 1, 0, "logits") == (1, 1, 0.0, "logits") and Timeline(1 << 20, 1 << 16, -FMAX, "deviation").level == -FMAX
    assert Timeline(level=0.1).level == float(np.float32(0.1)) and Timeline(of="smoothed").of == "smoothed"      # held as the fp32 value
    for kw, field in (({"span": 0}, "span"), ({"span": (1 << 20) + 1}, "span"), ({"span": 2.0}, "span"), ({"span": True}, "span"),
                      ({"span": None}, "span"), ({"buckets": 0}, "buckets"), ({"buckets": 65537}, "buckets"), ({"buckets": "8"}, "buckets"),
                      ({"buckets": False}, "buckets"), ({"level": NAN}, "level"), ({"level": INF}, "level"), ({"level": -INF}, "level"),
                      ({"level": 1e39}, "level"), ({"level": "0.5"}, "level"), ({"level": True}, "level"), ({"of": "judged"}, "of"),
                      ({"of": 0}, "of"), ({"of": "Logits"}, "of")):
        with pytest.raises(ValueError, match="Timeline: %s " % field):
            Timeline(**kw)
    # held buckets: max(0, bn - B + 1) .. bn with bn = (windows - 1) // span
    assert held_buckets(0, 3, 2) == range(0) and held_buckets(1, 3, 2) == range(0, 1) and held_buckets(3, 3, 2) == range(0, 1)
    assert held_buckets(4, 3, 2) == range(0, 2) and held_buckets(7, 3, 2) == range(1, 3) and held_buckets(7, 3, 2, last=1) == range(2, 3)
    assert held_buckets(7, 3, 2, last=9) == range(1, 3) and held_buckets(100, 1, 256) == range(0, 100) and held_buckets(300, 1, 256) == range(44, 300)
    assert read_rows([2, 0, 2], [range(4, 9), range(0), range(7, 8)], [300, 3, 256], [0, 300, 44]) == (RGOOD, RNOUT)


def _fold(state, gens, scores, first, span, B, level=None, slot=0, keys=(0,)):
    """one row of len(keys) columns over the flat row-major scores"""
    from clip_fsar_amd.timeline import reference_fold
    nc = len(keys)
    return reference_fold(state, gens, [[slot, len(scores) // nc, 0, nc, 0, 0]], list(keys), scores, [first], span, B, level)


def _cells(state, slot=0, key=0):
    """[(peak, at, above, marks)] per ring position"""
    return [tuple(p[slot, pos, key].item() for p in state) for pos in range(state[0].shape[1])]


def test_reference_fold_and_read_on_hand_written_rows():
    from clip_fsar_amd.timeline import new_state, reference_read
    gens = np.array([5, 1], np.int32)
    read = lambda st, b0, nb, span, B, keys=(0,): list(zip(*(v.tolist() for v in reference_read(st, gens, [[0, b0, nb, len(keys), 0, 0, 0]],
                                                                                                list(keys), span, B))))
    # a tie goes to the earlier window, a higher score replaces; first = 0, span 4, one bucket
    st = new_state(1, 2, 2)
    c = _fold(st, gens, [0.5, 0.25, 0.5, 1.0], 0, 4, 2)
    assert c == dict(ties=1, replaced=1, laps=0, restarted=0) and _cells(st)[0] == (1.0, 3, 4, 5)
    st = new_state(1, 2, 2)
    c = _fold(st, gens, [0.5, 0.25, 0.5, 0.5], 0, 4, 2)
    assert c["ties"] == 2 and c["replaced"] == 0 and _cells(st)[0] == (0.5, 0, 4, 5) and _cells(st)[1][3] == 0      # the other bucket: untouched
    # -0.0 before +0.0 keeps the first one's bits, and the other way round
    for a, b in ((-0.0, 0.0), (0.0, -0.0)):
        st = new_state(1, 1, 2)
        assert _fold(st, gens, [a, b], 0, 2, 1)["ties"] == 1
        assert _bits([_cells(st)[0][0]]) == _bits([a]) and _cells(st)[0][1:] == (0, 2, 5)
    # NaN and -inf neighbours are no candidates: they neither count nor replace; +inf is one and wins
    st = new_state(1, 1, 2)
    assert _fold(st, gens, [NAN, -1.0, -INF, NAN], 4, 4, 1) == dict(ties=0, replaced=0, laps=0, restarted=0)
    assert _cells(st)[0] == (-1.0, 5, 1, 5)
    st = new_state(1, 1, 2)
    _fold(st, gens, [FMAX, INF, INF, NAN], 0, 4, 1)
    assert _cells(st)[0] == (INF, 1, 3, 5)
    # level equal to a score counts it (>= as fp32); above it does not; no level counts every candidate
    third = float(np.float32(1 / 3))
    for level, n in ((1 / 3, 2), (float(np.nextafter(np.float32(third), np.float32(1))), 1), (FMAX, 0), (-FMAX, 3), (None, 3)):
        st = new_state(1, 1, 2)
        _fold(st, gens, [third, 0.5, 0.25, NAN], 0, 4, 1, level=level)
        assert _cells(st)[0] == (0.5, 1, n, 5), level
    # first off a bucket boundary: span 3, windows 4 .. 8 are bucket 1 (4, 5) and bucket 2 (6, 7, 8); B = 2: bucket 2 at position 0
    st = new_state(1, 2, 2)
    _fold(st, gens, [0.1, 0.2, 0.3, 0.9, 0.3], 4, 3, 2)
    assert _cells(st) == [(float(np.float32(0.9)), 7, 3, 5), (float(np.float32(0.2)), 5, 2, 5)]
    assert read(st, 1, 2, 3, 2) == [(float(np.float32(0.2)), 5, 2), (float(np.float32(0.9)), 7, 3)]
    assert read(st, 0, 1, 3, 2) == [(-INF, -1, 0)]                    # bucket 0 shares position 0 with bucket 2: an older lap's cell is not its
    # the same windows cut anywhere give the same state; the second call goes on in bucket 1's cell and sees the tie across the cut
    whole = new_state(1, 2, 2)
    _fold(whole, gens, [0.2, 0.2, 0.3, 0.9, 0.3], 4, 3, 2)
    cut = new_state(1, 2, 2)
    c1 = _fold(cut, gens, [0.2], 4, 3, 2)
    c2 = _fold(cut, gens, [0.2, 0.3, 0.9, 0.3], 5, 3, 2)
    assert all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(whole, cut)) and c1["ties"] == 0 and c2["ties"] == 1
    # a lap that overwrites a cell: B = 1, span 2 -- bucket 0 then bucket 1 in the one position, inside one call and across calls
    st = new_state(1, 1, 2)
    assert _fold(st, gens, [0.9, 0.1, 0.2, 0.3], 0, 2, 1)["laps"] == 1 and _cells(st)[0] == (float(np.float32(0.3)), 3, 2, 5)
    assert _fold(st, gens, [0.05], 4, 2, 1)["laps"] == 1 and _cells(st)[0] == (float(np.float32(0.05)), 4, 1, 5)
    # `at` of an older lap under the same generation: the cell starts empty, so a lower score takes it and the count restarts
    st = new_state(1, 2, 2)
    _fold(st, gens, [0.9, 0.9], 0, 2, 2)                              # bucket 0: peak 0.9 at 0, above 2
    c = _fold(st, gens, [0.1], 4, 2, 2)                               # bucket 2, position 0 again
    assert c == dict(ties=0, replaced=0, laps=1, restarted=0) and _cells(st)[0] == (float(np.float32(0.1)), 4, 1, 5)
    # a stale mark: the cell was written under generation 4, the slot is at 5 now; a mark of 0 was never written
    st = new_state(1, 1, 2)
    st[0][0, 0, 0], st[1][0, 0, 0], st[2][0, 0, 0], st[3][0, 0, 0] = 9.0, 1, 7, 4
    assert read(st, 0, 1, 4, 1) == [(-INF, -1, 0)]
    assert _fold(st, gens, [0.5], 2, 4, 1) == dict(ties=0, replaced=0, laps=0, restarted=1) and _cells(st)[0] == (0.5, 2, 1, 5)
    st = new_state(1, 1, 2)
    st[0][0, 0, 0], st[1][0, 0, 0], st[2][0, 0, 0] = 9.0, 1, 7       # marks 0
    assert _fold(st, gens, [0.5], 2, 4, 1) == dict(ties=0, replaced=0, laps=0, restarted=0) and _cells(st)[0] == (0.5, 2, 1, 5)
    # a live cell with at < 0 cannot be written by the fold; the read treats it as dead all the same
    st = new_state(1, 1, 2)
    st[1][0, 0, 0], st[3][0, 0, 0] = -1, 5
    assert read(st, 0, 1, 4, 1) == [(-INF, -1, 0)]
    # a bucket of non-candidates is left untouched: its stale cell keeps its bytes, the buckets around it are written
    st = new_state(1, 4, 2)
    st[0][0, 1, 0], st[1][0, 1, 0], st[2][0, 1, 0], st[3][0, 1, 0] = 7.0, 2, 1, 3
    _fold(st, gens, [0.5, 0.5, NAN, -INF, 0.25, NAN], 0, 2, 4)
    assert _cells(st)[:3] == [(0.5, 0, 2, 5), (7.0, 2, 1, 3), (0.25, 4, 1, 5)]
    assert read(st, 0, 3, 2, 4) == [(0.5, 0, 2), (-INF, -1, 0), (0.25, 4, 1)]
    # keys outside [0, cap) touch nothing and read as NaN; columns are folded apart; NW = 0 touches nothing
    st = new_state(1, 1, 2)
    _fold(st, gens, [0.75, 0.1, 0.2, 0.3, 0.5, 0.8, 0.9, 0.1], 0, 2, 1, keys=(1, -1, 2, 1 << 30))
    assert _cells(st, key=1)[0] == (0.75, 0, 2, 1) and _cells(st, key=0)[0][3] == 0
    got = read(st, 0, 1, 2, 1, keys=(1, -1, 2, 0))
    assert got[0] == (0.75, 0, 2) and got[3] == (-INF, -1, 0) and all(g[0] != g[0] and g[1:] == (-1, 0) for g in got[1:3])
    before = [a.copy() for a in st]
    _fold(st, gens, [], 7, 2, 1)
    assert all(np.array_equal(a, b) for a, b in zip(st, before))
    # a slot in two rows of a read, and NB = 0
    from clip_fsar_amd.timeline import read_rows
    rows, n_out = read_rows([0, 0, 0], [range(0, 1), range(0), range(0, 1)], [1, 1, 2], [1, 0, 0])
    p, a, n = reference_read(st, gens, rows, [0, 1], 2, 1)
    assert n_out == 3 and a.tolist() == [0, -1, 0] and n.tolist() == [2, 0, 2] and p.tolist() == [0.75, -INF, 0.75]


# ------------------------------------------------------------------ the option
def test_the_timeline_option_on_stub_heads():
    import inspect
    from clip_fsar_amd.baseline import Baseline
    from clip_fsar_amd.events import EventRule
    from clip_fsar_amd.gallery import SupportGallery
    from clip_fsar_amd.history import History
    from clip_fsar_amd.live_text_gallery import LiveTextGallery
    from clip_fsar_amd.pool import StreamPool
    from clip_fsar_amd.shortlist import Shortlist
    from clip_fsar_amd.still import StillGate
    from clip_fsar_amd.text_gallery import TextGallery
    from clip_fsar_amd.timeline import Timeline
    g = _live()                                   # T = 4, E = 8, classes 0, 1, 2
    tl = Timeline(span=3, buckets=2, level=0.5)
    p = StreamPool(g, max_streams=3, stride=2, max_push=5, timeline=tl)           # TypeError without the feature
    assert p._timeline == tl and p._keyed and p._tl_cells.planes is None and p._tl_tables is None and p._tl_work is None
    assert inspect.signature(StreamPool.__init__).parameters["timeline"].kind is inspect.Parameter.KEYWORD_ONLY
    for bad in (3, (3, 2, None, None), "timeline", {"span": 3}):
        with pytest.raises(TypeError, match="StreamPool: timeline must be a Timeline"):
            StreamPool(g, timeline=bad)
    for other in (SupportGallery(_stub_head(), "cpu"), TextGallery(_stub_head(COMBINE=True), "cpu")):
        with pytest.raises(ValueError, match="timeline= needs a gallery with a slot store.*%s" % type(other).__name__):
            StreamPool(other, timeline=tl)
    assert StreamPool(LiveTextGallery(_stub_head(COMBINE=True), "cpu", capacity=4), timeline=tl)._timeline is tl
    with pytest.raises(ValueError, match="timeline= together with shortlist= is not supported"):
        StreamPool(g, shortlist=Shortlist(g, keep=2), timeline=tl)
    with pytest.raises(ValueError, match=r"timeline.of = 'smoothed' names a plane this pool does not make -- build it with smooth > 0"):
        StreamPool(g, timeline=tl._replace(of="smoothed"))
    with pytest.raises(ValueError, match=r"timeline.of = 'smoothed' names a plane"):
        StreamPool(g, smooth=0.0, smooth_by="class", timeline=tl._replace(of="smoothed"))       # smooth = 0: the option is inert
    with pytest.raises(ValueError, match=r"timeline.of = 'deviation' names a plane this pool does not make -- build it with baseline="):
        StreamPool(g, timeline=tl._replace(of="deviation"))
    assert StreamPool(g, smooth=0.5, smooth_by="class", baseline=Baseline(), timeline=tl._replace(of="smoothed"))._timeline.of == "smoothed"
    assert StreamPool(g, baseline=Baseline(), timeline=tl._replace(of="deviation"))._keyed
    assert StreamPool(g, timeline=tl._replace(of="logits"))._keyed
    with pytest.raises(ValueError, match=r"timeline= keeps a state cell per \(session slot, bucket, store slot\): max_streams = 4096 x "
                       r"buckets = 2048 x store capacity = 256 is 2\^31 or more"):
        StreamPool(_live(capacity=256), max_streams=4096, timeline=Timeline(buckets=2048))
    assert StreamPool(_live(capacity=255), max_streams=4096, timeline=Timeline(buckets=2048))._tl_cells.planes is None
    # it combines with the other options and adds nothing to stats(); a pool without it is the pool as it was
    q = StreamPool(g, max_streams=3, smooth=0.5, smooth_by="class", events=EventRule(0.6, 0.4, 2, 2), rates=(1, 2), still=StillGate(),
                   history=History(128), baseline=Baseline(), timeline=tl)
    assert q.stats() == {"frames": 0, "tower_frames": 0, "windows": 0, "events": 0, "events_dropped": 0, "still_frames": 0, "open": 0}
    plain = StreamPool(g, max_streams=3, stride=2, max_push=5)
    assert plain._timeline is None and plain.stats() == p.stats() and not plain._keyed
    assert not any(hasattr(plain, a) for a in ("_tl_cells", "_tl_first", "_tl_tables", "_tl_work"))
    for call, name in ((lambda: plain.timeline(0), "timeline"), (lambda: plain.recall([0]), "recall")):
        with pytest.raises(ValueError, match=r"StreamPool.%s: this pool keeps no timeline \(build it with timeline=Timeline" % name):
            call()
    # open() and reset() queue the slot's marks for zeroing, in every keyed store of the pool
    a, b = p.open(), p.open(classes=[2, 0])
    assert p._tl_cells.forgotten == {0, 1} and q._tl_cells in q._stores
    # timeline(): every refusal before anything is allocated or launched
    with pytest.raises(ValueError, match="session 9 is not open"):
        p.timeline(9)
    for bad in (0, "01", {0, 1}):
        with pytest.raises(TypeError, match="StreamPool.timeline: classes must be None or a list of registered class ids"):
            p.timeline(a, classes=bad)
    for bad, words in (([], "classes= needs at least one class"), ([0, 0], r"a class appears twice in classes=: \[0, 0\]"),
                       ([0, 7], "class 7 is not registered")):
        with pytest.raises(ValueError, match="StreamPool.timeline: .*" + words):
            p.timeline(a, classes=bad)
    with pytest.raises(ValueError, match=r"StreamPool.timeline: class 1 is not registered \(classes= of session %d\)" % b):
        p.timeline(b, classes=[2, 1])
    for last in (0, -1, True, 1.0):
        with pytest.raises(ValueError, match=r"StreamPool.timeline: last must be None or an integer >= 1 \(buckets\)"):
            p.timeline(a, last=last)
    # a session without a window: empty planes over its own columns, nothing launched, nothing allocated
    v = p.timeline(a)
    assert (v.first_bucket, v.span, v.class_ids) == (0, 3, (0, 1, 2)) and all(tuple(t.shape) == (0, 3) for t in (v.peak, v.at, v.above))
    assert (v.peak.dtype, v.at.dtype, v.above.dtype) == (torch.float32, torch.int32, torch.int32)
    v = p.timeline(b)
    assert v.class_ids == (2, 0) and tuple(v.peak.shape) == (0, 2) and p.timeline(b, classes=[0]).class_ids == (0,)
    assert p._tl_cells.planes is None and p._tl_tables is None
    # the host's counters alone say which buckets are held: window k is complete at 2 k + 4 frames; span 3, two buckets
    for t, held in ((3, range(0)), (4, range(0, 1)), (9, range(0, 1)), (10, range(0, 2)), (16, range(1, 3)), (70, range(10, 12))):
        p._sessions[a].t = t
        assert p._held_buckets(p._sessions[a], None, "timeline") == held, t
    assert p._held_buckets(p._sessions[a], 1, "timeline") == range(11, 12)
    p.reset(a)
    assert p._held_buckets(p._sessions[a], None, "timeline") == range(0)
    # recall: every refusal before anything is allocated or launched
    for bad, words in (([], "classes= needs at least one class"), ([0, 0], r"a class appears twice in classes=: \[0, 0\]"), ([0, 7], "7")):
        with pytest.raises(ValueError, match="StreamPool.recall: .*" + words):
            p.recall(bad)
    for bad in (0, "01", None, {0, 1}):
        with pytest.raises(TypeError, match="StreamPool.recall: classes must be a list of registered class ids"):
            p.recall(bad)
    big = _live(capacity=80, ids=tuple(range(70)))
    with pytest.raises(ValueError, match="StreamPool.recall: 65 classes -- one recall takes 1 to 64"):
        StreamPool(big, timeline=tl).recall(list(range(65)))
    with pytest.raises(ValueError, match=r"StreamPool.recall: a session appears twice in sessions=: \[0, 1, 0\]"):
        p.recall([0], sessions=[a, b, a])
    with pytest.raises(ValueError, match="session 9 is not open"):
        p.recall([0], sessions=[a, 9])
    with pytest.raises(TypeError, match="StreamPool.recall: sessions must be None or a list of open sessions"):
        p.recall([0], sessions=a)
    for kw, words in ((dict(top=0), r"top must be an integer in \[1, 4096\], got 0"), (dict(top=4097), "top must be"), (dict(top=2.0), "top must be"),
                      (dict(separation=-1), "separation must be an integer >= 0, got -1"), (dict(separation=1.5), "separation must be"),
                      (dict(separation=None), "separation must be"), (dict(last=0), "last must be None or an integer >= 1"),
                      (dict(last=True), "last must be"), (dict(min_score=NAN), "min_score must be None or a number that is not NaN"),
                      (dict(min_score="1"), "min_score must be")):
        with pytest.raises(ValueError, match="StreamPool.recall: " + words):
            p.recall([0, 1], **kw)
    wide = StreamPool(g, stride=1, max_push=5, timeline=Timeline(span=1, buckets=10000))
    wide._sessions[wide.open()].t = 12000
    with pytest.raises(ValueError, match=r"StreamPool.recall: separation = 5000 over a longest row of 10000 windows"):
        wide.recall([0], separation=5000)
    # nothing is held yet: empty lists, nothing launched, nothing allocated
    r = p.recall([2, 0], top=3, min_score=0.5, separation=0, last=4)
    assert r == ({2: [], 0: []}, {2: 0, 0: 0}, 0) and r._fields == ("hits", "peaks", "buckets")
    assert p.recall([1], sessions=[]).hits == {1: []} and p._tl_cells.planes is None and p._tl_tables is None and p._tl_work is None
    p.close(a)
    with pytest.raises(ValueError, match="session %d is not open" % a):
        p.timeline(a)
    # a recall's hit is a history.Hit with two attributes more
    from clip_fsar_amd.history import Hit
    from clip_fsar_amd.timeline import RecallHit
    h = RecallHit(b, 2, 17, 0.75, None, bucket=5, above=2)
    assert isinstance(h, Hit) and h == Hit(b, 2, 17, 0.75, None) and (h.window, h.tempo, h.bucket, h.above) == (17, None, 5, 2)
