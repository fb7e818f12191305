"""CPU: the pinned selection of a stream pool with a shortlist (libclipfsar_pool_select.so, include/ext/clipfsar_pool_select.h,
clip_fsar_amd.pool_select_hip, StreamPool(shortlist=...)) -- the plug-in library's exports, ABI check at load, resource report and place
in the build (one more name of the open registry, build.PLUGIN_LIBS); every host validation of cfps_select_pinned without a GPU;
reference_select_pinned on hand-written cases; every refusal of StreamPool(shortlist=...) on stub heads."""
import ctypes
import json
import os
import re
from types import SimpleNamespace as NS

import pytest

import _abi
from _abi import check_abi_at_load, check_exports

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ext", "clipfsar_pool_select.h")
KERNELS = {"select_pinned_kernel": 1}
ROW = _abi._row("pool_select", "pool_select_hip", "cfps_", "ext/clipfsar_pool_select.h",
                "version abi_version last_error workspace_floats select_pinned", KERNELS, 1)
INF, NAN = float("inf"), float("nan")
NONE = 0x7fffffff


@pytest.fixture(scope="module")
def clib():
    import __graft_entry__ as ge
    ge.build()                                    # builds every library (no-op when up to date)
    from clip_fsar_amd import pool_select_hip
    return pool_select_hip.lib()


# ------------------------------------------------------------------ the library and its place in the build
def test_header_exported_exactly_and_arity_matches(clib):
    check_exports(ROW)
    assert ROW.exports == {"cfps_" + e for e in ("version", "abi_version", "last_error", "workspace_floats", "select_pinned")}
    from clip_fsar_amd import pool_select_hip as ph
    from clip_fsar_amd import shortlist_hip as sh
    text = open(HEADER).read()
    for name in ("MAX_KEEP", "MAX_GROUPS", "MAX_STREAMS", "MAX_HOLD", "TABLE_COLS", "Q0", "NQ", "SLOT", "TICK", "PIN_EVENT", "PIN_HOLD"):
        assert int(re.search(r"#define CFPS_%s (\d+)" % name, text).group(1)) == getattr(ph, name), name
    assert ph.MAX_KEEP == sh.MAX_KEEP and ph.MAX_GROUPS == sh.MAX_GROUPS and ph.MAX_HOLD == 1 << 20      # the limits are cfsh_select's
    assert (ph.Q0, ph.NQ) == (sh.Q0, sh.NQ) and (ph.SLOT, ph.TICK) == (2, 3)
    assert int(re.search(r"#define CFPS_NONE (0x[0-9a-f]+)", text).group(1), 16) == ph.NONE == sh.NONE == NONE
    assert [len(ph.SIGNATURES["cfps_" + e]) for e in ("workspace_floats", "select_pinned")] == [2, 24]
    for other in _abi.LIBS:                       # its prefix hides no other library's, and none hides it
        assert not other.prefix.startswith(ROW.prefix) and not ROW.prefix.startswith(other.prefix), other.name
    for prefix in ("cfcs_", "cfev_", "cfbl_", "cfsh_"):
        assert not prefix.startswith(ROW.prefix) and not ROW.prefix.startswith(prefix)
    assert clib.cfps_workspace_floats(3, 5) == 15 == ph.workspace_floats(3, 5)
    for G, NC in ((0, 5), (65537, 5), (3, 0), (65536, 1 << 15), (-1, -1)):
        assert clib.cfps_workspace_floats(G, NC) == -1, (G, NC)
        with pytest.raises(RuntimeError, match="no workspace"):
            ph.workspace_floats(G, NC)
    assert clib.cfps_workspace_floats(65536, (1 << 15) - 1) == 65536 * ((1 << 15) - 1)
    assert ph.table_rows([3, 0, 17], [5, 0, 2], [1, 9, 4]) == ([[0, 3, 5, 1], [3, 0, 0, 9], [3, 17, 2, 4]], 20)


def test_abi_version_is_checked_at_load(clib, monkeypatch):
    check_abi_at_load(ROW, monkeypatch)


def test_the_kernel_is_the_listed_one_and_uses_no_scratch(clib):
    from clip_fsar_amd import build as b
    from clip_fsar_amd import pool_select_hip as ph
    pl = b.PLUGIN_LIBS["pool_select"]
    if not os.path.exists(pl.usage):
        b.build_plugin("pool_select", force=True, verbose=False)
    usage = json.load(open(pl.usage))
    assert len(usage) == ROW.total == sum(KERNELS.values()), sorted(usage)
    for fragment, count in KERNELS.items():
        assert sum(fragment in n for n in usage) == count, (fragment, sorted(usage))
    for n, u in usage.items():
        assert u.get("scratch", 0) == 0 and u.get("spills", 0) == 0, (n, u)
    assert pl.lib == ph.LIB_PATH and pl.lib.endswith(os.sep + "libclipfsar_pool_select.so") and os.path.exists(pl.lib)
    others = [b.USAGE] + [x.usage for reg in (b.SIDE_LIBS, b.EXT_LIBS, b.ADDON_LIBS) for x in reg.values()]
    others += [x.usage for n, x in b.PLUGIN_LIBS.items() if n != "pool_select"]
    for path in others:                           # and no other library's report names it
        if os.path.exists(path):
            assert not any(fragment in n for n in json.load(open(path)) for fragment in KERNELS), path
    # the conventions: the shared error plumbing and the one copy of the select body; no assembly, no allocation, no stream of its own;
    # the only atomic is the histogram count in LDS; no loop that could wait on another workgroup
    source = open(pl.source).read()
    shared = open(os.path.join(b.EXT, "select_keys.h")).read()
    assert '#include "../csrc/side_lib.h"' in source and '#include "../../include/ext/clipfsar_pool_select.h"' in source
    assert '#include "select_keys.h"' in source and '#include "select_keys.h"' in open(b.PLUGIN_LIBS["shortlist"].source).read()
    for text in (source, shared):
        for body in ("asm", "thread_local", "calloc", "malloc", "hipMalloc", "hipStreamCreate", "__builtin_amdgcn_mfma", "hipMemcpy",
                     "hipDeviceSynchronize", "hipStreamSynchronize", "while"):
            assert body not in text, body
    assert len(re.findall(r"atomic\w*\(", source)) == source.count("atomicAdd(&hist[") == 1 and "__shared__ unsigned hist[" in source
    assert not re.findall(r"atomic\w*\(", shared)
    for name in ("score_key(", "kth_largest_key(", "compact_selected(", "block_prefix("):                  # defined once, in the shared header
        assert len(re.findall(r"__device__ __forceinline__ \w+ %s" % re.escape(name), shared)) == 1, name
        assert not re.search(r"__device__ __forceinline__ \w+ %s" % re.escape(name), source), name
        assert not re.search(r"__device__ __forceinline__ \w+ %s" % re.escape(name), open(b.PLUGIN_LIBS["shortlist"].source).read()), name


def test_pool_select_is_a_name_of_the_open_registry_and_follows_the_recipe():
    from clip_fsar_amd import build as b
    assert "pool_select" in b.PLUGIN_LIBS and "pool_select" in b.plugin_lib_names()
    assert all("pool_select" not in reg for reg in (b.SIDE_LIBS, b.EXT_LIBS, b.ADDON_LIBS))
    pl = b.PLUGIN_LIBS["pool_select"]
    assert isinstance(pl, b.ExtLib)
    assert pl.source == os.path.join(b.EXT, "pool_select.hip") and os.path.exists(pl.source)
    assert pl.header == HEADER and os.path.exists(pl.header)
    assert pl.lib == os.path.join(b.HERE, "libclipfsar_pool_select.so")
    assert pl.usage == os.path.join(b.HERE, "build", "pool_select", "resource_usage.json")
    deps = b._plugin_deps("pool_select")
    for f in (pl.source, pl.header, os.path.abspath(b.__file__), os.path.join(b.EXT, "select_keys.h"), os.path.join(b.CSRC, "side_lib.h"),
              os.path.join(b.CSRC, "common.h")):
        assert f in deps, f
    assert os.path.join(b.EXT, "select_keys.h") in b._plugin_deps("shortlist")
    for call in (b.build_side, b._side_deps, b.build_ext, b._ext_deps, b.build_addon, b._addon_deps):       # the three closed registries
        with pytest.raises(KeyError):
            call("pool_select")
    assert not os.path.exists(os.path.join(b.CSRC, "pool_select.hip")) and not os.path.exists(os.path.join(b.CSRC, "select_keys.h"))
    assert not any("pool_select" in open(os.path.join(b.CSRC, f)).read() for f in os.listdir(b.CSRC))      # nothing of csrc/ knows it


def test_staleness_of_the_pool_select_library_and_of_no_other(monkeypatch):
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

    for edited in ("pool_select.hip", "clipfsar_pool_select.h"):                  # its own files: it alone
        assert stale_after(edited) == (set(), {"pool_select"}), edited
    assert stale_after("select_keys.h") == (set(), {"pool_select", "shortlist"})  # the select body's one copy: its two users
    for edited in ("shortlist.hip", "clipfsar_shortlist.h"):
        assert stale_after(edited) == (set(), {"shortlist"}), edited
    for edited in ("otam_tile.h", "fp32_tile_gemm.h", "otam_dp.h"):               # the tile code is the shortlist's, not this library's
        assert stale_after(edited) == (STALE[edited], {"shortlist"}), edited
    for edited in ("side_lib.h", "build.py", "common.h"):                         # what every library reaches
        old, plugins = stale_after(edited)
        assert STALE[edited] <= old and plugins == set(b.PLUGIN_LIBS), edited
    for edited in ("baseline.hip", "clipfsar_baseline.h", "chunk_row.h"):
        assert stale_after(edited) == (set(), {"baseline"}), edited
    for edited in ("pool.hip", "clipfsar_pool.h", "groups.hip", "class_smooth.hip", "events.hip", "gemm.hip"):
        assert "pool_select" not in stale_after(edited)[1], edited
    assert stale_after("no_such_file.h") == (set(), set())


# ------------------------------------------------------------------ validation, without a GPU
def _tbl(rows):
    flat = [v for r in rows for v in r]
    return (ctypes.c_int32 * len(flat))(*flat)


#        Q0  NQ SLOT TICK
GOOD = [[0, 3, 2, 1], [3, 0, 0, 7], [3, 17, 5, 2], [20, 1, 1, 1 << 30]]          # NQ = 21, max_streams 6


def test_select_pinned_validation_without_gpu(clib):
    p = ctypes.c_void_p(4096)                     # never dereferenced: every call below fails validation before any device work
    err, good = clib.cfps_last_error, _tbl(GOOD)

    # select_pinned(S, cols, gens, ev_streak, ev_marks, seen, merit, smooth_marks, base_marks, table_host, table_dev,
    #               G, NQ, NC, keep, hold, max_streams, cap, sel_cols, sel_slots, sel_pin, n_pins, work, stream)
    def call(t=good, G=4, NQ=21, NC=100, keep=8, hold=2, ms=6, cap=300, ptrs=None):
        a = ptrs or [p] * 9 + [t, p] + [p] * 5
        return clib.cfps_select_pinned(*a[:11], G, NQ, NC, keep, hold, ms, cap, *a[11:], None)

    required = [0, 1, 2, 5, 6, 9, 10, 11, 12, 13, 14, 15]
    for i in required:
        ptrs = [p] * 9 + [good, p] + [p] * 5
        ptrs[i] = None
        assert call(ptrs=ptrs) != 0 and b"null pointer" in err(), i
    for i, word in ((3, b"ev_streak null, ev_marks given"), (4, b"ev_streak given, ev_marks null")):     # one without the other
        ptrs = [p] * 9 + [good, p] + [p] * 5
        ptrs[i] = None
        assert call(ptrs=ptrs) != 0 and b"both null or both given" in err() and word in err(), i
    for G in (0, -1, 65537):
        assert call(G=G) != 0 and b"G=" in err(), G
    for NQ in (0, -5):
        assert call(NQ=NQ) != 0 and b"NQ=" in err(), NQ
    for NC in (0, -1):
        assert call(NC=NC) != 0 and b"NC=" in err(), NC
    for keep in (0, -1, 4097):
        assert call(keep=keep) != 0 and b"keep=" in err(), keep
    for hold in (-1, (1 << 20) + 1):
        assert call(hold=hold) != 0 and b"hold=" in err(), hold
    for ms in (0, -1, 65537):
        assert call(ms=ms) != 0 and b"max_streams=" in err(), ms
    for cap in (0, -7):
        assert call(cap=cap) != 0 and b"cap=" in err(), cap
    assert call(ms=65536, cap=1 << 15) != 0 and b"max_streams * cap" in err()     # 2^31 cells
    assert call(ms=3) != 0 and b"G=4 groups for max_streams=3" in err()
    assert call(t=_tbl([[0, 1 << 16, 0, 1]]), G=1, NQ=1 << 16, NC=1 << 15) != 0 and b"NQ * NC" in err()
    big = _tbl([[0, 1, 0, 1]] + [[1, 0, i, 1] for i in range(1, 65536)])
    assert call(t=big, G=65536, NQ=1, NC=1 << 15, ms=65536, cap=1) != 0 and b"G * NC" in err()

    def edit(row, col, value):
        rows = [list(r) for r in GOOD]
        rows[row][col] = value
        return _tbl(rows)

    assert call(t=edit(1, 1, -1)) != 0 and b"group 1" in err() and b"NQ=-1" in err()
    assert call(t=edit(2, 0, 4)) != 0 and b"group 2" in err() and b"Q0=4" in err()                    # the running sum
    assert call(t=edit(0, 0, 1)) != 0 and b"group 0" in err() and b"Q0=1" in err()
    assert call(t=edit(3, 1, 2)) != 0 and b"add up to 22 queries, not to NQ = 21" in err()
    assert call(NQ=20) != 0 and b"not to NQ = 20" in err()
    for slot in (-1, 6):
        assert call(t=edit(2, 2, slot)) != 0 and b"group 2" in err() and b"SLOT=%d outside" % slot in err(), slot
    assert call(t=edit(3, 2, 2)) != 0 and b"SLOT=2 appears twice" in err() and b"group 3" in err()     # a duplicate SLOT
    assert call(t=edit(1, 2, 5)) != 0 and b"SLOT=5 appears twice" in err() and b"group 2" in err()     # also of a group without queries
    for tick in (0, -3):
        assert call(t=edit(1, 3, tick)) != 0 and b"group 1" in err() and b"TICK=%d" % tick in err(), tick


def test_python_wrapper_rejects_cpu_tensors_and_bad_shapes(clib):
    import torch
    from clip_fsar_amd import pool_select_hip as ph
    i32 = dict(dtype=torch.int32)
    S, cols, gens = torch.zeros(3, 5), torch.zeros(5, **i32), torch.zeros(7, **i32)
    plane = lambda: torch.zeros(4, 7, **i32)
    host = torch.tensor([[0, 2, 1, 1], [2, 1, 3, 4]], **i32)
    table = ph.Table(host, host, 2)
    out = lambda: torch.zeros(2, 4, **i32)
    args = lambda: [S, cols, gens, plane(), plane(), plane(), plane(), plane(), plane(), table, 4, 2, out(), out(), out(),
                    torch.zeros(2, **i32), torch.zeros(10)]
    with pytest.raises(RuntimeError, match="HIP device tensor"):
        ph.select_pinned(*args())
    for i, t in ((1, cols[:4]), (2, gens[:6]), (3, plane()[:3]), (6, plane()[:, :6]), (7, plane()[:2]), (8, plane()[:, :1]),
                 (12, out()[:, :3]), (13, out()[:1]), (14, out()[:, :2]), (15, torch.zeros(3, **i32)), (16, torch.zeros(9)), (10, 9)):
        a = args()
        a[i] = t
        with pytest.raises(RuntimeError, match="shape"):
            ph.select_pinned(*a)
    a = args()
    a[9] = ph.Table(host[:, :2], host[:, :2], 2)
    with pytest.raises(RuntimeError, match="table must be a Table"):
        ph.select_pinned(*a)


# ------------------------------------------------------------------ the rule, on hand-written cases
def _sel(S, counts, keep, pinned):
    from clip_fsar_amd.shortlist import reference_select_pinned
    return reference_select_pinned(S, counts, keep, pinned)


def test_reference_select_pinned_without_pins_is_reference_select():
    from clip_fsar_amd.shortlist import reference_select
    S = [[NAN, 1.0, 5.0, NAN, -0.0],
         [7.0, NAN, 2.0, NAN, 0.0],
         [0.0, NAN, 9.0, 8.0, -INF]]
    for counts in ([3], [2, 1], [1, 0, 2], [1, 1, 1]):
        for keep in (1, 2, 4, 5, 9):
            cols, pins, n = _sel(S, counts, keep, [None] * len(counts))
            assert cols == reference_select(S, counts, keep) and n == [0] * len(counts)
            assert pins == [[0] * min(keep, 5)] * len(counts)
            assert _sel(S, counts, keep, [{}] * len(counts)) == (cols, pins, n)


def test_reference_select_pinned_keeps_every_pin_when_they_fit():
    S = [[5.0, 3.0, 3.0, 3.0, 1.0, 3.0]]
    assert _sel(S, [1], 3, [{4: 1}]) == ([[0, 1, 4]], [[0, 0, 1]], [1])            # the worst score stays; the rest by score, then column
    assert _sel(S, [1], 3, [{4: 1, 5: 2}]) == ([[0, 4, 5]], [[0, 1, 2]], [2])
    assert _sel(S, [1], 3, [{4: 1, 5: 2, 2: 3}]) == ([[2, 4, 5]], [[3, 1, 2]], [3])   # P = K: the pins and nothing else, not even the 5.0
    assert _sel(S, [1], 9, [{4: 2}]) == ([[0, 1, 2, 3, 4, 5]], [[0, 0, 0, 0, 2, 0]], [1])


def test_reference_select_pinned_a_pin_on_a_column_without_a_score():
    S = [[NAN, 4.0, -INF, 2.0, NAN]]
    assert _sel(S, [1], 2, [{0: 1}]) == ([[0, 1]], [[1, 0]], [1])                   # a NaN column, pinned: kept whatever its score
    assert _sel(S, [1], 3, [{0: 1, 2: 2}]) == ([[0, 1, 2]], [[1, 0, 2]], [2])       # and a -inf one
    assert _sel(S, [1], 5, [{4: 1}]) == ([[1, 3, 4, NONE, NONE]], [[0, 0, 1, 0, 0]], [1])      # the padding is behind the pin


def test_reference_select_pinned_more_pins_than_places():
    # pins 0 (3.0), 1 (NaN: no score), 2 (3.0), 3 (-0.0), 4 (0.0), 5 (3.0), 6 (-inf: no score); column 7 (9.0) is not pinned
    S = [[3.0, NAN, 3.0, -0.0, 0.0, 3.0, -INF, 9.0]]
    pins = {c: 1 + c % 3 for c in range(7)}
    assert _sel(S, [1], 1, [pins]) == ([[0]], [[1]], [7])                          # the best pin, the lowest column of the tie; never 7
    assert _sel(S, [1], 2, [pins]) == ([[0, 2]], [[1, 3]], [7])
    assert _sel(S, [1], 4, [pins]) == ([[0, 2, 3, 5]], [[1, 3, 1, 3]], [7])         # both zeros are equal: the lower column
    assert _sel(S, [1], 5, [pins]) == ([[0, 2, 3, 4, 5]], [[1, 3, 1, 2, 3]], [7])
    assert _sel(S, [1], 6, [pins]) == ([[0, 1, 2, 3, 4, 5]], [[1, 2, 3, 1, 2, 3]], [7])       # a pin without a score: below every score,
    assert _sel(S, [1], 7, [pins]) == ([[0, 1, 2, 3, 4, 5, 6]], [[1, 2, 3, 1, 2, 3, 1]], [7])  # the lower column first; P = K
    assert _sel(S, [1], 8, [pins])[0] == [list(range(8))]


def test_reference_select_pinned_a_group_without_windows_and_bad_arguments():
    S = [[1.0, 2.0], [4.0, 3.0]]
    assert _sel(S, [1, 0, 1], 1, [{0: 1}, {1: 2}, None]) == ([[0], [NONE], [0]], [[1], [0], [0]], [1, 0, 0])
    assert _sel([], [0], 3, [None]) == ([[]], [[]], [0])
    with pytest.raises(ValueError, match="add up to"):
        _sel([[1.0]], [2], 1, [None])
    with pytest.raises(ValueError, match="pins for 1"):
        _sel(S, [1, 1], 1, [None])
    for bad in ({2: 1}, {-1: 1}, {0: 0}):
        with pytest.raises(ValueError, match="a pin names a column outside"):
            _sel(S, [2], 1, [bad])


# ------------------------------------------------------------------ StreamPool's option, on stub heads
def _stub_head(T=4, **train):
    engine = NS(arch={"embed": 8})
    return NS(args=NS(TRAIN=NS(**train), DATA=NS(NUM_INPUT_FRAMES=T)), _get_engine=lambda dev: engine, _engine_key=("stub",),
              arch_name="stub", precision="fp32", depth=1)


def _live(capacity=4, ids=(0, 1, 2)):
    from clip_fsar_amd import live_gallery as lg
    g = lg.LiveGallery(_stub_head(), "cpu", capacity=capacity)
    if ids:
        g._install(lg.plan_add(g._book, list(ids)).book)       # registered on the host alone: nothing below reaches the device
    return g


def test_stream_pool_shortlist_refusals_are_raised_before_the_device_is_touched():
    from clip_fsar_amd import pool as pm
    from clip_fsar_amd.baseline import Baseline
    from clip_fsar_amd.events import EventRule
    from clip_fsar_amd.pool import StreamPool
    from clip_fsar_amd.shortlist import Shortlist
    from clip_fsar_amd.stream import StreamOutput
    g, other = _live(), _live()
    sl = Shortlist(g, keep=2)
    rule, base = EventRule(0.6, 0.4, 2, 2), Baseline()
    p = StreamPool(g, max_streams=3, smooth=0.5, smooth_by="class", events=rule, baseline=base, shortlist=sl, shortlist_hold=2)
    assert p._shortlist is sl and p._hold == 2 and p._sl_cells.planes is None
    assert StreamPool(g, shortlist=sl)._hold == 0 and StreamPool(g, shortlist=sl, shortlist_hold=1 << 20)._hold == 1 << 20
    # the two names are keyword-only, and events / baseline are still the 9th and 10th positional arguments
    q = StreamPool(g, 3, 1, 1, 64, 0.5, None, "class", rule, base, shortlist=sl)
    assert q._events is rule and q._baseline is base and q._shortlist is sl
    assert StreamPool(g, 3, 1, 1, 64, 0.5, None, "class", rule)._baseline is None
    for args, kw in (((rule, base, sl), {}), ((rule,), {"events": rule}), ((rule, base), {"baseline": base})):
        with pytest.raises(TypeError, match="StreamPool: at most 10 positional arguments"):
            StreamPool(g, 3, 1, 1, 64, 0.5, None, "class", *args, **kw)
    for bad in ("shortlist", 64, g, (g, 64)):
        with pytest.raises(TypeError, match="StreamPool: shortlist must be a Shortlist"):
            StreamPool(g, shortlist=bad)
    with pytest.raises(ValueError, match="StreamPool: shortlist= was built over another gallery"):
        StreamPool(other, shortlist=sl)
    for smooth_by in ({}, {"smooth_by": "column"}):
        with pytest.raises(ValueError, match="shortlist=.*smooth > 0.*smooth_by=\"class\""):
            StreamPool(g, smooth=0.5, shortlist=sl, **smooth_by)
    assert StreamPool(g, smooth=0.0, smooth_by="column", shortlist=sl)._by_class is False          # smooth = 0: the option is inert
    for hold in (-1, (1 << 20) + 1, True, 2.0, "2"):
        with pytest.raises(ValueError, match=r"StreamPool: shortlist_hold must be an integer in \[0, 2\^20\]"):
            StreamPool(g, shortlist=sl, shortlist_hold=hold)
    for hold in (0, 2):
        with pytest.raises(ValueError, match="StreamPool: shortlist_hold = %d is given without shortlist=" % hold):
            StreamPool(g, shortlist_hold=hold)
    with pytest.raises(ValueError, match="shortlist= keeps a state cell.*2\\^31"):
        big = _live(1 << 15)
        StreamPool(big, max_streams=1 << 16, shortlist=Shortlist(big))
    with pytest.raises(ValueError, match=r"open\(classes=\) on a pool with shortlist= is not supported.*out of scope"):
        p.open(classes=[0, 1])
    h = p.open()
    assert p._sl_cells.forgotten == {0} == p._ev_cells.forgotten and p._sessions[h].tick == 0
    with pytest.raises(ValueError, match=r"enroll\(join=True\) on a pool with shortlist= is not supported.*out of scope"):
        p.enroll(h, 7, join=True)
    assert p.active(h) == [] and p.baseline(h) == []
    assert p.stats() == {"frames": 0, "tower_frames": 0, "windows": 0, "events": 0, "events_dropped": 0, "pins": 0, "pins_dropped": 0,
                         "open": 1}
    p.reset(h)
    assert p._sl_cells.forgotten == {0}
    # a pool without the option is the pool as it was
    plain = StreamPool(g, smooth=0.5, smooth_by="class", events=rule)
    assert plain._shortlist is None and not hasattr(plain, "_sl_cells") and "pins" not in plain.stats()
    assert plain.open(classes=[0, 1]) == 0
    # the output types: subclasses of the plain ones with the same tuple
    for plain_type, mine, both in ((pm.PackedOutput, pm.ShortlistPackedOutput, pm.DeviationShortlistPackedOutput),
                                   (StreamOutput, pm.ShortlistStreamOutput, pm.DeviationShortlistStreamOutput)):
        assert issubclass(mine, plain_type) and issubclass(both, mine) and mine._fields == both._fields == plain_type._fields
        n = len(plain_type._fields)
        o = both(*range(n), deviation="d", columns="c", pinned="p", ids=("x",))
        assert tuple(o) == tuple(range(n)) and (o.deviation, o.columns, o.pinned) == ("d", "c", "p")
    assert g._store is None and sl._coarse is None and sl.stats == {"calls": 0, "refreshed": 0}
