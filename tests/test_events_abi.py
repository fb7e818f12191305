"""CPU: stream events (libclipfsar_events.so, include/ext/clipfsar_events.h, clip_fsar_amd.events_hip, clip_fsar_amd.events) -- the add-on
library's exports, ABI check at load, resource report and place in the build (a third registry, build.ADDON_LIBS); the host validation of
cfev_detect without a GPU; EventRule; reference_events and the translator on hand-written cases; StreamPool's events= option on stub heads."""
import ctypes
import json
import os
import random
import re
from types import SimpleNamespace as NS

import pytest

import _abi
from _abi import check_abi_at_load, check_exports

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ext", "clipfsar_events.h")
KERNELS = {"event_count_kernel": 1, "event_scan_kernel": 1, "event_emit_kernel": 1}
ROW = _abi._row("events", "events_hip", "cfev_", "ext/clipfsar_events.h", "version abi_version last_error workspace_ints detect", KERNELS, 3)


@pytest.fixture(scope="module")
def clib():
    import __graft_entry__ as ge
    ge.build()                                    # builds every library (no-op when up to date)
    from clip_fsar_amd import events_hip
    return events_hip.lib()


# ------------------------------------------------------------------ the library and its place in the build
def test_header_exported_exactly_and_arity_matches(clib):
    check_exports(ROW)
    assert ROW.exports == {"cfev_version", "cfev_abi_version", "cfev_last_error", "cfev_workspace_ints", "cfev_detect"}
    from clip_fsar_amd import class_smooth_hip as ch
    from clip_fsar_amd import events as ev
    from clip_fsar_amd import events_hip as eh
    text = open(HEADER).read()
    smooth = open(os.path.join(ROOT, "include", "ext", "clipfsar_class_smooth.h")).read()
    for name in ("MAX_STREAMS", "CHUNK", "TABLE_COLS", "SLOT", "NW", "OUT0", "NC", "KEY0", "CHUNK0"):       # the table is CFCS_*'s, redeclared
        mine = int(re.search(r"#define CFEV_%s (\d+)" % name, text).group(1))
        assert mine == int(re.search(r"#define CFCS_%s (\d+)" % name, smooth).group(1)) == getattr(eh, name) == getattr(ch, name), name
    for name, value in (("ONSET", 1), ("OFFSET", 2), ("EVENT_COLS", 5), ("VALUE_COLS", 2)):
        assert int(re.search(r"#define CFEV_%s (\d+)" % name, text).group(1)) == getattr(eh, name) == value, name
    assert (ev.ONSET, ev.OFFSET) == (eh.ONSET, eh.OFFSET) and eh.plan_rows is ch.plan_rows
    assert len(eh.SIGNATURES["cfev_detect"]) == 24
    for other in _abi.LIBS:                       # its prefix hides no other library's, and none hides it
        assert not other.prefix.startswith(ROW.prefix) and not ROW.prefix.startswith(other.prefix), other.name
    assert clib.cfev_workspace_ints(1) == 257 and clib.cfev_workspace_ints(832) == 832 * 257
    assert clib.cfev_workspace_ints(0) == -1 and clib.cfev_workspace_ints(-3) == -1 and clib.cfev_workspace_ints(1 << 23) == -1
    assert eh.workspace_ints(13) == 13 * 257
    with pytest.raises(RuntimeError, match="workspace"):
        eh.workspace_ints(0)


def test_abi_version_is_checked_at_load(clib, monkeypatch):
    check_abi_at_load(ROW, monkeypatch)


def test_the_kernels_are_the_listed_ones_and_use_no_scratch(clib):
    from clip_fsar_amd import build as b
    from clip_fsar_amd import events_hip as eh
    al = b.ADDON_LIBS["events"]
    if not os.path.exists(al.usage):
        b.build_addon("events", force=True, verbose=False)
    usage = json.load(open(al.usage))
    assert len(usage) == ROW.total == 3, sorted(usage)
    for fragment, count in KERNELS.items():
        assert sum(fragment in n for n in usage) == count, (fragment, sorted(usage))
    for n, u in usage.items():
        assert u.get("scratch", 0) == 0 and u.get("spills", 0) == 0, (n, u)
    assert os.path.normpath(al.usage).endswith(os.path.join("build", "events", "resource_usage.json"))
    assert al.lib == eh.LIB_PATH and al.lib.endswith(os.sep + "libclipfsar_events.so") and os.path.exists(al.lib)
    assert os.path.normpath(al.source).endswith(os.path.join("clip-fsar_amd", "ext", "events.hip")) and al.header == HEADER
    others = [b.USAGE] + [sl.usage for sl in b.SIDE_LIBS.values()] + [el.usage for el in b.EXT_LIBS.values()]
    assert len(others) == 12
    for path in others:                           # and no other library's report holds one of them
        names = json.load(open(path))
        assert not any(fragment in n for n in names for fragment in KERNELS), path
    source = open(al.source).read()               # plain C++ on the shared error plumbing: no assembly, no allocation, no stream, no atomics
    assert '#include "../csrc/side_lib.h"' in source and '#include "../../include/ext/clipfsar_events.h"' in source
    for body in ("asm", "thread_local", "calloc", "hipMalloc", "hipStreamCreate", "atomic", "__builtin_amdgcn"):
        assert body not in source, body


def test_three_registries():
    from clip_fsar_amd import build as b
    assert list(b.ADDON_LIBS) == b.addon_lib_names() == ["events"]
    assert b.ADDON_LIBS is not b.EXT_LIBS and b.ADDON_LIBS is not b.SIDE_LIBS
    assert not set(b.ADDON_LIBS) & set(b.SIDE_LIBS) and not set(b.ADDON_LIBS) & set(b.EXT_LIBS)
    assert all(isinstance(v, b.ExtLib) for v in b.ADDON_LIBS.values())
    for call in (b._addon_deps, b.build_addon):
        with pytest.raises(KeyError):
            call("pool")
        with pytest.raises(KeyError):
            call("class_smooth")
    for call in (b.build_ext, b._ext_deps, b.build_side):
        with pytest.raises(KeyError):
            call("events")
    libs = [b.LIB] + [x.lib for reg in (b.SIDE_LIBS, b.EXT_LIBS, b.ADDON_LIBS) for x in reg.values()]
    reports = [b.USAGE] + [x.usage for reg in (b.SIDE_LIBS, b.EXT_LIBS, b.ADDON_LIBS) for x in reg.values()]
    assert len(set(libs)) == len(set(reports)) == 13
    assert not os.path.exists(os.path.join(b.CSRC, "events.hip"))


def test_staleness_of_the_add_on_and_of_nothing_else(monkeypatch):
    from clip_fsar_amd import build as b
    from test_build_recipe import NAMES, STALE, P
    monkeypatch.setattr(b.os.path, "exists", lambda p: True)

    def stale_after(edited):
        monkeypatch.setattr(b.os.path, "getmtime", lambda p: 2.0 if p.endswith(os.sep + edited) else 1.0)
        old = {P} if b._stale(b.LIB, b._product_deps()) else set()
        old |= {n for n in NAMES if b._stale(b.SIDE_LIBS[n].lib, b._side_deps(n))}
        old |= {n for n in b.EXT_LIBS if b._stale(b.EXT_LIBS[n].lib, b._ext_deps(n))}
        return old, b._stale(b.ADDON_LIBS["events"].lib, b._addon_deps("events"))

    for edited in ("events.hip", "clipfsar_events.h"):                            # the add-on's own files: it alone
        assert stale_after(edited) == (set(), True), edited
    for edited in ("side_lib.h", "build.py", "common.h"):                         # shared: the others as their matrix has it
        assert stale_after(edited) == (STALE[edited] | {"class_smooth"}, True), edited
    for edited in ("pool.hip", "clipfsar_pool.h", "otam_tile.h", "gemm.hip"):
        assert stale_after(edited) == (STALE[edited], False), edited
    for edited in ("class_smooth.hip", "clipfsar_class_smooth.h"):                # the extension's own files leave the add-on alone
        assert stale_after(edited) == ({"class_smooth"}, False), edited
    assert stale_after("no_such_file.h") == (set(), False)


# ------------------------------------------------------------------ validation, without a GPU
def _tbl(rows):
    flat = [v for r in rows for v in r]
    return (ctypes.c_int32 * len(flat))(*flat)


#        slot nW out0 NC key0 chunk0
GOOD = [[2, 2, 0, 300, 0, 0],                    # two chunks of 256 columns
        [0, 0, 600, 3, 300, 2],                  # no windows
        [1, 5, 600, 256, 44, 3]]                 # a list that overlaps the first; NOUT = 600 + 1280, NKEYS = 303, max_streams 4, cap 300
NOUT, NKEYS = 1880, 303


def _edit(row, col, value):
    rows = [list(r) for r in GOOD]
    rows[row][col] = value
    return _tbl(rows)


def test_argument_validation_without_gpu(clib):
    p = ctypes.c_void_p(4096)                     # never dereferenced: every call below fails validation before any device work
    err, good = clib.cfev_last_error, _tbl(GOOD)
    # detect(scores, streak, length, peak, marks, gens, keys, events, values, n_events, work, table_host, table_dev,
    #        S, NOUT, NKEYS, max_streams, cap, on, off, min_on, min_off, max_events, stream)

    def call(t, S=3, nout=NOUT, nkeys=NKEYS, ms=4, cap=300, on=0.6, off=0.4, min_on=2, min_off=2, max_events=64):
        return clib.cfev_detect(p, p, p, p, p, p, p, p, p, p, p, t, p, S, nout, nkeys, ms, cap, on, off, min_on, min_off, max_events, None)

    for i in range(13):
        args = [p] * 11 + [good, p]
        args[i] = None
        assert clib.cfev_detect(*args, 3, NOUT, NKEYS, 4, 300, 0.6, 0.4, 2, 2, 64, None) != 0 and b"null" in err(), i
    for on, off in ((float("nan"), 0.4), (0.6, float("nan")), (float("inf"), 0.4), (0.6, float("-inf"))):
        assert call(good, on=on, off=off) != 0 and b"finite" in err(), (on, off)
    assert call(good, on=0.4, off=0.6) != 0 and b"above" in err()
    for kw in ({"min_on": 0}, {"min_off": 0}, {"min_on": -2}, {"min_off": -1}):
        assert call(good, **kw) != 0 and b"min_on" in err() and b"at least 1" in err(), kw
    for max_events in (0, -5):
        assert call(good, max_events=max_events) != 0 and b"max_events" in err(), max_events
    for ms in (0, -1, 65537, 1 << 20):
        assert call(good, ms=ms) != 0 and b"max_streams" in err(), ms
    for S in (0, -2, 5):                          # no rows; more rows than slots
        assert call(good, S=S) != 0 and b"rows" in err(), S
    for cap in (0, -7):
        assert call(good, cap=cap) != 0 and b"cap=" in err(), cap
    assert call(good, ms=65536, cap=1 << 15) != 0 and b"too large" in err()       # 2^31 cells
    assert call(good, nout=-1) != 0 and b"bad shape" in err()
    assert call(good, nkeys=0) != 0 and b"bad shape" in err()

    def rejected(table, row, *words, **kw):
        assert call(table, **kw) != 0 and all(w in err() for w in words + (b"row %d" % row,)), (row, words, err())

    for slot in (-1, 4):
        rejected(_edit(1, 0, slot), 1, b"slot", b"outside")
    rejected(_edit(2, 0, 2), 2, b"appears twice")
    rejected(_edit(0, 1, -1), 0, b"negative count")
    for NC in (0, -3):
        rejected(_edit(1, 3, NC), 1, b"width")
    rejected(_edit(1, 2, 599), 1, b"prefix sums")         # OUT0
    rejected(_edit(2, 2, 603), 2, b"prefix sums")
    rejected(_edit(0, 2, 1), 0, b"prefix sums")
    rejected(_edit(1, 5, 1), 1, b"prefix sums")           # CHUNK0: the first row has two chunks
    rejected(_edit(2, 5, 2), 2, b"prefix sums")
    rejected(_edit(2, 4, -1), 2, b"keys[")                # KEY0 below 0, and the list's end beyond NKEYS
    rejected(_edit(2, 4, 48), 2, b"keys[")
    rejected(_edit(0, 4, 4), 0, b"keys[")
    rejected(good, 0, b"keys[", nkeys=299)
    rejected(good, 1, b"keys[", nkeys=302)
    assert call(good, nout=NOUT + 1) != 0 and b"not to NOUT" in err()
    assert call(good, nout=NOUT - 1) != 0 and b"not to NOUT" in err()
    # products beyond 2^31: 40 000 windows x 60 000 columns
    big = _tbl([[0, 40000, 0, 60000, 0, 0]])
    assert call(big, S=1, nout=0, nkeys=60000, cap=60000) != 0 and b"too large" in err() and b"row 0" in err()
    # a table without a window is valid and launches nothing; on == off is a valid rule
    assert call(_tbl([[3, 0, 0, 7, 0, 0]]), S=1, nout=0, nkeys=7, on=0.5, off=0.5) == 0, err()


def test_python_wrapper_rejects_cpu_tensors_and_bad_shapes(clib):
    import torch
    from clip_fsar_amd import events_hip as eh
    host = torch.tensor(GOOD, dtype=torch.int32)
    table = eh.Table(host, host, 3)
    i32 = dict(dtype=torch.int32)
    x, st, ln, pk, mk = torch.zeros(NOUT), torch.zeros(4, 300, **i32), torch.zeros(4, 300, **i32), torch.zeros(4, 300), torch.zeros(4, 300, **i32)
    gens, keys = torch.ones(300, **i32), torch.zeros(NKEYS, **i32)
    ev, va, n, work = torch.zeros(8, 5, **i32), torch.zeros(8, 2), torch.zeros(1, **i32), torch.zeros(4 * 257, **i32)
    good = [x, st, ln, pk, mk, gens, keys, ev, va, n, work]
    with pytest.raises(RuntimeError, match="HIP device tensor"):
        eh.detect(*good, table, 0.6, 0.4, 1, 1)
    for at, bad in ((0, x.view(2, -1)), (2, ln[:3]), (3, pk[:, :299]), (4, mk[:3]), (5, gens[:299]), (6, keys.view(1, -1)), (7, ev[:, :4]),
                    (7, ev[:0]), (8, va[:7]), (9, torch.zeros(2, **i32)), (10, work[:4 * 257 - 1]), (10, work.view(4, 257))):
        args = list(good)
        args[at] = bad
        with pytest.raises(RuntimeError, match="shape|flat|work holds"):
            eh.detect(*args, table, 0.6, 0.4, 1, 1)
    with pytest.raises(RuntimeError, match="table must be a Table"):
        eh.detect(*good, eh.Table(host[:, :5], host[:, :5], 3), 0.6, 0.4, 1, 1)


# ------------------------------------------------------------------ the rule, the reference and the translator
def test_event_rule_errors_name_the_field():
    from clip_fsar_amd.events import EventRule
    r = EventRule(0.6, 0.4)
    assert r == (0.6, 0.4, 1, 1, 4096) and r._fields == ("on", "off", "min_on", "min_off", "max_events")
    assert EventRule(on=1, off=1, min_on=3, min_off=2, max_events=7) == (1.0, 1.0, 3, 2, 7)
    for kw, field in (({"on": float("nan")}, "on"), ({"on": float("inf")}, "on"), ({"on": 1e39}, "on"), ({"on": "1"}, "on"),
                      ({"on": True}, "on"), ({"off": float("nan")}, "off"), ({"off": float("-inf")}, "off"), ({"off": None}, "off"),
                      ({"off": 0.7}, "off"), ({"min_on": 0}, "min_on"), ({"min_on": 1.0}, "min_on"), ({"min_on": True}, "min_on"),
                      ({"min_off": -1}, "min_off"), ({"min_off": 1 << 31}, "min_off"), ({"max_events": 0}, "max_events"),
                      ({"max_events": 2.5}, "max_events")):
        with pytest.raises(ValueError, match="EventRule: %s " % field):
            EventRule(**dict({"on": 0.6, "off": 0.4}, **kw))


def _records(scores, rule, cell=None):
    from clip_fsar_amd.events import reference_events
    recs, cell = reference_events(scores, rule, cell)
    return [tuple(r) for r in recs], tuple(cell)


def test_reference_events_on_hand_written_cases():
    from clip_fsar_amd.events import EventRule
    nan = float("nan")
    ON, OFF = 1, 2
    # min 1 / 1: the alternating column gives an event every window; the window of one transition never counts towards the other
    recs, cell = _records([1.0, 0.0, 1.0, 0.0, 1.0], EventRule(0.5, 0.5))
    assert recs == [(0, ON, 1, 1.0, 1.0), (1, OFF, 1, 0.0, 1.0), (2, ON, 1, 1.0, 1.0), (3, OFF, 1, 0.0, 1.0), (4, ON, 1, 1.0, 1.0)]
    assert cell == (-1, 1, 1.0)
    # the band between off and on holds the state both ways; the peak of an idle streak restarts with the streak
    rule = EventRule(0.6, 0.4, min_on=2, min_off=2)
    s = [0.7, 0.5, 0.9, 0.65, 0.5, 0.3, 0.5, 0.3, 0.2, 0.8]
    #    on   -    on   ON    .    b    .    b    OFF  on
    recs, cell = _records(s, rule)
    assert recs == [(3, ON, 2, 0.65, 0.9), (8, OFF, 5, 0.2, 0.9)] and cell == (1, 7, 0.8)
    # NaN: ends an idle streak, and ends a run below off; it still extends the event, and fmaxf ignores it
    recs, cell = _records([0.7, nan, 0.7, 0.8, 0.1, nan, 0.1, 0.1], rule)
    assert recs == [(3, ON, 2, 0.8, 0.8), (7, OFF, 4, 0.1, 0.8)] and cell[0] == 0
    # from a cell: an active one with one window below off; a saturated length stays
    recs, cell = _records([0.1], rule, (-2, 9, 0.95))
    assert recs == [(0, OFF, 8, 0.1, 0.95)] and cell == (0, 10, 0.95)
    recs, cell = _records([0.9], rule, (-1, (1 << 31) - 1, 0.5))
    assert recs == [] and cell == (-1, (1 << 31) - 1, 0.9)
    # the thresholds compare as fp32: 0.6 as fp32 lies above the double 0.6
    assert _records([0.6], EventRule(0.6, 0.4))[0] == [] and len(_records([0.6000000238418579], EventRule(0.6, 0.4))[0]) == 1


def test_reference_events_do_not_depend_on_the_split():
    """uniform scores, 257 columns x 12 windows, four rule pairs -- hundreds of events of both kinds each, and the
    stream is the same however the windows are cut into calls"""
    from clip_fsar_amd.events import EventRule
    rng = random.Random(5)
    import struct
    cols = [[struct.unpack("f", struct.pack("f", rng.random()))[0] for _ in range(12)] for _ in range(257)]
    for (min_on, min_off), least in (((1, 1), 800), ((2, 2), 200), ((3, 2), 80), ((2, 3), 150)):
        rule = EventRule(0.6, 0.4, min_on, min_off)
        total, kinds = 0, set()
        for col in cols:
            whole, cell = _records(col, rule)
            for cuts in ((5, 5, 12), tuple(range(1, 13)), (0, 12, 12)):
                got, c, k0 = [], None, 0
                for k1 in cuts:
                    part, c = _records(col[k0:k1], rule, c)
                    got += [(r[0] + k0,) + r[1:] for r in part]
                    k0 = k1
                assert got == whole and c == cell, cuts
            total += len(whole)
            kinds |= {r[1] for r in whole}
        assert total >= least and kinds == {1, 2}, (min_on, min_off, total)


def test_the_translator():
    from clip_fsar_amd.events import Event, EventRule, translate
    rule = EventRule(0.6, 0.4, min_on=3, min_off=2)
    # records arrive ordered by (row, column, window); rows 0 and 1 are sessions 7 and 4, with first windows 10 and 0
    events = [[0, 0, 4, 1, 3], [0, 2, 1, 2, 6], [0, 2, 4, 1, 3], [1, 1, 0, 2, 9], [1, 1, 3, 1, 3], [9, 9, 9, 9, 9]]
    values = [[0.7, 0.9], [0.1, 0.95], [0.8, 0.8], [0.2, 0.7], [0.61, 0.75], [0.0, 0.0]]
    got = translate(events, values, 5, [7, 4], [10, 0], [("a", "b", "c"), [5, 6]], rule)
    assert got == [Event(7, "c", "offset", 11, 4, 6, 0.1, 0.95),          # window, then column within a session
                   Event(7, "a", "onset", 14, 12, 3, 0.7, 0.9),
                   Event(7, "c", "onset", 14, 12, 3, 0.8, 0.8),
                   Event(4, 6, "offset", 0, -10, 9, 0.2, 0.7),            # an event older than the session's counter start
                   Event(4, 6, "onset", 3, 1, 3, 0.61, 0.75)]
    assert Event._fields == ("session", "class_id", "kind", "window", "start", "length", "score", "peak")
    assert translate(events, values, 0, [7, 4], [10, 0], [("a", "b", "c"), [5, 6]], rule) == []
    assert len(translate(events[:3], values[:3], 40, [7, 4], [10, 0], [("a", "b", "c"), [5, 6]], rule)) == 3    # n is the true total
    import torch
    assert translate(torch.tensor(events), torch.tensor(values, dtype=torch.float64), 5, [7, 4], [10, 0], [("a", "b", "c"), [5, 6]], rule) == got


# ------------------------------------------------------------------ StreamPool's option, on stub heads
def _stub_head(T=4, **train):
    engine = NS(arch={"embed": 8})
    return NS(args=NS(TRAIN=NS(**train), DATA=NS(NUM_INPUT_FRAMES=T)), _get_engine=lambda dev: engine, _engine_key=("stub",),
              arch_name="stub", precision="fp32", depth=1)


def _live(kind, capacity):
    from clip_fsar_amd.live_gallery import LiveGallery
    from clip_fsar_amd.live_text_gallery import LiveTextGallery
    if kind == "live":
        return LiveGallery(_stub_head(), "cpu", capacity=capacity)
    return LiveTextGallery(_stub_head(COMBINE=True), "cpu", capacity=capacity)


def test_the_events_option_on_stub_heads():
    from clip_fsar_amd.events import EventRule
    from clip_fsar_amd.gallery import SupportGallery
    from clip_fsar_amd.pool import StreamPool
    from clip_fsar_amd.text_gallery import TextGallery
    rule = EventRule(0.6, 0.4, 2, 2)
    live = _live("live", 4)
    p = StreamPool(live, max_streams=3, smooth=0.5, smooth_by="class", events=rule)          # TypeError without the feature
    assert p.stats() == {"frames": 0, "tower_frames": 0, "windows": 0, "events": 0, "events_dropped": 0, "open": 0}
    assert p.take_events() == []
    h = p.open()
    assert p.active(h) == [] and p._ev_cells.forgotten == {0} == p._smooth_cells.forgotten
    assert StreamPool(_live("live_text", 4), events=rule).stats()["events"] == 0                 # no smoothing: the logits are scored
    assert StreamPool(live, smooth=0.0, smooth_by="column", events=rule)._by_class is False
    plain = StreamPool(live, smooth=0.5, smooth_by="class")
    assert set(plain.stats()) == {"frames", "tower_frames", "windows", "open"} and not hasattr(plain, "_ev_queue")
    for call in (plain.take_events, lambda: plain.active(plain.open())):
        with pytest.raises(ValueError, match="no event rule"):
            call()
    for g in (SupportGallery(_stub_head(), "cpu"), TextGallery(_stub_head(COMBINE=True), "cpu")):
        with pytest.raises(ValueError, match="events=.*slot store.*%s" % type(g).__name__):
            StreamPool(g, events=rule)
    for smooth_by in ({}, {"smooth_by": "column"}):
        with pytest.raises(ValueError, match="events=.*smooth > 0.*smooth_by=\"class\""):
            StreamPool(live, smooth=0.5, events=rule, **smooth_by)
    with pytest.raises(ValueError, match="events= keeps a state cell.*2\\^31"):
        StreamPool(_live("live", 1 << 15), max_streams=1 << 16, events=rule)
    for bad in ((0.6, 0.4), "rule", 1, {"on": 0.6}):
        with pytest.raises(TypeError, match="EventRule"):
            StreamPool(live, events=bad)
    with pytest.raises(ValueError, match="session 99 is not open"):
        p.active(99)
