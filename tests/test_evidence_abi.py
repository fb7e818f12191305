"""CPU: event evidence (libclipfsar_evidence.so, include/ext/clipfsar_evidence.h, clip_fsar_amd.evidence_hip, clip_fsar_amd.evidence,
StreamPool(evidence=...)) -- the plug-in library's exports, ABI check at load, resource report and place in the build (one more name of
the open registry, build.PLUGIN_LIBS); every host validation of cfed_capture without a GPU; reference_capture on hand-written cases, a
tempo shift against a brute-force list of frame numbers; Evidence's refusals; every refusal of StreamPool(evidence=...) and of the event
methods on stub heads."""
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
HEADER = os.path.join(ROOT, "include", "ext", "clipfsar_evidence.h")
KERNELS = {"evidence_place_kernel": 1, "evidence_copy_kernel": 2}                # the copy in its 16-byte and its 4-byte form
ROW = _abi._row("evidence", "evidence_hip", "cfed_", "ext/clipfsar_evidence.h", "version abi_version last_error workspace_ints capture",
                KERNELS, 3)


@pytest.fixture(scope="module")
def clib():
    import __graft_entry__ as ge
    ge.build()                                    # builds every library (no-op when up to date)
    from clip_fsar_amd import evidence_hip
    return evidence_hip.lib()


# ------------------------------------------------------------------ the library and its place in the build
def test_header_exported_exactly_and_arity_matches(clib):
    check_exports(ROW)
    assert ROW.exports == {"cfed_" + e for e in ("version", "abi_version", "last_error", "workspace_ints", "capture")}
    from clip_fsar_amd import evidence as em
    from clip_fsar_amd import evidence_hip as eh
    text = open(HEADER).read()
    define = lambda name: int(re.search(r"#define CFED_%s \(?(-?\d+)\)?" % name, text).group(1))
    assert define("ABI_VERSION") == eh.ABI_VERSION == 1
    assert define("TABLE_COLS") == eh.TABLE_COLS == em.TABLE_COLS == 6
    assert [define(n) for n in ("SLOT", "POS0", "NW", "KEEP0", "OUT0", "NC")] == [eh.SLOT, eh.POS0, eh.NW, eh.KEEP0, eh.OUT0, eh.NC] \
        == [em.SLOT, em.POS0, em.NW, em.KEEP0, em.OUT0, em.NC] == list(range(6))
    assert [define(n) for n in ("NOT_CAPTURED", "LEFT_RING", "NO_ROOM")] == [eh.NOT_CAPTURED, eh.LEFT_RING, eh.NO_ROOM] \
        == [em.NOT_CAPTURED, em.LEFT_RING, em.NO_ROOM] == [-1, -2, -3]
    assert define("MAX_RATES") == eh.MAX_RATES == 8 and define("CHUNK") == eh.CHUNK == 256 and define("WORK_COLS") == eh.WORK_COLS
    assert (define("KIND_ONSET"), define("KIND_OFFSET")) == (eh.KIND_ONSET, eh.KIND_OFFSET) == (em.KIND_BITS["onset"], em.KIND_BITS["offset"])
    assert [len(eh.SIGNATURES["cfed_" + e]) for e in ("workspace_ints", "capture")] == [1, 23]
    assert clib.cfed_workspace_ints(5) == 5 * eh.WORK_COLS == eh.workspace_ints(5)
    assert clib.cfed_workspace_ints(0) == -1 == clib.cfed_workspace_ints(-3) == clib.cfed_workspace_ints(1 << 30)
    with pytest.raises(RuntimeError, match="no workspace for capacity=0"):
        eh.workspace_ints(0)
    for other in _abi.LIBS:                       # its prefix hides no other library's, and none hides it
        assert not other.prefix.startswith(ROW.prefix) and not ROW.prefix.startswith(other.prefix), other.name
    for prefix in ("cfcs_", "cfev_", "cfbl_", "cfsh_", "cfps_", "cfal_", "cftp_"):
        assert not prefix.startswith(ROW.prefix) and not ROW.prefix.startswith(prefix)


def test_abi_version_is_checked_at_load(clib, monkeypatch):
    check_abi_at_load(ROW, monkeypatch)


def test_the_kernels_are_the_listed_ones_and_use_no_scratch(clib):
    from clip_fsar_amd import build as b
    from clip_fsar_amd import evidence_hip as eh
    pl = b.PLUGIN_LIBS["evidence"]
    if not os.path.exists(pl.usage):
        b.build_plugin("evidence", force=True, verbose=False)
    usage = json.load(open(pl.usage))
    assert len(usage) == ROW.total == sum(KERNELS.values()), sorted(usage)
    for fragment, count in KERNELS.items():
        assert sum(fragment in n for n in usage) == count, (fragment, sorted(usage))
    for n, u in usage.items():
        assert u.get("scratch", 0) == 0 and u.get("spills", 0) == 0, (n, u)
    assert pl.lib == eh.LIB_PATH and pl.lib.endswith(os.sep + "libclipfsar_evidence.so") and os.path.exists(pl.lib)
    others = [b.USAGE] + [x.usage for reg in (b.SIDE_LIBS, b.EXT_LIBS, b.ADDON_LIBS) for x in reg.values()]
    others += [x.usage for n, x in b.PLUGIN_LIBS.items() if n != "evidence"]
    for path in others:                           # no other library's report names them, and they carry no other library's fragment
        if os.path.exists(path):
            assert not any(fragment in n for n in json.load(open(path)) for fragment in KERNELS), path
    import test_align_abi, test_baseline_abi, test_events_abi, test_pool_select_abi, test_shortlist_abi, test_tempo_abi
    claimed = [f for row in _abi.SIDE for f in row.kernels]
    claimed += [f for mod in (test_align_abi, test_baseline_abi, test_events_abi, test_pool_select_abi, test_shortlist_abi, test_tempo_abi)
                for f in mod.KERNELS]
    for n in usage:
        assert not any(f in n for f in claimed), n
    # the conventions: the ring libraries' row pieces, the shared error plumbing, the detector's record layout and its own header --
    # nothing else; plain C++, no atomics, no allocation, no copy or wait of its own
    source = open(pl.source).read()
    assert re.findall(r'^#include [<"]([^>"]+)[>"]', source, flags=re.M) == ["../csrc/ring_rows.h", "../csrc/side_lib.h",
                                                                            "../../include/ext/clipfsar_events.h",
                                                                            "../../include/ext/clipfsar_evidence.h"]
    for body in ("asm", "atomic", "malloc", "hipMalloc", "hipMemcpy", "hipDeviceSynchronize"):
        assert body not in source, body
    for shared in ("Piece<VEC>", "vec_ok(", "blocks_for(", "MAX_ITEMS", "SIDE_REQUIRE(", "check_launch(", "CFEV_ONSET", "CFEV_EVENT_COLS"):
        assert shared in source, shared
    assert "rates_dev" not in source and "Rates rates" in source     # the rates travel by value
    assert source.count("hipLaunchKernelGGL(evidence_place_kernel, dim3(1), dim3(THREADS)") == 1     # ONE workgroup places


def test_evidence_is_a_name_of_the_open_registry_and_follows_the_recipe():
    from clip_fsar_amd import build as b
    assert "evidence" in b.PLUGIN_LIBS and "evidence" in b.plugin_lib_names()
    assert all("evidence" not in reg for reg in (b.SIDE_LIBS, b.EXT_LIBS, b.ADDON_LIBS))
    pl = b.PLUGIN_LIBS["evidence"]
    assert isinstance(pl, b.ExtLib)
    assert pl.source == os.path.join(b.EXT, "evidence.hip") and os.path.exists(pl.source)
    assert pl.header == HEADER and os.path.exists(pl.header)
    assert pl.lib == os.path.join(b.HERE, "libclipfsar_evidence.so")
    assert pl.usage == os.path.join(b.HERE, "build", "evidence", "resource_usage.json")
    deps = b._plugin_deps("evidence")
    assert sorted(deps) == sorted([pl.source, pl.header, os.path.abspath(b.__file__), os.path.join(b.CSRC, "ring_rows.h"),
                                   os.path.join(b.CSRC, "side_lib.h"), os.path.join(b.CSRC, "common.h"),
                                   os.path.join(ROOT, "include", "ext", "clipfsar_events.h"),
                                   os.path.join(ROOT, "include", "clipfsar_hip.h")])
    for call in (b.build_side, b._side_deps, b.build_ext, b._ext_deps, b.build_addon, b._addon_deps):       # the three closed registries
        with pytest.raises(KeyError):
            call("evidence")
    assert not os.path.exists(os.path.join(b.CSRC, "evidence.hip"))
    assert not any("clipfsar_evidence" in open(os.path.join(b.CSRC, f)).read() for f in os.listdir(b.CSRC))  # nothing of csrc/ knows it


def test_staleness_of_the_evidence_library_and_of_no_other(monkeypatch):
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

    for edited in ("evidence.hip", "clipfsar_evidence.h"):                        # its own files: it alone
        assert stale_after(edited) == (set(), {"evidence"}), edited
    old, plugins = stale_after("clipfsar_events.h")                               # the records' layout: the detector and it
    assert "events" in old and "evidence" in plugins and "tempo" not in plugins
    old, plugins = stale_after("ring_rows.h")                                     # the row pieces: the ring libraries and it
    assert STALE["ring_rows.h"] <= old and "evidence" in plugins and "align" not in plugins
    for edited in ("side_lib.h", "build.py", "common.h"):                         # what every library reaches
        old, plugins = stale_after(edited)
        assert STALE[edited] <= old and plugins == set(b.PLUGIN_LIBS), edited
    for edited in ("pool.hip", "clipfsar_pool.h", "clipfsar_tempo.h", "tempo.hip", "events.hip", "select_keys.h", "chunk_row.h",
                   "otam_tile.h", "fp32_tile_gemm.h", "align.hip", "gemm.hip"):
        assert "evidence" not in stale_after(edited)[1], edited
    assert stale_after("no_such_file.h") == (set(), set())


# ------------------------------------------------------------------ validation, without a GPU
def _tbl(rows):
    flat = [v for r in rows for v in r]
    return (ctypes.c_int32 * len(flat))(*flat)


def _rates(*r):
    return (ctypes.c_int32 * max(1, len(r)))(*r)


#        slot pos0 nW keep0 out0 nc
GOOD = [[2, 5, 3, 0, 0, 4],
        [0, 0, 0, 0, 12, 2],
        [1, 15, 4, 2, 12, 2]]                  # cap 16, max_streams 4, T 4, stride 2, rate 2: 2 kept windows span 2 + 6 + 1 = 9 frames


def _edit(row, col, value):
    rows = [list(r) for r in GOOD]
    rows[row][col] = value
    return _tbl(rows)


def test_capture_validation_without_gpu(clib):
    base = 1 << 24
    ptrs0 = [ctypes.c_void_p(base * (i + 1)) for i in range(10)]      # far apart and never dereferenced: every call fails validation
    err, good, r12 = clib.cfed_last_error, _tbl(GOOD), _rates(1, 2)
    names = "ring events n_events tempo store head where work table_host table_dev".split()

    # capture(ring, events, n_events, tempo, store, head, where, work, table_host, table_dev, S, max_streams, cap, max_events, kinds, T, E,
    #         stride, rate, rates_host, R, capacity, stream)
    def call(table=good, S=3, ms=4, cap=16, M=7, kinds=1, T=4, E=64, stride=2, rate=2, rates=r12, R=2, capacity=3, **ptr):
        a = list(ptrs0)
        a[8] = table
        for name, v in ptr.items():
            a[names.index(name)] = v
        return clib.cfed_capture(*a, S, ms, cap, M, kinds, T, E, stride, rate, rates, R, capacity, None)

    def refused(words, **kw):
        assert call(**kw) != 0, kw
        msg = err()
        assert msg.startswith(b"cfed_capture: ") and words in msg, (kw, msg)

    for name in names:
        if name != "tempo":
            refused(b"null pointer", **{name: None})
    refused(b"tempo is NULL with R=2", tempo=None)                    # the plane goes with the rates ...
    refused(b"tempo is given with R=0", R=0)                          # ... and NULL with R = 0
    refused(b"null pointer (rates_host with R=2)", rates=None)
    for R in (-1, 9):
        refused(b"R=%d rates outside 0 .. 8" % R, R=R, rates=_rates(*range(1, 10)))
    for ms in (0, 1 << 20):
        refused(b"max_streams=%d outside 1 .. 65536" % ms, ms=ms)
    for S in (0, 5):
        refused(b"S=%d rows for max_streams=4" % S, S=S)
    for kw in ({"T": 0}, {"E": 0}, {"cap": 0}, {"T": -1}):
        refused(b"bad shape", **kw)
    refused(b"stride=0 must be at least 1", stride=0)
    refused(b"rate=0 must be at least 1", rate=0, R=0, tempo=None)
    for capacity in (0, -2):
        refused(b"capacity=%d must be at least 1" % capacity, capacity=capacity)
    refused(b"max_events=0 must be at least 1", M=0)
    for kinds in (0, 4, -1):
        refused(b"kinds=%d outside 1 .. 3" % kinds, kinds=kinds)
    refused(b"capacity=1048576 x T=4 x E=512 floats is 2^31 or more", capacity=1 << 20, E=512)
    refused(b"max_streams=65536 x cap=32768 rows is 2^31 or more", ms=65536, cap=32768)
    # the rates: at least 1, strictly ascending, the last one the pool's rate
    for first in (0, -2):
        refused(b"rates[0]=%d must be at least 1" % first, rates=_rates(first, 2))
    for bad in ((2, 2), (3, 2), (1, 1, 2)):
        refused(b"strictly ascending", rates=_rates(*bad), R=len(bad))
    refused(b"rate=2 is not rates[1]=3", rates=_rates(1, 3))
    refused(b"rate=5 is not rates[1]=2", rate=5, cap=64)
    # the table, row by row
    for slot in (-1, 4):
        refused(b"row 1 has slot %d outside 0 .. 3" % slot, table=_edit(1, 0, slot))
    for pos in (-1, 16):
        refused(b"row 0 has ring position pos0=%d outside 0 .. cap-1" % pos, table=_edit(0, 1, pos))
    refused(b"row 1 has a negative count (nW=-1)", table=_edit(1, 2, -1))
    for keep in (-1, 5):
        refused(b"row 2 has keep0=%d outside 0 .. nW=4" % keep, table=_edit(2, 3, keep))
    refused(b"row 0 has nc=0 columns", table=_edit(0, 5, 0))
    refused(b"row 2 has a negative cell offset (out0=-4)", table=_edit(2, 4, -4))
    # the windows that can be captured lie in the ring together: 3 windows at stride 2 of T = 4 frames at rate 2 span 4 + 6 + 1 = 11
    # frames and fit cap = 16; 4 do at keep0 = 2 (9 frames) and not at keep0 = 0 (13 frames fit, at stride 4 they are 19)
    refused(b"row 2: the 19 frames of its windows keep0=0 .. nW=4 do not fit a ring of cap=16", table=_edit(2, 3, 0), stride=4)
    refused(b"row 0: the 20 frames", rate=5, rates=_rates(1, 5))      # 2 * 2 + 3 * 5 + 1
    assert call(table=_edit(2, 3, 4), stride=1 << 20) != 0 and b"row 0" in err()       # keep0 = nW: the row has no window to check
    # a store inside the ring, at its start, over its end, and the ring inside the store
    ring_bytes, store_bytes = 4 * 16 * 64 * 4, 3 * 4 * 64 * 4
    ring = ptrs0[0].value
    for at in (0, 4, ring_bytes - 4, -store_bytes + 4):
        refused(b"store overlaps ring", store=ctypes.c_void_p(ring + at))
    refused(b"of its own", store=ctypes.c_void_p(ring + 64))


def test_python_wrapper_rejects_cpu_tensors_and_bad_shapes(clib):
    from clip_fsar_amd import evidence_hip as eh
    host = torch.tensor(GOOD, dtype=torch.int32)
    table = eh.Table(host, host, 3)               # a device copy that is no device tensor
    i32 = dict(dtype=torch.int32)
    ring, store = torch.zeros(4, 16, 8), torch.zeros(3, 4, 8)
    ev, n, head, where, work = torch.zeros(7, 5, **i32), torch.zeros(1, **i32), torch.zeros(1, **i32), torch.zeros(7, 2, **i32), torch.zeros(9, **i32)
    with pytest.raises(RuntimeError, match="HIP device tensor"):
        eh.capture(ring, ev, n, None, store, head, where, work, table, 1, 2, 2)
    with pytest.raises(RuntimeError, match=r"store has shape .* expected \[capacity, T, 8\]"):
        eh.capture(ring, ev, n, None, torch.zeros(3, 4, 4), head, where, work, table, 1, 2, 2)
    with pytest.raises(RuntimeError, match="events has shape"):
        eh.capture(ring, torch.zeros(7, 4, **i32), n, None, store, head, where, work, table, 1, 2, 2)
    with pytest.raises(RuntimeError, match="where has shape"):
        eh.capture(ring, ev, n, None, store, head, torch.zeros(6, 2, **i32), work, table, 1, 2, 2)
    with pytest.raises(RuntimeError, match="head has shape"):
        eh.capture(ring, ev, n, None, store, torch.zeros(2, **i32), where, work, table, 1, 2, 2)
    with pytest.raises(RuntimeError, match="a store of 3 slots needs 9 ints"):
        eh.capture(ring, ev, n, None, store, head, where, work[:8], table, 1, 2, 2)
    with pytest.raises(RuntimeError, match="tempo and rates go together"):
        eh.capture(ring, ev, n, None, store, head, where, work, table, 1, 2, 2, rates=(1, 2))
    with pytest.raises(RuntimeError, match="Table"):
        eh.capture(ring, ev, n, None, store, head, where, work, eh.Table(host[:, :5], host, 3), 1, 2, 2)


# ------------------------------------------------------------------ reference_capture on hand-written cases
def _ring(M=3, cap=11, E=2):
    """ring[m, p] = (100 m + p, -(100 m + p)): a row names its slot and position"""
    v = (100 * torch.arange(M).view(M, 1) + torch.arange(cap).view(1, cap)).float()
    return torch.stack([v, -v], -1)


def _rows(store):
    return [[int(v) for v in slot[:, 0].tolist()] for slot in store]


ONSET, OFFSET = 1, 2


def test_reference_capture_hand_cases():
    from clip_fsar_amd.evidence import reference_capture
    ring = _ring()
    T, stride, rate = 3, 2, 2
    #          slot pos0 nW keep0 out0 nc
    table = [[1, 9, 3, 0, 0, 2],
             [2, 4, 4, 2, 6, 1]]
    fresh = lambda capacity: torch.full((capacity, T, 2), -7.0)
    # both kinds in the records, onsets captured: the offset is "kind"; k < keep0 is "ring"; positions wrap mod cap = 11
    events = [[0, 1, 0, ONSET, 2], [0, 0, 2, OFFSET, 5], [1, 0, 1, ONSET, 2], [1, 0, 3, ONSET, 2], [0, 0, 1, ONSET, 2], [9, 9, 9, 9, 9]]
    where, head, store = reference_capture(ring, events, 5, None, table, 2, fresh(4), 1, T, stride, rate)
    assert where.dtype == torch.int32 and where.tolist() == [[2, 0], [-1, 0], [-2, 0], [3, 0], [0, 0], [-1, 0]] and head == 1
    assert _rows(store) == [[100, 102, 104], [-7] * 3, [109, 100, 102], [210, 201, 203]]      # slot 1 keeps its bytes
    assert torch.equal(store[2, :, 1], -store[2, :, 0])
    # both kinds captured: the offset takes a slot in record order; kinds = 2: the offset alone
    where, head, store = reference_capture(ring, events, 5, None, table, 2, fresh(4), 3, T, stride, rate)
    assert where.tolist() == [[2, 0], [3, 0], [-2, 0], [0, 0], [1, 0], [-1, 0]] and head == 2
    assert _rows(store)[3] == [102, 104, 106]
    where, head, store = reference_capture(ring, events, 5, None, table, 0, fresh(4), 2, T, stride, rate)
    assert where.tolist() == [[-1, 0], [0, 0], [-1, 0], [-1, 0], [-1, 0], [-1, 0]] and head == 1
    # more qualifiers than capacity: the first `capacity` in record order, the head advances by capacity alone (here: a full turn)
    where, head, store = reference_capture(ring, events, 5, None, table, 1, fresh(2), 1, T, stride, rate)
    assert where.tolist() == [[1, 0], [-1, 0], [-2, 0], [0, 0], [-3, 0], [-1, 0]] and head == 1
    assert _rows(store) == [[210, 201, 203], [109, 100, 102]]
    # n below and above the records; malformed records (row, k, j out of range, an unknown kind) take no rank
    where, head, _ = reference_capture(ring, events, 1, None, table, 3, fresh(4), 1, T, stride, rate)
    assert where[:, 0].tolist() == [3, -1, -1, -1, -1, -1] and head == 0
    bad = [[2, 0, 0, ONSET, 1], [-1, 0, 0, ONSET, 1], [0, 0, 3, ONSET, 1], [0, 0, -1, ONSET, 1], [0, 2, 0, ONSET, 1], [0, -1, 0, ONSET, 1],
           [0, 0, 0, 3, 1], [0, 0, 0, ONSET, 1]]
    where, head, _ = reference_capture(ring, bad, 99, None, table, 0, fresh(4), 3, T, stride, rate)
    assert where.tolist() == [[-1, 0]] * 7 + [[0, 0]] and head == 1
    # the input store is left alone
    mine = fresh(4)
    reference_capture(ring, events, 5, None, table, 0, mine, 1, T, stride, rate)
    assert bool((mine == -7).all())
    with pytest.raises(ValueError, match="tempo and rates go together"):
        reference_capture(ring, events, 5, [0] * 10, table, 0, mine, 1, T, stride, rate)


@pytest.mark.parametrize("T", [1, 3, 4])
def test_reference_capture_tempo_shift_against_brute_force_frames(T):
    """The ring as a list of frame numbers: frame f lies at f mod cap.  Window w of a session is completed by frame
    e = w * stride + (T - 1) * rmax, and its tempo i holds the frames e - (T - 1 - j) * rates[i]."""
    from clip_fsar_amd.evidence import keep0, reference_capture
    from clip_fsar_amd.stream import window_plan
    rates, stride, max_push = (1, 2, 3), 2, 6
    rmax = rates[-1]
    cap = (T - 1) * rmax + max_push
    checked = 0
    for t0, n in ((cap + 1, max_push), (3 * cap + 2, 3), (2 * cap, 2 * max_push)):     # the last: two rounds, early windows overwritten
        t = t0 + n
        frames = torch.full((1, cap, 1), -1.0)
        for f in range(t):
            frames[0, f % cap, 0] = f
        first, nW = window_plan(t0, n, T, stride, rmax)
        assert nW >= 1
        k0 = keep0(first, nW, stride, t, cap)
        assert (k0 > 0) == (n > max_push)
        NC = 3
        tempo = [(5 * k + j) % 4 - (k == 1) for k in range(nW) for j in range(NC)]     # 0 .. 3 and a -1: out of range reads as R - 1
        events = [[0, (k + 1) % NC, k, ONSET, 1] for k in range(nW)]
        where, head, store = reference_capture(frames, events, nW, tempo, [[0, (first * stride) % cap, nW, k0, 0, NC]], 0,
                                               torch.zeros(nW, T, 1), 1, T, stride, rmax, rates)
        assert head == (nW - k0) % nW
        for k in range(nW):
            if k < k0:
                assert where[k].tolist() == [-2, 0]
                continue
            raw = tempo[k * NC + (k + 1) % NC]
            i = raw if 0 <= raw < 3 else 2
            assert where[k].tolist() == [k - k0, i]
            e = (first + k) * stride + (T - 1) * rmax
            assert store[k - k0, :, 0].tolist() == [float(e - (T - 1 - j) * rates[i]) for j in range(T)], (t0, k, i)
            checked += 1
    assert checked >= 6


# ------------------------------------------------------------------ the option
def test_evidence_refusals():
    from clip_fsar_amd.evidence import Evidence, EvidenceEvent
    from clip_fsar_amd.events import Event
    ev = Evidence()
    assert ev == (256, ("onset",)) and ev.mask == 1
    assert Evidence(1, ["offset", "onset"]).kinds == ("onset", "offset") and Evidence(1, ("offset", "onset")).mask == 3
    assert Evidence(1 << 20, ("offset",)).mask == 2
    for bad in (0, -1, (1 << 20) + 1, 2.0, True, "4", None):
        with pytest.raises(ValueError, match=r"Evidence: capacity must be an integer in \[1, 2\^20\]"):
            Evidence(bad)
    for bad in ("onset", b"onset", None, {"onset"}):
        with pytest.raises(TypeError, match="Evidence: kinds must be a tuple"):
            Evidence(4, bad)
    for bad in ((), ("onset", "onset"), ("peak",), ("onset", 1)):
        with pytest.raises(ValueError, match="Evidence: kinds must be a non-empty subset"):
            Evidence(4, bad)
    assert EvidenceEvent._fields == Event._fields + ("evidence", "missed", "tempo") and len(Event._fields) == 8


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


def test_stream_pool_evidence_refusals_on_stub_heads():
    from clip_fsar_amd.baseline import Baseline
    from clip_fsar_amd.events import Event, EventRule
    from clip_fsar_amd.evidence import Evidence, EvidenceEvent
    from clip_fsar_amd.pool import StreamPool
    from clip_fsar_amd.shortlist import Shortlist
    g = _live()
    rule, ev = EventRule(0.6, 0.4, 2, 2), Evidence(capacity=4)
    with pytest.raises(ValueError, match=r"evidence= is given without events= .* build the pool with events=EventRule\(\.\.\.\) as well"):
        StreamPool(g, evidence=ev)
    for bad in (4, (4, ("onset",)), "onset"):
        with pytest.raises(TypeError, match="StreamPool: evidence must be an Evidence"):
            StreamPool(g, events=rule, evidence=bad)
    with pytest.raises(TypeError):
        StreamPool(g, 3, 1, 1, 5, 0.0, None, "column", rule, None, ev)              # keyword-only
    # it combines with everything events= combines with
    p = StreamPool(g, max_streams=3, smooth=0.5, smooth_by="class", events=rule, baseline=Baseline(), evidence=ev, rates=(1, 2))
    assert p.stats() == {"frames": 0, "tower_frames": 0, "windows": 0, "events": 0, "events_dropped": 0, "evidence": 0,
                         "evidence_missed": 0, "open": 0}
    assert p._ed_store is None and p.take_events() == []              # nothing is allocated before the first push that detects
    assert StreamPool(g, events=rule, evidence=ev, shortlist=Shortlist(g, keep=2)).stats()["evidence"] == 0
    assert StreamPool(g, events=rule, evidence=ev).open(classes=[0, 1]) == 0
    plain = StreamPool(g, events=rule)                                # without the option: the pool as it was
    assert "evidence" not in plain.stats() and not hasattr(plain, "_ed_store")
    # the event methods
    q = StreamPool(g, events=rule, evidence=ev)
    mine = lambda pool, **kw: pool._event_type(**dict(dict(session=0, class_id=1, kind="onset", window=5, start=4, length=2, score=0.7,
                                                           peak=0.8, evidence=0, missed=None, tempo=None), **kw))
    e = mine(p)
    assert isinstance(e, EvidenceEvent) and type(e).__name__ == "EvidenceEvent" and e[:8] == Event(0, 1, "onset", 5, 4, 2, 0.7, 0.8)
    calls = [("held", lambda pool, e: pool.held(e)), ("evidence_features", lambda pool, e: pool.evidence_features(e)),
             ("explain_event", lambda pool, e: pool.explain_event(e)), ("enroll_event", lambda pool, e: pool.enroll_event(e, 7))]
    for name, call in calls:
        with pytest.raises(ValueError, match=r"StreamPool.%s: this pool keeps no evidence \(build it with events=.*evidence=Evidence" % name):
            call(plain, e)
        for foreign, words in ((mine(q), "got EvidenceEvent of another pool"), (tuple(e), "got tuple"), (Event(*e[:8]), "got Event"),
                               (EvidenceEvent(*e), "got EvidenceEvent of another pool"), (None, "got NoneType")):
            with pytest.raises(TypeError, match="StreamPool.%s: takes an EvidenceEvent that this pool's take_events\\(\\) returned, %s"
                               % (name, words)):
                call(p, foreign)
    why = {"ring": "its window had left the ring", "capacity": "the push that detected it captured more than capacity = 4 windows",
           "kind": "evidence is kept for onset events, this one is an offset"}
    for name, call in calls[1:]:
        for missed, words in why.items():
            with pytest.raises(ValueError, match="StreamPool.%s: the event has no evidence \\(missed = '%s'\\): %s" % (name, missed, words)):
                call(p, mine(p, evidence=None, missed=missed, kind="offset" if missed == "kind" else "onset"))
        # held: serial s while captured_total - s <= capacity
        p._ed_captured = 9
        for s in (0, 4):
            with pytest.raises(ValueError, match="StreamPool.%s: evidence %d is no longer held -- %d windows were captured since, the store "
                               "keeps the newest capacity = 4" % (name, s, 8 - s)):
                call(p, mine(p, evidence=s))
        with pytest.raises(ValueError, match=r"evidence 9 is not a serial this pool has handed out \(9 so far\)"):
            call(p, mine(p, evidence=9))
        p._ed_captured = 0
    p._ed_captured = 9
    assert [p.held(mine(p, evidence=s)) for s in (0, 4, 5, 8, 9)] == [False, False, True, True, False]
    assert p.held(mine(p, evidence=None, missed="ring")) is False
    with pytest.raises(TypeError):
        p.held(Event(*e[:8]))
    # a held event gets as far as the store, which no push has made: nothing of the gallery or a session was touched on the way
    p._ed_store = torch.zeros(4, 4, 8)
    assert tuple(p.evidence_features(mine(p, evidence=6)).shape) == (4, 8)
    with pytest.raises(RuntimeError, match="HIP device tensor"):
        p.explain_event(mine(p, evidence=6))
    with pytest.raises(RuntimeError, match="HIP device tensor"):
        p.enroll_event(mine(p, evidence=6), 1)
    assert g._store is None and g.class_ids == [0, 1, 2]
