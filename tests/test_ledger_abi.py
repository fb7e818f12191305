"""CPU: the shot ledger (libclipfsar_ledger.so, include/ext/clipfsar_ledger.h, clip_fsar_amd.ledger_hip, clip_fsar_amd.ledger,
LiveGallery(ledger=...)) -- the plug-in library's exports, ABI check at load, resource report and place in the build (one more name of
the open registry, build.PLUGIN_LIBS); every host validation of cfld_put, cfld_resum and cfld_fit without a GPU; the host planners on
hand-written cases; reference_fit on hand rows; ShotLedger's and LiveGallery(ledger=...)'s refusals on stub heads."""
import ctypes
import json
import math
import os
import re

import numpy as np
import pytest
import torch

import _abi
from _abi import check_abi_at_load, check_exports
from test_contest_abi import _stub_head

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ext", "clipfsar_ledger.h")
KERNELS = {"ledger_put_kernel": 1, "ledger_resum_kernel": 1, "ledger_fit_kernel": 1}
ROW = _abi._row("ledger", "ledger_hip", "cfld_", "ext/clipfsar_ledger.h", "version abi_version last_error put resum fit", KERNELS, 3)


@pytest.fixture(scope="module")
def clib():
    import __graft_entry__ as ge
    ge.build()                                    # builds every library (no-op when up to date)
    from clip_fsar_amd import ledger_hip
    return ledger_hip.lib()


# ------------------------------------------------------------------ the library and its place in the build
def test_header_exported_exactly_and_arity_matches(clib):
    check_exports(ROW)
    assert ROW.exports == {"cfld_" + e for e in ("version", "abi_version", "last_error", "put", "resum", "fit")}
    from clip_fsar_amd import ledger_hip as lh
    from clip_fsar_amd import live_hip
    text = open(HEADER).read()
    define = lambda name: int(re.search(r"#define CFLD_%s \(?(-?\w+)\)?" % name, text).group(1), 0)
    assert define("ABI_VERSION") == lh.ABI_VERSION == 1
    assert define("TABLE_COLS") == lh.TABLE_COLS == 3
    assert [define(n) for n in ("SLOT", "FIRST", "N")] == [lh.SLOT, lh.FIRST, lh.N] == [0, 1, 2]
    assert define("MAX_ROWS") == lh.MAX_ROWS == live_hip.MAX_ROWS == 65536
    assert define("MAX_T") == lh.MAX_T == live_hip.MAX_T == 32
    assert [len(lh.SIGNATURES["cfld_" + e]) for e in ("put", "resum", "fit")] == [9, 15, 15]
    for other in _abi.LIBS:                       # its prefix hides no other library's, and none hides it
        assert not other.prefix.startswith(ROW.prefix) and not ROW.prefix.startswith(other.prefix), other.name
    for prefix in ("cfcs_", "cfev_", "cfbl_", "cfsh_", "cfps_", "cfal_", "cftp_", "cfed_", "cfsk_", "cfct_", "cfhs_"):
        assert not prefix.startswith(ROW.prefix) and not ROW.prefix.startswith(prefix)


def test_abi_version_is_checked_at_load(clib, monkeypatch):
    check_abi_at_load(ROW, monkeypatch)


def test_the_kernels_are_the_listed_ones_and_use_no_scratch(clib):
    from clip_fsar_amd import build as b
    from clip_fsar_amd import ledger_hip as lh
    pl = b.PLUGIN_LIBS["ledger"]
    if not os.path.exists(pl.usage):
        b.build_plugin("ledger", force=True, verbose=False)
    usage = json.load(open(pl.usage))
    assert len(usage) == ROW.total == sum(KERNELS.values()) == 3, sorted(usage)
    for fragment, count in KERNELS.items():
        assert sum(fragment in n for n in usage) == count, (fragment, sorted(usage))
    for n, u in usage.items():
        assert u.get("scratch", 0) == 0 and u.get("spills", 0) == 0, (n, u)
    assert pl.lib == lh.LIB_PATH and pl.lib.endswith(os.sep + "libclipfsar_ledger.so") and os.path.exists(pl.lib)
    others = [b.USAGE] + [x.usage for reg in (b.SIDE_LIBS, b.EXT_LIBS, b.ADDON_LIBS) for x in reg.values()]
    others += [x.usage for n, x in b.PLUGIN_LIBS.items() if n != "ledger"]
    for path in others:                           # no other library's report names them, and they carry no other library's fragment
        if os.path.exists(path):
            assert not any(fragment in n for n in json.load(open(path)) for fragment in KERNELS), path
    import test_align_abi, test_baseline_abi, test_contest_abi, test_events_abi, test_evidence_abi, test_history_abi, test_pool_select_abi
    import test_shortlist_abi, test_still_abi, test_tempo_abi
    claimed = [f for row in _abi.SIDE for f in row.kernels]
    claimed += [f for mod in (test_align_abi, test_baseline_abi, test_contest_abi, test_events_abi, test_evidence_abi, test_history_abi,
                              test_pool_select_abi, test_shortlist_abi, test_still_abi, test_tempo_abi) for f in mod.KERNELS]
    claimed += ["event_", "evidence_", "still_", "tempo_", "history_"]
    for n in usage:
        assert not any(f in n for f in claimed), n


def test_the_source_follows_the_conventions():
    from clip_fsar_amd import build as b
    source = open(b.PLUGIN_LIBS["ledger"].source).read()
    assert re.findall(r'^#include [<"]([^>"]+)[>"]', source, flags=re.M) == ["../csrc/side_lib.h", "../../include/ext/clipfsar_ledger.h",
                                                                            "math.h"]
    # plain C++: no assembly, no allocation, no stream, copy or wait of its own, no atomics, no loop that could wait on another
    # workgroup; wave64 throughout; one launch per entry point
    for body in ("asm", "thread_local", "calloc", "malloc", "hipMalloc", "hipStreamCreate", "__builtin_amdgcn_mfma", "hipMemcpy", "hipMemset",
                 "hipDeviceSynchronize", "hipStreamSynchronize", "while", "warpSize", "atomic"):
        assert body not in source, body
    assert source.count("hipLaunchKernelGGL(") == 3 and source.count("check_launch(") == 3 and source.count("__global__") == 3
    assert "SIDE_REQUIRE(" in source and "constexpr int WAVE = 64;" in source
    # resum keeps accumulate_kernel's operation order: a sequential sum from 0, then one multiplication by 1 / n
    live = open(os.path.join(b.CSRC, "live.hip")).read()
    assert "for (int v = lo; v < hi; ++v) a += X[" in live and "o[e] = a * inv;" in live and "sm[e] = a;" in live
    assert "float a = 0.f;" in source and "for (int i = lo; i < hi; ++i) a += store[" in source
    assert "sm[e] = a;" in source and "o[e] = a * inv;" in source and "const float inv = 1.0f / (float)(hi - lo);" in source
    assert "means_by_slot ? slot : s" in source and "means_by_slot ? slot : s" in live
    # fit: slot_norms_kernel's chain and reduction; the row sum by one thread
    assert source.count("wave_sum(") == 3 and "fmaf(" in source and "wave_sum(ss)" in live
    assert "fit[p] = n == 1 ? __builtin_nanf(\"\")" in source


def test_ledger_is_a_name_of_the_open_registry_and_follows_the_recipe():
    from clip_fsar_amd import build as b
    assert "ledger" in b.PLUGIN_LIBS and "ledger" in b.plugin_lib_names()
    assert all("ledger" not in reg for reg in (b.SIDE_LIBS, b.EXT_LIBS, b.ADDON_LIBS))
    pl = b.PLUGIN_LIBS["ledger"]
    assert isinstance(pl, b.ExtLib)
    assert pl.source == os.path.join(b.EXT, "ledger.hip") and os.path.exists(pl.source)
    assert pl.header == HEADER and os.path.exists(pl.header)
    assert pl.lib == os.path.join(b.HERE, "libclipfsar_ledger.so")
    assert pl.usage == os.path.join(b.HERE, "build", "ledger", "resource_usage.json")
    deps = b._plugin_deps("ledger")
    assert sorted(deps) == sorted([pl.source, pl.header, os.path.abspath(b.__file__), os.path.join(b.CSRC, "side_lib.h"),
                                   os.path.join(b.CSRC, "common.h"), os.path.join(ROOT, "include", "clipfsar_hip.h")])
    for call in (b.build_side, b._side_deps, b.build_ext, b._ext_deps, b.build_addon, b._addon_deps):       # the three closed registries
        with pytest.raises(KeyError):
            call("ledger")
    assert not os.path.exists(os.path.join(b.CSRC, "ledger.hip"))
    assert not any("clipfsar_ledger" in open(os.path.join(b.CSRC, f)).read() for f in os.listdir(b.CSRC))    # nothing of csrc/ knows it
    # the host half is pure Python and numpy on the CPU: no binding, no library, no torch
    sem = open(os.path.join(b.HERE, "ledger.py")).read()
    code = re.sub(r'""".*?"""', "", sem, flags=re.S)
    assert "ledger_hip" not in code and "ctypes" not in sem and ".cuda" not in sem and "import torch" not in sem


def test_staleness_of_the_ledger_library_and_of_no_other(monkeypatch):
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

    for edited in ("ledger.hip", "clipfsar_ledger.h"):                            # its own files: it alone
        assert stale_after(edited) == (set(), {"ledger"}), edited
    for edited in ("side_lib.h", "build.py", "common.h"):                         # what every library reaches
        old, plugins = stale_after(edited)
        assert STALE[edited] <= old and plugins == set(b.PLUGIN_LIBS), edited
    for edited in ("live.hip", "clipfsar_live.h", "gallery.hip", "history.hip", "clipfsar_history.h", "select_keys.h", "chunk_row.h",
                   "ring_rows.h", "otam_tile.h", "evidence.hip", "gemm.hip", "ledger.py", "ledger_hip.py", "live_gallery.py"):
        assert "ledger" not in stale_after(edited)[1], edited
    assert stale_after("no_such_file.h") == (set(), set())


# ------------------------------------------------------------------ validation, without a GPU
def _tbl(rows):
    flat = [v for r in rows for v in r]
    return (ctypes.c_int32 * len(flat))(*flat)


#        slot first n
GOOD = [[5, 0, 3],
        [0, 3, 1],
        [2, 4, 2]]                                # n_list 6


def _edit(row, col, value):
    rows = [list(r) for r in GOOD]
    rows[row][col] = value
    return _tbl(rows)


BASE = 1 << 24                                    # far apart, 16-byte aligned and never dereferenced: every call fails validation


def test_put_validation_without_gpu(clib):
    err = clib.cfld_last_error
    names = "X store slots".split()

    # put(X, store, slots, Nv, L, E, shots, rows_kept, stream)
    def refused(words, Nv=3, L=9, E=8, shots=16, rows_kept=8, **ptr):
        a = [ctypes.c_void_p(BASE * (i + 1)) for i in range(3)]
        for name, v in ptr.items():
            a[names.index(name)] = v
        assert clib.cfld_put(*a, Nv, L, E, shots, rows_kept, None) != 0, (words, ptr)
        msg = err()
        assert msg.startswith(b"cfld_put: ") and words in msg, msg

    for name in names:
        refused(b"null pointer", **{name: None})
    for kw in (dict(Nv=0), dict(Nv=-2), dict(L=0), dict(shots=0), dict(rows_kept=0), dict(rows_kept=10), dict(rows_kept=-1)):
        refused(b"bad shape", **kw)
    for E in (0, 2, 6, -4, 250):
        refused(b"E=%d must be a multiple of 4, at least 4" % E, E=E)
    refused(b"16-byte aligned", X=ctypes.c_void_p(BASE + 4))
    refused(b"16-byte aligned", store=ctypes.c_void_p(2 * BASE + 8))
    refused(b"Nv * rows_kept = 2147483648 rows exceed 32-bit sizes", Nv=1 << 28, rows_kept=8)
    for at in (0, 16, 3 * 9 * 8 * 4 - 16, -16 * 8 * 8 * 4 + 16):                  # the store inside X, over its end, X inside it
        refused(b"store overlaps X", store=ctypes.c_void_p(BASE + at))


def test_resum_and_fit_validation_without_gpu(clib):
    err, good = clib.cfld_last_error, _tbl(GOOD)

    # resum(store, list, sums, means, table_host, table_dev, S, n_list, shots, rows_kept, L, E, cap, means_by_slot, stream)
    # fit(store, sums, list, fit, table_host, table_dev, S, n_list, shots, rows_kept, L, T, E, cap, stream)
    def call(fn, table=good, S=3, n_list=6, shots=16, rows_kept=8, L=9, T=8, E=8, cap=8, null=None, ptr=None):
        a = [ctypes.c_void_p(BASE * (i + 1)) for i in range(6)]
        a[4] = table
        if null is not None:
            a[null] = None
        for i, v in (ptr or {}).items():
            a[i] = v
        if fn == "resum":
            return clib.cfld_resum(*a, S, n_list, shots, rows_kept, L, E, cap, 1, None)
        return clib.cfld_fit(*a, S, n_list, shots, rows_kept, L, T, E, cap, None)

    for fn in ("resum", "fit"):
        who = b"cfld_" + fn.encode()

        def refused(words, **kw):
            assert call(fn, **kw) != 0, (fn, kw)
            msg = err()
            assert msg.startswith(who + b": ") and words in msg, (fn, kw, msg)

        for i in range(6):
            refused(b"null pointer", null=i)
        for kw in (dict(n_list=0), dict(shots=0), dict(L=0), dict(cap=0), dict(rows_kept=0), dict(rows_kept=10)):
            refused(b"bad shape", **kw)
        for S in (0, -1, 9, 65537):               # cap = 8
            refused(b"a table of %d rows (1 .. min(65536, cap = 8))" % S, S=S)
        refused(b"row 1: slot 8 outside [0, 8)", table=_edit(1, 0, 8))
        refused(b"row 0: slot -1 outside [0, 8)", table=_edit(0, 0, -1))
        refused(b"row 2: slot 5 appears twice in the table", table=_edit(2, 0, 5))
        refused(b"row 1: a class of 0 shots, at least 1 is needed", table=_edit(1, 2, 0))
        refused(b"row 0: a class of -3 shots", table=_edit(0, 2, -3))
        refused(b"row 1: FIRST = 2 is not the running sum 3 of the counts before", table=_edit(1, 1, 2))
        refused(b"row 0: FIRST = 1 is not the running sum 0", table=_edit(0, 1, 1))
        refused(b"row 2: FIRST = 4 is not the running sum 5", table=_edit(1, 2, 2))
        for n_list in (5, 7):
            refused(b"the classes' shots add up to 6, not to n_list = %d" % n_list, n_list=n_list)
    # fit alone: T and E
    who = b"cfld_fit: "
    for T in (0, -1, 9, 33):
        assert call("fit", T=T) != 0 and err().startswith(who) and b"T=%d rows outside 1 .. min(32, rows_kept = 8)" % T in err()
    for E in (0, 2, 6, 250):
        assert call("fit", E=E) != 0 and b"E=%d must be a multiple of 4, at least 4" % E in err()
    assert call("fit", ptr={0: ctypes.c_void_p(BASE + 4)}) != 0 and b"16-byte aligned" in err()
    assert call("fit", ptr={1: ctypes.c_void_p(2 * BASE + 8)}) != 0 and b"16-byte aligned" in err()
    assert call("resum", E=0) != 0 and b"bad shape" in err()


def test_python_wrapper_rejects_cpu_tensors_and_bad_shapes(clib):
    from clip_fsar_amd import ledger_hip as lh
    host = torch.tensor(GOOD, dtype=torch.int32)
    table = lh.Table(host, host, 3)               # a device copy that is no device tensor
    i32 = dict(dtype=torch.int32)
    X, store, slots = torch.zeros(3, 9, 8), torch.zeros(16, 8, 8), torch.zeros(3, **i32)
    sums, means, lst, out = torch.zeros(8, 9, 8), torch.zeros(8, 8, 8), torch.zeros(6, **i32), torch.zeros(6)
    with pytest.raises(RuntimeError, match="HIP device tensor"):
        lh.put(X, store, slots)
    with pytest.raises(RuntimeError, match="HIP device tensor"):
        lh.resum(store, lst, sums, means, table, True)
    with pytest.raises(RuntimeError, match="HIP device tensor"):
        lh.fit(store, sums, lst, out, table, 8)
    with pytest.raises(RuntimeError, match=r"X must be \[Nv, L, E\] and store \[shots, rows_kept, E\]"):
        lh.put(X.view(-1), store, slots)
    with pytest.raises(RuntimeError, match=r"store has shape \(16, 8, 8\), expected \(16, 8, 4\)"):
        lh.put(X[:, :, :4], store, slots)
    with pytest.raises(RuntimeError, match=r"slots has shape \(2,\), expected \(3,\)"):
        lh.put(X, store, slots[:2])
    with pytest.raises(RuntimeError, match=r"sums has shape \(8, 9, 4\), expected \(8, 9, 8\)"):
        lh.resum(store, lst, sums[:, :, :4], means, table, True)
    with pytest.raises(RuntimeError, match=r"means has shape \(8, 8, 8\), expected \(3, 8, 8\)"):
        lh.resum(store, lst, sums, means, table, False)
    with pytest.raises(RuntimeError, match=r"means has shape \(3, 8, 8\), expected \(8, 8, 8\)"):
        lh.resum(store, lst, sums, means[:3], table, True)
    with pytest.raises(RuntimeError, match=r"slot_list has shape \(0,\), expected a non-empty \[n\]"):
        lh.resum(store, lst[:0], sums, means, table, True)
    with pytest.raises(RuntimeError, match=r"out has shape \(5,\), expected \(6,\)"):
        lh.fit(store, sums, lst, out[:5], table, 8)
    for T in (0, 9, 33, True, 8.0):
        with pytest.raises(RuntimeError, match=r"T must be an integer in \[1, min\(32, rows_kept = 8\)\]"):
            lh.fit(store, sums, lst, out, table, T)
    with pytest.raises(RuntimeError, match="Table"):
        lh.resum(torch.zeros(16, 8, 8), lst, sums, means, lh.Table(host[:, :2], host, 3), True)


# ------------------------------------------------------------------ the option's type, the planners and the rule
def test_shot_ledger_refusals_name_the_field():
    from clip_fsar_amd.ledger import ShotLedger
    assert ShotLedger() == (4096, None, False) and ShotLedger(shots=8, per_class=2, features=True) == (8, 2, True)
    for bad in (0, -5, 2.0, True, "4096", None):
        with pytest.raises(ValueError, match="ShotLedger: shots must be an integer >= 1"):
            ShotLedger(bad)
    for bad in (0, -1, 2.0, True, "2"):
        with pytest.raises(ValueError, match="ShotLedger: per_class must be None or an integer >= 1"):
            ShotLedger(8, per_class=bad)
    for bad in (0, 1, None, "yes"):
        with pytest.raises(ValueError, match="ShotLedger: features must be True or False"):
            ShotLedger(8, features=bad)


def test_the_planners_on_hand_cases():
    from clip_fsar_amd import ledger as L
    b0 = L.new_ledger_book(6)
    # the lowest free slot first, in the call's (class-grouped) order; serials rise
    p = L.plan_put(b0, [("a", 2), ("b", 1), ("c", 2)], "add_classes")
    assert (p.serials, p.slots, p.evicted) == ([0, 1, 2, 3, 4], [0, 1, 2, 3, 4], {})
    assert p.book.lists == {"a": [0, 1], "b": [2], "c": [3, 4]} and p.book.free == [5] and p.book.next_serial == 5
    assert b0.lists == {} and b0.free == list(range(6)) and b0.next_serial == 0          # a plan changes nothing
    b1 = p.book
    # removal in the middle of a class's list, and of two classes at once; first-appearance order of the touched classes
    b2 = L.plan_put(b1, [("a", 1)], "enroll").book                                     # a: serials 0, 1, 5 in slots 0, 1, 5
    d = L.plan_drop(b2, [1])
    assert d.classes == ["a"] and d.book.lists["a"] == [0, 5] and d.book.free == [1] and 1 not in d.book.slot_of
    d = L.plan_drop(b2, [4, 0])
    assert d.classes == ["c", "a"] and d.book.lists == {"a": [1, 5], "b": [2], "c": [3]} and sorted(d.book.free) == [0, 4]
    assert b2.lists["a"] == [0, 1, 5] and b2.free == []
    # the freed slots are the next ones taken, lowest first; a serial is never reused
    p = L.plan_put(d.book, [("b", 2)], "add_shots")
    assert (p.serials, p.slots) == ([6, 7], [0, 4]) and p.book.lists["b"] == [2, 6, 7]
    assert [p.book.origin_of[s] for s in (2, 5, 6)] == ["add_classes", "enroll", "add_shots"] and p.book.class_of[7] == "b"
    # the refusals: unknown, repeated, a class's last shot (alone and together), no serial at all
    for bad, words in (([9], "9 is not the serial of a ledgered shot"), ([True], "True is not the serial"), (["0"], "'0' is not the serial"),
                       ([0, 0], r"a serial appears twice in remove_shots: \[0, 0\]"), ([2], "the last shot of class 'b' -- use remove_classes"),
                       ([3, 4], "the last shot of class 'c' -- use remove_classes"), ([], "at least one serial")):
        with pytest.raises(ValueError, match="X: .*" + words):
            L.plan_drop(b2, bad, "X")
    with pytest.raises(ValueError, match="origin is one of"):
        L.plan_put(b1, [("a", 1)], "moved")
    # a full store, without per_class: refused whole, before anything changes
    assert L.room_needed(b2, {"a": 1}) == 1 and L.room_needed(b1, {"a": 1, "z": 3}) == 4
    with pytest.raises(ValueError, match=r"X: the shot ledger is full -- the call needs 1 more addends, 0 of 6 are free"):
        L.plan_put(b2, [("a", 1)], "add_shots", None, "X")
    with pytest.raises(ValueError, match=r"needs 2 more addends, 1 of 6 are free"):
        L.plan_put(b1, [("b", 1), ("z", 1)], "add_shots")
    # per_class: the newest k stay, the oldest go, oldest first; a class at its cap counts its own eviction, so a full store takes it
    p = L.plan_put(b2, [("a", 1)], "add_shots", per_class=3)
    assert L.room_needed(b2, {"a": 1}, 3) == 0 and L.room_needed(b2, {"a": 2, "b": 1}, 3) == 1
    assert (p.serials, p.slots, p.evicted) == ([6], [0], {"a": [0]}) and p.book.lists["a"] == [1, 5, 6] and p.book.free == []
    p = L.plan_put(b2, [("a", 2)], "add_shots", per_class=3)
    assert (p.slots, p.evicted) == ([0, 1], {"a": [0, 1]}) and p.book.lists["a"] == [5, 6, 7]
    with pytest.raises(ValueError, match="the shot ledger is full -- the call needs 1 more addends, 0 of 6 are free"):
        L.plan_put(b2, [("a", 1), ("b", 1)], "add_shots", per_class=3)
    # more shots in one call than the cap: the oldest of the call itself are never stored (slot -1) but have serials
    p = L.plan_put(L.new_ledger_book(4), [("q", 5), ("r", 1)], "add_classes", per_class=2)
    assert (p.serials, p.slots, p.evicted) == ([0, 1, 2, 3, 4, 5], [-1, -1, -1, 0, 1, 2], {"q": [0, 1, 2]})
    assert p.book.lists == {"q": [3, 4], "r": [5]} and p.book.free == [3] and sorted(p.book.slot_of) == [3, 4, 5]
    p = L.plan_put(b1, [("a", 1), ("c", 1)], "enroll", per_class=2)                      # b1: slot 5 free; each frees its oldest first
    assert (p.slots, p.evicted) == ([0, 3], {"a": [0], "c": [3]}) and p.book.free == [5]
    # remove_classes frees the slots; an unledgered class keeps nothing and refuses
    b3 = L.drop_classes(b2, ["a"])
    assert sorted(b3.free) == [0, 1, 5] and "a" not in b3.lists and set(b3.slot_of) == {2, 3, 4}
    un = b1._replace(unledgered=frozenset(["u"]))
    p = L.plan_put(un, [("u", 2), ("b", 1)], "add_shots")
    assert (p.serials, p.slots) == ([5, 6, 7], [-1, -1, 5]) and "u" not in p.book.lists and L.room_needed(un, {"u": 9}) == 0
    with pytest.raises(ValueError, match=r"X: class 'u' is unledgered .* \(shot_fit\)"):
        L.ledgered(un, "u", "shot_fit", "X")
    with pytest.raises(ValueError, match="5 is not the serial of a ledgered shot"):
        L.plan_drop(p.book, [5])
    assert L.ledgered(b1, "c", "shot_fit") == [3, 4] and "u" not in L.drop_classes(un, ["u"]).unledgered
    # the descriptor table: a row per class, the shared list in class order
    assert L.resum_rows(b2, ["c", "a"], {"a": 7, "b": 1, "c": 0}) == ([(0, 0, 2), (7, 2, 3)], [3, 4, 0, 1, 5])


def test_reference_fit_hand_rows():
    from clip_fsar_amd.ledger import reference_fit
    rng = np.random.default_rng(0)
    x = rng.standard_normal((1, 3, 8))
    assert np.allclose(reference_fit(np.concatenate([x, x])), [1.0, 1.0], atol=1e-15)      # an identical pair
    assert np.isnan(reference_fit(x)).all() and reference_fit(x).shape == (1,)             # one shot: nothing to compare with
    a, b = np.zeros((1, 2, 4)), np.zeros((1, 2, 4))
    a[0, :, 0], b[0, :, 1] = 1.0, 2.0
    assert np.allclose(reference_fit(np.concatenate([a, b])), [0.0, 0.0], atol=1e-15)      # an orthogonal shot
    f = reference_fit(np.concatenate([a, a, b]))                                           # b against 2a: 0; a against a + b
    assert abs(f[2]) < 1e-15 and np.allclose(f[:2], 1 / math.sqrt(5), atol=1e-15)
    assert np.allclose(reference_fit(np.concatenate([a, -a])), [-1.0, -1.0])
    f = reference_fit(np.concatenate([a, -a, b]))                                          # the others of b cancel exactly: 0 / 0
    assert np.isnan(f[2]) and np.isfinite(f[:2]).all()
    # T: the first rows alone
    y = rng.standard_normal((4, 3, 8))
    assert np.array_equal(reference_fit(y, 2), reference_fit(y[:, :2])) and not np.array_equal(reference_fit(y, 2), reference_fit(y))
    for bad, words in ((np.zeros((3, 8)), r"addends must be \[N >= 1, rows, E\]"), (np.zeros((0, 3, 8)), "addends must be")):
        with pytest.raises(ValueError, match="reference_fit: " + words):
            reference_fit(bad)
    with pytest.raises(ValueError, match="reference_fit: T = 4 outside 1 .. 3 rows"):
        reference_fit(y, 4)


# ------------------------------------------------------------------ the option
def _ledgered(ledger, capacity=4, ids=(0, 1, 2), T=4):
    from clip_fsar_amd import live_gallery as lg
    g = lg.LiveGallery(_stub_head(T), "cpu", capacity=capacity, ledger=ledger)          # TypeError without the feature
    if ids:
        g._install(lg.plan_add(g._book, list(ids)).book)      # registered on the host alone: nothing below reaches the device
    return g


def test_the_ledger_option_on_stub_heads():
    from clip_fsar_amd import ledger as L
    from clip_fsar_amd import live_gallery as lg
    from clip_fsar_amd.ledger import ShotLedger
    from clip_fsar_amd.live_text_gallery import LiveTextGallery
    g = _ledgered(ShotLedger(shots=4))
    assert g._ledger == (4, None, False) and g._lstore is None and g._ltables is None and g.last_shots == []     # nothing is allocated yet
    for bad in (4096, (4096, None, False), "ledger", {"shots": 8}):
        with pytest.raises(TypeError, match="LiveGallery: ledger must be a ShotLedger"):
            lg.LiveGallery(_stub_head(), "cpu", ledger=bad)
    with pytest.raises(TypeError):
        lg.LiveGallery(_stub_head(), "cpu", 4, ShotLedger())                                # keyword-only
    head = _stub_head()
    head._get_engine(None).arch["embed"] = 6
    with pytest.raises(ValueError, match=r"ledger= needs E % 4 == 0 .* got E = 6"):
        lg.LiveGallery(head, "cpu", ledger=ShotLedger())
    head._get_engine(None).arch["embed"] = 8
    with pytest.raises(TypeError):
        LiveTextGallery(_stub_head(COMBINE=True), "cpu", capacity=4, ledger=ShotLedger())   # out of scope: it does not take the option
    # a gallery without the option is the gallery as it was
    plain = lg.LiveGallery(_stub_head(), "cpu", capacity=4)
    assert plain._ledger is None and plain._lbook is None and plain._lstore is None
    for call, name in ((lambda: plain.last_shots, "last_shots"), (lambda: plain.shot_list(0), "shot_list"),
                       (lambda: plain.remove_shots([0]), "remove_shots"), (lambda: plain.move_shots([0], 1), "move_shots"),
                       (lambda: plain.shot_features(0), "shot_features"), (lambda: plain.shot_fit(0), "shot_fit"),
                       (lambda: plain.shot_fits(), "shot_fit")):
        with pytest.raises(ValueError, match=r"LiveGallery.%s: this gallery keeps no shot ledger \(build it with ledger=ShotLedger" % name):
            call()
    for call, name in ((lambda: g.move_shots([0], 1), "move_shots"), (lambda: g.shot_features(0), "shot_features")):
        with pytest.raises(ValueError, match=r"LiveGallery.%s: this ledger keeps no tower rows \(build it with ShotLedger\(features=True" % name):
            call()
    # the room is checked when a call is planned, on the book the plan started from: two plans of one call count together
    g._lbook = L.plan_put(g._lbook, [(0, 1), (1, 1), (2, 1)], "add_classes").book          # three shots on the host alone; one slot free
    g._book = g._book._replace(shots={0: 1, 1: 1, 2: 1})
    assert [s.serial for c in (0, 1, 2) for s in g.shot_list(c)] == [0, 1, 2] and g.shot_list(1) == [L.Shot(1, 1, "add_classes")]
    with pytest.raises(ValueError, match=r"class 7 is not registered \(shot_list\)"):
        g.shot_list(7)
    first = g._plan_shots([0])
    assert g._lpending[0] is first.book and g._lpending[1] == 1
    with pytest.raises(ValueError, match="LiveGallery: the shot ledger is full -- the call needs 2 more addends, 1 of 4 are free"):
        g._plan_shots([1], first.book)                                                    # the same call, planned on
    assert g._plan_shots([1]).book.shots[1] == 2                                          # a call of its own: it fits
    with pytest.raises(ValueError, match="needs 2 more addends, 1 of 4 are free"):
        g._plan_shots([1, 2])
    assert g._book.shots == {0: 1, 1: 1, 2: 1} and g._lbook.free == [3]                   # planning changed nothing
    capped = _ledgered(ShotLedger(shots=3, per_class=1))
    capped._lbook = L.plan_put(capped._lbook, [(0, 1), (1, 1), (2, 1)], "add_classes").book
    capped._book = capped._book._replace(shots={0: 1, 1: 1, 2: 1})
    assert capped._plan_shots([0, 1, 2, 0]).book.shots[0] == 3                            # a full store: every class evicts its own
    # every refusal of remove_shots / move_shots / shot_fit before the device is touched (a stub head has no engine to be stale)
    for bad, words in (([5], "5 is not the serial of a ledgered shot"), ([0, 0], "a serial appears twice"),
                       ([1], "the last shot of class 1 -- use remove_classes")):
        with pytest.raises(ValueError, match="LiveGallery: .*" + words):
            g.remove_shots(bad)
    f = _ledgered(ShotLedger(shots=4, features=True))
    f._lbook = L.plan_put(f._lbook, [(0, 2), (1, 1)], "enroll").book
    f._book = f._book._replace(shots={0: 2, 1: 1, 2: 1})
    with pytest.raises(ValueError, match=r"class 'kite' is not registered"):
        f.move_shots([0], "kite")
    with pytest.raises(ValueError, match="the last shot of class 1"):
        f.move_shots([2], 0)
    with pytest.raises(ValueError, match=r"9 is not the serial of a ledgered shot \(shot_features\)"):
        f.shot_features(9)
    assert f._lbook.lists == {0: [0, 1], 1: [2]} and f._lstore is None
    for bad, words in (([7], "class 7 is not registered"), ([0, 0], "a class appears twice in shot_fit")):
        with pytest.raises(ValueError, match=words):
            g.shot_fits(bad)
    # remove_classes frees the ledger slots; clear() empties the ledger and serials go on
    g.remove_classes([1])
    assert g._lbook.free == [1, 3] and g.shot_list(0)[0].serial == 0 and 1 not in g._lbook.lists
    g.clear()
    assert g._lbook.free == [0, 1, 2, 3] and g._lbook.lists == {} and g._lbook.next_serial == 3 and g.last_shots == []
    # a state without "ledger": every class is unledgered -- it lists nothing and refuses removal and the audit
    u = _ledgered(ShotLedger(shots=4), ids=())
    u._load_ledger(None, [0, 1], [2, 1])
    u._install(lg.plan_add(u._book, [0, 1], [2, 1]).book)
    assert u._lbook.unledgered == {0, 1} and u.shot_list(0) == [] and u.shot_fits() == {}
    with pytest.raises(ValueError, match=r"class 0 is unledgered -- it was loaded from a state without a ledger.*\(shot_fit\)"):
        u.shot_fit(0)
    with pytest.raises(ValueError, match="0 is not the serial of a ledgered shot"):
        u.remove_shots([0])
    assert u._plan_shots([0, 0, 0, 0, 0]).book.shots[0] == 7                               # it takes shots as ever: they need no room


def test_a_book_planned_before_an_eviction_does_not_bring_the_old_count_back(monkeypatch):
    """StreamPool.enroll_windows plans its further shots and its new classes before either runs; the device work is left out here"""
    from clip_fsar_amd import ledger as L
    from clip_fsar_amd import live_gallery as lg
    from clip_fsar_amd.ledger import ShotLedger
    g = _ledgered(ShotLedger(shots=4, per_class=1), ids=(7,))
    g._ledger_install_put(L.plan_put(g._lbook, [(7, 1)], "add_classes"))
    g._levicted = {}
    resummed = []
    monkeypatch.setattr(g, "_resum_classes", lambda eng, classes: resummed.append(list(classes)))
    shot_plan = g._plan_shots([7], g._book)
    add_plan = lg.plan_add(shot_plan.book, ["new"], [1])
    g._ledger_room(shot_plan.book, add_plan.book, {"new": 1})
    assert add_plan.book.shots == {7: 2, "new": 1}
    # the further shot: class 7 is over its cap, the oldest goes
    g._ledger_install_put(L.plan_put(g._lbook, [(7, 1)], "enroll", 1))
    g._book = shot_plan.book
    g._ledger_evict(None)
    assert g.shots(7) == 1 and g._lbook.lists == {7: [1]} and resummed == [[7]] and g.last_shots == [1]
    # the new class: its Book still says 2
    g._ledger_install_put(L.plan_put(g._lbook, [("new", 1)], "enroll", 1))
    g._install(add_plan.book)
    g._ledger_evict(None)
    assert g._book.shots == {7: 1, "new": 1} and g._lbook.lists == {7: [1], "new": [2]} and resummed == [[7]]
    # a load that is refused leaves last_shots alone
    with pytest.raises(ValueError, match="serials, class ids and origins do not agree"):
        g._load_ledger({"serials": [1, 2], "class_ids": [7], "origins": ["enroll", "enroll"]}, [7, "new"], [1, 1])
    assert g.last_shots == [2] and g._lbook.lists == {7: [1], "new": [2]}
