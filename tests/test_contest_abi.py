"""CPU: the contest (libclipfsar_contest.so, include/ext/clipfsar_contest.h, clip_fsar_amd.contest_hip, clip_fsar_amd.contest,
StreamPool(contest=...)) -- the plug-in library's exports, ABI check at load, resource report and place in the build (one more name of the
open registry, build.PLUGIN_LIBS); every host validation of cfct_contest without a GPU; Contest's refusals; reference_contest on
hand-written rows; every refusal of StreamPool(contest=...) and of leaders() on stub heads."""
import ctypes
import json
import os
import re
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import _abi
from _abi import check_abi_at_load, check_exports

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ext", "clipfsar_contest.h")
KERNELS = {"contest_kernel": 1}
ROW = _abi._row("contest", "contest_hip", "cfct_", "ext/clipfsar_contest.h", "version abi_version last_error workspace_words contest",
                KERNELS, 1)
INF, NAN = float("inf"), float("nan")
FMAX = float(np.finfo(np.float32).max)
NONE = 0x7FFFFFFF


@pytest.fixture(scope="module")
def clib():
    import __graft_entry__ as ge
    ge.build()                                    # builds every library (no-op when up to date)
    from clip_fsar_amd import contest_hip
    return contest_hip.lib()


# ------------------------------------------------------------------ the library and its place in the build
def test_header_exported_exactly_and_arity_matches(clib):
    check_exports(ROW)
    assert ROW.exports == {"cfct_" + e for e in ("version", "abi_version", "last_error", "workspace_words", "contest")}
    from clip_fsar_amd import class_smooth_hip as cs
    from clip_fsar_amd import contest as cm
    from clip_fsar_amd import contest_hip as ch
    from clip_fsar_amd import events_hip as eh
    text = open(HEADER).read()
    define = lambda name, prefix="CFCT": int(re.search(r"#define %s_%s \(?(-?\w+)\)?" % (prefix, name), text).group(1), 0)
    assert define("ABI_VERSION") == ch.ABI_VERSION == 1
    assert define("TABLE_COLS") == ch.TABLE_COLS == eh.TABLE_COLS == cs.TABLE_COLS == 6       # the detector's table, declared again
    cols = ("SLOT", "NW", "OUT0", "NC", "KEY0", "CHUNK0")
    events_h = open(os.path.join(ROOT, "include", "ext", "clipfsar_events.h")).read()
    assert [define(n) for n in cols] == [getattr(ch, n) for n in cols] == [getattr(eh, n) for n in cols] == list(range(6))
    assert [int(re.search(r"#define CFEV_%s (\d+)" % n, events_h).group(1)) for n in cols] == list(range(6))
    assert define("MAX_STREAMS") == ch.MAX_STREAMS == 65536
    assert define("NONE") == ch.NONE == cm.NONE == NONE
    assert [len(ch.SIGNATURES["cfct_" + e]) for e in ("workspace_words", "contest")] == [1, 16]
    assert [clib.cfct_workspace_words(n) for n in (0, 1, 4097, (1 << 31) - 1, -1, -5)] == [0, 1, 4097, (1 << 31) - 1, -1, -1]
    assert ch.workspace_words(12) == 12
    with pytest.raises(RuntimeError, match="no workspace for n_out=-1"):
        ch.workspace_words(-1)
    for other in _abi.LIBS:                       # its prefix hides no other library's, and none hides it
        assert not other.prefix.startswith(ROW.prefix) and not ROW.prefix.startswith(other.prefix), other.name
    for prefix in ("cfcs_", "cfev_", "cfbl_", "cfsh_", "cfps_", "cfal_", "cftp_", "cfed_", "cfsk_"):
        assert not prefix.startswith(ROW.prefix) and not ROW.prefix.startswith(prefix)


def test_abi_version_is_checked_at_load(clib, monkeypatch):
    check_abi_at_load(ROW, monkeypatch)


def test_the_kernels_are_the_listed_ones_and_use_no_scratch(clib):
    from clip_fsar_amd import build as b
    from clip_fsar_amd import contest_hip as ch
    pl = b.PLUGIN_LIBS["contest"]
    if not os.path.exists(pl.usage):
        b.build_plugin("contest", force=True, verbose=False)
    usage = json.load(open(pl.usage))
    assert len(usage) == ROW.total == sum(KERNELS.values()), sorted(usage)
    for fragment, count in KERNELS.items():
        assert sum(fragment in n for n in usage) == count, (fragment, sorted(usage))
    for n, u in usage.items():
        assert u.get("scratch", 0) == 0 and u.get("spills", 0) == 0, (n, u)
    assert pl.lib == ch.LIB_PATH and pl.lib.endswith(os.sep + "libclipfsar_contest.so") and os.path.exists(pl.lib)
    others = [b.USAGE] + [x.usage for reg in (b.SIDE_LIBS, b.EXT_LIBS, b.ADDON_LIBS) for x in reg.values()]
    others += [x.usage for n, x in b.PLUGIN_LIBS.items() if n != "contest"]
    for path in others:                           # no other library's report names it, and it carries no other library's fragment
        if os.path.exists(path):
            assert not any(fragment in n for n in json.load(open(path)) for fragment in KERNELS), path
    import test_align_abi, test_baseline_abi, test_events_abi, test_evidence_abi, test_pool_select_abi, test_shortlist_abi, test_still_abi
    import test_tempo_abi
    claimed = [f for row in _abi.SIDE for f in row.kernels]
    claimed += [f for mod in (test_align_abi, test_baseline_abi, test_events_abi, test_evidence_abi, test_pool_select_abi,
                              test_shortlist_abi, test_still_abi, test_tempo_abi) for f in mod.KERNELS]
    for n in usage:
        assert not any(f in n for f in claimed), n
    # the conventions: the shared error plumbing and its own header; plain C++, no assembly, no allocation, no stream, copy or wait of
    # its own, no loop that could wait on another workgroup; the one atomic is the histogram count in LDS; ONE launch
    source = open(pl.source).read()
    assert re.findall(r'^#include [<"]([^>"]+)[>"]', source, flags=re.M) == ["../csrc/side_lib.h", "../../include/ext/clipfsar_contest.h",
                                                                            "math.h"]
    for body in ("asm", "thread_local", "calloc", "malloc", "hipMalloc", "hipStreamCreate", "__builtin_amdgcn_mfma", "hipMemcpy", "hipMemset",
                 "hipDeviceSynchronize", "hipStreamSynchronize", "while"):
        assert body not in source, body
    assert len(re.findall(r"atomic\w*\(", source)) == source.count("atomicAdd(&hist[") == 1 and "__shared__ unsigned hist[" in source
    assert source.count("hipLaunchKernelGGL(") == 1 and "SIDE_REQUIRE(" in source and "check_launch(" in source
    # the select is the one of ext/select_keys.h: the same key, passes and tie rule, line for line where they do the work
    shared = open(os.path.join(b.EXT, "select_keys.h")).read()
    for line in ("const unsigned u = v == 0.0f ? 0u : __float_as_uint(v);", "return (u & 0x80000000u) ? ~u : (u | 0x80000000u);",
                 "const int shift = 24 - 8 * pass;", "if (above < left && incl >= left) {", "const bool take = gt || (eq && eq_rank < need_eq);",
                 "return before + (unsigned)__popcll(m & ((1ull << lane) - 1ull));"):
        assert line in source and line in shared, line


def test_contest_is_a_name_of_the_open_registry_and_follows_the_recipe():
    from clip_fsar_amd import build as b
    assert "contest" in b.PLUGIN_LIBS and "contest" in b.plugin_lib_names()
    assert all("contest" not in reg for reg in (b.SIDE_LIBS, b.EXT_LIBS, b.ADDON_LIBS))
    pl = b.PLUGIN_LIBS["contest"]
    assert isinstance(pl, b.ExtLib)
    assert pl.source == os.path.join(b.EXT, "contest.hip") and os.path.exists(pl.source)
    assert pl.header == HEADER and os.path.exists(pl.header)
    assert pl.lib == os.path.join(b.HERE, "libclipfsar_contest.so")
    assert pl.usage == os.path.join(b.HERE, "build", "contest", "resource_usage.json")
    deps = b._plugin_deps("contest")
    assert sorted(deps) == sorted([pl.source, pl.header, os.path.abspath(b.__file__), os.path.join(b.CSRC, "side_lib.h"),
                                   os.path.join(b.CSRC, "common.h"), os.path.join(ROOT, "include", "clipfsar_hip.h")])
    for call in (b.build_side, b._side_deps, b.build_ext, b._ext_deps, b.build_addon, b._addon_deps):       # the three closed registries
        with pytest.raises(KeyError):
            call("contest")
    assert not os.path.exists(os.path.join(b.CSRC, "contest.hip"))
    assert not any("clipfsar_contest" in open(os.path.join(b.CSRC, f)).read() for f in os.listdir(b.CSRC))   # nothing of csrc/ knows it
    # the rule is pure Python and numpy on the CPU: no binding, no library
    sem = open(os.path.join(b.HERE, "contest.py")).read()
    assert "contest_hip" not in re.sub(r'""".*?"""', "", sem, flags=re.S) and "ctypes" not in sem and ".cuda" not in sem


def test_staleness_of_the_contest_library_and_of_no_other(monkeypatch):
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

    for edited in ("contest.hip", "clipfsar_contest.h"):                          # its own files: it alone
        assert stale_after(edited) == (set(), {"contest"}), edited
    for edited in ("side_lib.h", "build.py", "common.h"):                         # what every library reaches
        old, plugins = stale_after(edited)
        assert STALE[edited] <= old and plugins == set(b.PLUGIN_LIBS), edited
    for edited in ("pool.hip", "clipfsar_pool.h", "clipfsar_events.h", "events.hip", "class_smooth.hip", "clipfsar_class_smooth.h",
                   "select_keys.h", "shortlist.hip", "pool_select.hip", "chunk_row.h", "ring_rows.h", "otam_tile.h", "baseline.hip",
                   "gemm.hip", "contest.py", "contest_hip.py"):
        assert "contest" not in stale_after(edited)[1], edited
    assert stale_after("no_such_file.h") == (set(), set())


# ------------------------------------------------------------------ validation, without a GPU
def _tbl(rows):
    flat = [v for r in rows for v in r]
    return (ctypes.c_int32 * len(flat))(*flat)


#        slot nW out0 nc key0 chunk0
GOOD = [[2, 3, 0, 4, 0, 0],
        [0, 0, 12, 2, 4, 1],
        [1, 2, 12, 5, 1, 2]]                   # NOUT 22, NKEYS 6


def _edit(row, col, value):
    rows = [list(r) for r in GOOD]
    rows[row][col] = value
    return _tbl(rows)


def test_contest_validation_without_gpu(clib):
    base = 1 << 24
    ptrs0 = [ctypes.c_void_p(base * (i + 1)) for i in range(8)]       # far apart and never dereferenced: every call fails validation
    err, good = clib.cfct_last_error, _tbl(GOOD)
    names = "scores keys out leaders n_leaders work table_host table_dev".split()

    # contest(scores, keys, out, leaders, n_leaders, work, table_host, table_dev, S, NOUT, NKEYS, cap, top, has_margin, margin, stream)
    def call(table=good, S=3, NOUT=22, NKEYS=6, cap=16, top=2, has_margin=0, margin=0.0, **ptr):
        a = list(ptrs0)
        a[6] = table
        for name, v in ptr.items():
            a[names.index(name)] = v
        return clib.cfct_contest(*a, S, NOUT, NKEYS, cap, top, has_margin, margin, None)

    def refused(words, **kw):
        assert call(**kw) != 0, kw
        msg = err()
        assert msg.startswith(b"cfct_contest: ") and words in msg, (kw, msg)

    for name in ("scores", "out", "work", "table_host", "table_dev"):
        refused(b"null pointer", **{name: None})
    refused(b"leaders and n_leaders go together, leaders alone is given", n_leaders=None)
    refused(b"leaders and n_leaders go together, n_leaders alone is given", leaders=None)
    for S in (0, -1, 65537):
        refused(b"a table of S=%d rows (1 .. 65536)" % S, S=S)
    refused(b"bad shape (NOUT=-1)", NOUT=-1)
    for top in (0, -3):
        refused(b"top=%d must be at least 1" % top, top=top)
    for NKEYS in (0, -2):
        refused(b"bad shape (NKEYS=%d with a key list)" % NKEYS, NKEYS=NKEYS)
    for cap in (0, -1):
        refused(b"cap=%d must be at least 1" % cap, cap=cap)
    for margin, words in ((-0.5, b"margin=-0.5"), (NAN, b"margin=nan"), (INF, b"margin=inf"), (-INF, b"margin=-inf")):
        refused(words + b" must be finite and at least 0", has_margin=1, margin=margin)
    # the table, row by row: OUT0, NW and NC tile NOUT; the lists lie inside the keys
    refused(b"row 1 has a negative count (nW=-1)", table=_edit(1, 1, -1))
    for NC in (0, -4):
        refused(b"row 0 has width NC=%d, at least 1 is needed" % NC, table=_edit(0, 3, NC))
    refused(b"row 1 has OUT0=11, the nW * NC of the rows before it add up to 12", table=_edit(1, 2, 11))
    refused(b"row 0 has OUT0=4", table=_edit(0, 2, 4))
    refused(b"row 1 has OUT0=12, the nW * NC of the rows before it add up to 16", table=_edit(0, 1, 4))
    refused(b"row 2 has its list at keys[2 .. 7), outside 0 .. NKEYS=6", table=_edit(2, 4, 2))
    refused(b"row 0 has its list at keys[-1 .. 3)", table=_edit(0, 4, -1))
    refused(b"row 1 has its list at keys[4 .. 6), outside 0 .. NKEYS=5", NKEYS=5)
    for NOUT in (21, 23, 0):
        refused(b"the table's nW * NC sum to 22, not to NOUT=%d" % NOUT, NOUT=NOUT)
    refused(b"the table's nW * NC sum to 26, not to NOUT=22", table=_edit(2, 3, 7), NKEYS=8)
    refused(b"the table's counts are too large for one launch (row 0)", table=_edit(0, 1, 1 << 30))
    # out inside scores, at its start, over its end, and scores inside out
    scores = ptrs0[0].value
    for at in (0, 4, 22 * 4 - 4, -22 * 4 + 4):
        refused(b"out overlaps scores", out=ctypes.c_void_p(scores + at))
    # keys == NULL: NKEYS, KEY0 and cap are ignored -- such a call gets as far as the overlap
    refused(b"out overlaps scores", keys=None, NKEYS=0, cap=0, table=_edit(2, 4, 99), out=ctypes.c_void_p(scores))
    # leaders and n_leaders both NULL, and has_margin = 0 with any margin, pass as well
    refused(b"out overlaps scores", leaders=None, n_leaders=None, margin=NAN, out=ctypes.c_void_p(scores + 8))
    # no windows at all: the table is validated, nothing is launched
    assert call(table=_tbl([[0, 0, 0, 3, 0, 0]]), S=1, NOUT=0) == 0


def test_python_wrapper_rejects_cpu_tensors_and_bad_shapes(clib):
    from clip_fsar_amd import contest_hip as ch
    host = torch.tensor(GOOD, dtype=torch.int32)
    table = ch.Table(host, host, 3)               # a device copy that is no device tensor
    i32 = dict(dtype=torch.int32)
    x, keys, work = torch.zeros(22), torch.zeros(6, **i32), torch.zeros(22, **i32)
    lead, n = torch.zeros(5, 2, **i32), torch.zeros(5, **i32)
    with pytest.raises(RuntimeError, match="HIP device tensor"):
        ch.contest(x, keys, torch.zeros(22), lead, n, work, table, 16, 2)
    with pytest.raises(RuntimeError, match="HIP device tensor"):
        ch.contest(torch.zeros(0), None, torch.zeros(0), None, None, torch.zeros(0, **i32), ch.Table(host[:1] * 0 + torch.tensor(
            [0, 0, 0, 1, 0, 0], **i32), host[:1], 1), 16, 2)
    with pytest.raises(RuntimeError, match="must be flat"):
        ch.contest(x.view(2, 11), keys, torch.zeros(22), lead, n, work, table, 16, 2)
    with pytest.raises(RuntimeError, match=r"out has shape \(21,\), expected \(22,\)"):
        ch.contest(x, keys, torch.zeros(21), lead, n, work, table, 16, 2)
    with pytest.raises(RuntimeError, match="leaders and n_leaders go together"):
        ch.contest(x, keys, torch.zeros(22), lead, None, work, table, 16, 2)
    with pytest.raises(RuntimeError, match=r"leaders has shape \(5, 2\), expected \[sum NW = 5, top = 3\]"):
        ch.contest(x, keys, torch.zeros(22), lead, n, work, table, 16, 3)
    with pytest.raises(RuntimeError, match=r"n_leaders has shape \(4,\), expected \(5,\)"):
        ch.contest(x, keys, torch.zeros(22), lead, n[:4], work, table, 16, 2)
    with pytest.raises(RuntimeError, match="work holds 21 words, a plane of 22 scores needs 22"):
        ch.contest(x, keys, torch.zeros(22), lead, n, work[:21], table, 16, 2)
    for top in (0, True, 2.0):
        with pytest.raises(RuntimeError, match="top must be an integer >= 1"):
            ch.contest(x, keys, torch.zeros(22), lead, n, work, table, 16, top)
    with pytest.raises(RuntimeError, match="Table"):
        ch.contest(x, keys, torch.zeros(22), lead, n, work, ch.Table(host[:, :5], host, 3), 16, 2)


# ------------------------------------------------------------------ the rule
def test_contest_refusals_name_the_field():
    from clip_fsar_amd.contest import Contest
    assert Contest() == (1, None) and Contest(3, 0) == (3, 0.0) and Contest(top=(1 << 31) - 1).top == (1 << 31) - 1
    assert Contest(2, 0.1).margin == float(np.float32(0.1)) and isinstance(Contest(2, 1).margin, float)      # rounded to fp32
    assert Contest(1, 1e-60).margin == 0.0 and Contest(1, FMAX).margin == FMAX
    for bad in (0, -1, 1 << 31, 2.0, True, "1", None):
        with pytest.raises(ValueError, match=r"Contest: top must be an integer in \[1, 2\^31\)"):
            Contest(bad)
    for bad in (-0.5, -1e-30, NAN, INF, -INF, 1e39, True, "0.1", (0.1,)):
        with pytest.raises(ValueError, match=r"Contest: margin must be None or a finite number >= 0 \(as fp32\)"):
            Contest(1, bad)


def _ref(row, keys, cap, top, margin):
    """one row through reference_contest -> (the output's bits as a list of floats with NaN spelled "nan", the leaders)"""
    from clip_fsar_amd.contest import reference_contest
    src = np.array([row], dtype=np.float32)
    out, leaders = reference_contest(src, keys, cap, top, margin)
    assert out.dtype == np.float32 and out.shape == src.shape
    untouched = out.view(np.uint32) == src.view(np.uint32)
    assert bool((untouched | np.isneginf(out)).all())                 # a cell keeps its bits or becomes -inf, nothing else
    return ["nan" if v != v else v for v in out[0].tolist()], leaders[0]


def test_reference_contest_hand_rows():
    from clip_fsar_amd.contest import leaders_table, reference_contest
    every = None
    # a tie at the R-th place: the lowest columns first
    assert _ref([0.5, 0.875, 0.5, 0.5, 0.125], every, 0, 2, None) == ([0.5, 0.875, -INF, -INF, -INF], [0, 1])
    assert _ref([0.5, 0.875, 0.5, 0.5, 0.125], every, 0, 3, None) == ([0.5, 0.875, 0.5, -INF, -INF], [0, 1, 2])
    assert _ref([0.5, 0.5, 0.5], every, 0, 1, None) == ([0.5, -INF, -INF], [0])
    # -0.0 against +0.0: equal, so the lower column wins, and each keeps its own bits
    out, lead = _ref([-1.0, -0.0, 0.0], every, 0, 1, None)
    assert lead == [1] and out == [-INF, 0.0, -INF] and np.signbit(np.float32(out[1]))
    out, lead = _ref([0.0, -0.0, -1.0], every, 0, 2, None)
    assert lead == [0, 1] and not np.signbit(np.float32(out[0])) and np.signbit(np.float32(out[1]))
    # all NaN, all -inf: no candidate, nothing changes, no leader
    assert _ref([NAN, NAN], every, 0, 1, None) == (["nan", "nan"], [])
    assert _ref([-INF, -INF, -INF], every, 0, 2, 0.0) == ([-INF, -INF, -INF], [])
    assert _ref([NAN, -INF, 0.25, NAN], every, 0, 1, None) == (["nan", -INF, 0.25, "nan"], [2])        # a NaN never disappears
    # best = +inf with a margin: floor = +inf, only +inf stays
    assert _ref([INF, 3.0, INF, FMAX], every, 0, 4, 1.0) == ([INF, -INF, INF, -INF], [0, 2])
    assert _ref([INF, 3.0, INF, FMAX], every, 0, 1, FMAX) == ([INF, -INF, -INF, -INF], [0])
    # margin = 0: the best score and its equals, up to top of them
    assert _ref([0.75, 0.875, 0.875, 0.875], every, 0, 4, 0.0) == ([-INF, 0.875, 0.875, 0.875], [1, 2, 3])
    assert _ref([0.75, 0.875, 0.875, 0.875], every, 0, 2, 0.0) == ([-INF, 0.875, 0.875, -INF], [1, 2])
    assert _ref([0.0, -0.0, -1e-45], every, 0, 3, 0.0) == ([0.0, -0.0, -INF], [0, 1])
    # ONE rounded fp32 subtraction: 1 - 2^-25 rounds to 1 (ties to even), so 1 - 2^-24 lies below the floor
    below = float(np.nextafter(np.float32(1), np.float32(0)))
    assert _ref([1.0, below], every, 0, 2, 2.0 ** -25) == ([1.0, -INF], [0])
    assert _ref([1.0, below], every, 0, 2, 2.0 ** -24) == ([1.0, below], [0, 1])
    # a margin that overflows floor to -inf: nobody is below it
    assert _ref([-FMAX, -1.0, FMAX / 2], every, 0, 3, FMAX) == ([-INF, -1.0, FMAX / 2], [1, 2])        # floor -FMAX / 2 is finite: -FMAX is below
    assert _ref([-FMAX, -FMAX / 2], every, 0, 2, FMAX) == ([-FMAX, -FMAX / 2], [0, 1])                # -FMAX / 2 - FMAX overflows
    # top > NC: everybody leads; with a margin, everybody within it
    assert _ref([0.125, 0.375, 0.25], every, 0, 8, None) == ([0.125, 0.375, 0.25], [0, 1, 2])
    assert _ref([0.125, 0.375, 0.25], every, 0, (1 << 31) - 1, 0.125) == ([-INF, 0.375, 0.25], [1, 2])
    # an invalid key on the row's best score: copied unchanged, no candidate, and `best` is the best CANDIDATE
    keys = [3, -1, 0, 5, 0x7FFFFFFF]
    assert _ref([0.25, 0.875, 0.5, 0.625, 0.9375], keys, 5, 1, None) == ([-INF, 0.875, 0.5, 0.625, 0.9375], [2])     # key 5 = cap: invalid as well
    assert _ref([0.25, 0.875, 0.5, 0.625, 0.9375], keys, 6, 2, 0.25) == ([-INF, 0.875, 0.5, 0.625, 0.9375], [2, 3])  # floor 0.375, not 0.625 or 0.6875
    assert _ref([0.25, 0.875, 0.5, 0.625, 0.9375], keys, 6, 2, 0.0625) == ([-INF, 0.875, -INF, 0.625, 0.9375], [3])
    # several rows, keys per row, and the padded form
    out, leaders = reference_contest(torch.tensor([[1.0, 2.0, 3.0], [3.0, 2.0, 1.0]]), [[0, 1, 9], [0, 1, 2]], 3, 1, None)
    assert out.tolist() == [[-INF, 2.0, 3.0], [3.0, -INF, -INF]] and leaders == [[1], [0]]
    table, counts = leaders_table([[1, 2], [], [0]], 3)
    assert table.dtype == np.int32 and table.tolist() == [[1, 2, NONE], [NONE] * 3, [0, NONE, NONE]] and counts.tolist() == [2, 0, 1]
    with pytest.raises(ValueError, match="Contest: top"):
        reference_contest([[1.0]], None, 0, 0, None)
    with pytest.raises(ValueError, match=r"scores must be \[rows, NC\]"):
        reference_contest([1.0, 2.0], None, 0, 1, None)


def test_a_demoted_pair_under_the_detector():
    """what the rule means under reference_events: outranked for min_off windows ends the event, and that OFFSET's score is -inf"""
    from clip_fsar_amd.contest import reference_contest
    from clip_fsar_amd.events import EventRule, reference_events
    rule = EventRule(0.6, 0.4, 2, 2)
    plane = np.array([[0.9, 0.8], [0.9, 0.8], [0.7, 0.8], [0.7, 0.8], [0.7, 0.3], [0.7, 0.3]], dtype=np.float32)
    out, _ = reference_contest(plane, None, 0, 1, None)
    (on0, off0, again), (on1, off1) = (reference_events(col, rule)[0] for col in out.T.tolist())
    assert (on0.k, on0.kind, off0.k, off0.kind) == (1, 1, 3, 2) and off0.score == -INF          # outranked at windows 2 and 3
    assert (again.k, again.kind) == (5, 1)                                                       # and leading again at 4 and 5
    assert (on1.k, on1.kind, off1.k, off1.kind) == (3, 1, 5, 2) and off1.score == -INF          # faded AND outranked: -inf all the same
    ungated = [len(reference_events(col, rule)[0]) for col in plane.T.tolist()]
    assert ungated == [1, 2]                      # class 0 never ends without the contest; class 1's onset came two windows earlier


# ------------------------------------------------------------------ the option
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


def test_the_contest_option_on_stub_heads():
    from clip_fsar_amd.baseline import Baseline
    from clip_fsar_amd.contest import Contest
    from clip_fsar_amd.events import EventRule
    from clip_fsar_amd.evidence import Evidence
    from clip_fsar_amd.pool import PackedOutput, StreamPool
    from clip_fsar_amd.shortlist import Shortlist
    from clip_fsar_amd.stream import StreamOutput
    g = _live()
    rule, ct = EventRule(0.6, 0.4, 2, 2), Contest(top=1)
    with pytest.raises(ValueError, match=r"contest= is given without events= .* build the pool with events=EventRule\(\.\.\.\) as well"):
        StreamPool(g, contest=ct)                 # TypeError without the feature
    for bad in (1, (1, None), "top", {"top": 1}):
        with pytest.raises(TypeError, match="StreamPool: contest must be a Contest"):
            StreamPool(g, events=rule, contest=bad)
    with pytest.raises(TypeError):
        StreamPool(g, 3, 1, 1, 5, 0.0, None, "column", rule, None, ct)              # keyword-only
    # it combines with everything events= combines with, and adds nothing to stats()
    p = StreamPool(g, max_streams=3, smooth=0.5, smooth_by="class", events=rule, baseline=Baseline(), evidence=Evidence(capacity=4),
                   rates=(1, 2), contest=Contest(2, 0.25))
    assert p.stats() == {"frames": 0, "tower_frames": 0, "windows": 0, "events": 0, "events_dropped": 0, "evidence": 0,
                         "evidence_missed": 0, "open": 0}
    assert p._ct_work is None and p._ct_tables is None and p.take_events() == []      # nothing is allocated before the first push
    assert StreamPool(g, events=rule, contest=ct, shortlist=Shortlist(g, keep=2)).stats()["events"] == 0
    assert StreamPool(g, events=rule, contest=ct).open(classes=[0, 1]) == 0
    from clip_fsar_amd.live_text_gallery import LiveTextGallery
    text = LiveTextGallery(_stub_head(COMBINE=True), "cpu", capacity=4)       # the text galleries: a rank over probabilities is a rank
    assert StreamPool(text, events=rule, contest=ct)._contest_rule == ct
    plain = StreamPool(g, events=rule)                                # without the option: the pool as it was
    assert plain._contest_rule is None and not hasattr(plain, "_ct_work") and plain.stats() == StreamPool(g, events=rule, contest=ct).stats()
    # leaders(): a pool without a contest refuses before it looks at the output
    for pool in (plain, StreamPool(g)):
        with pytest.raises(ValueError, match=r"StreamPool.leaders: this pool holds no contest \(build it with events=.*contest=Contest"):
            pool.leaders(None)
    # an output without windows: empty answers of the right shape, nothing launched, nothing allocated
    q = StreamPool(g, events=rule, contest=Contest(3))
    for out in (StreamOutput(0, torch.zeros(0, 3), None), PackedOutput([0, 1], [0, 0], [0, 0, 0], torch.zeros(0, 3), None)):
        columns, counts = q.leaders(out)
        assert tuple(columns.shape) == (0, 3) and tuple(counts.shape) == (0,) and columns.dtype == counts.dtype == torch.int32
    assert q._ct_work is None and q._ct_tables is None
    # an output with windows gets as far as the binding, which has no CPU path
    with pytest.raises(RuntimeError, match="HIP device tensor"):
        q.leaders(StreamOutput(0, torch.zeros(2, 3), None))
