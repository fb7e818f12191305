"""CPU: the history search (libclipfsar_history.so, include/ext/clipfsar_history.h, clip_fsar_amd.history_hip, clip_fsar_amd.history,
StreamPool(history=...)) -- the plug-in library's exports, ABI check at load, resource report and place in the build (one more name of
the open registry, build.PLUGIN_LIBS); the source's conventions and its select held to ext/select_keys.h line for line; every host
validation of cfhs_peaks without a GPU; History's refusals; plan_search and reference_search on hand-written sessions and rows; every
refusal of StreamPool(history=...), search(), searchable() and the *_hit methods on stub heads."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import _abi
from _abi import check_abi_at_load, check_exports
from test_contest_abi import _live, _stub_head

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ext", "clipfsar_history.h")
KERNELS = {"history_peaks_kernel": 1, "history_hits_kernel": 1}
ROW = _abi._row("history", "history_hip", "cfhs_", "ext/clipfsar_history.h", "version abi_version last_error workspace_words peaks",
                KERNELS, 2)
INF, NAN = float("inf"), float("nan")
FMAX = float(np.finfo(np.float32).max)
NONE = 0x7FFFFFFF


@pytest.fixture(scope="module")
def clib():
    import __graft_entry__ as ge
    ge.build()                                    # builds every library (no-op when up to date)
    from clip_fsar_amd import history_hip
    return history_hip.lib()


# ------------------------------------------------------------------ the library and its place in the build
def test_header_exported_exactly_and_arity_matches(clib):
    check_exports(ROW)
    assert ROW.exports == {"cfhs_" + e for e in ("version", "abi_version", "last_error", "workspace_words", "peaks")}
    from clip_fsar_amd import history as hm
    from clip_fsar_amd import history_hip as hh
    from clip_fsar_amd import pool_hip as ph
    text = open(HEADER).read()
    define = lambda name, prefix="CFHS": int(re.search(r"#define %s_%s \(?(-?\w+)\)?" % (prefix, name), text).group(1), 0)
    assert define("ABI_VERSION") == hh.ABI_VERSION == 1
    assert define("TABLE_COLS") == hh.TABLE_COLS == ph.TABLE_COLS == 8                         # the pool's table, declared again
    cols = ("SLOT", "PUT_POS", "N", "FEAT_OFF", "WIN_POS", "NW", "WIN_OFF", "HAS_STATE")
    pool_h = open(os.path.join(ROOT, "include", "clipfsar_pool.h")).read()
    assert [define(n) for n in cols] == [getattr(hh, n) for n in cols] == [getattr(ph, n) for n in cols] == list(range(8))
    assert [int(re.search(r"#define CFSP_%s (\d+)" % n, pool_h).group(1)) for n in cols] == list(range(8))
    assert define("MAX_STREAMS") == hh.MAX_STREAMS == ph.MAX_STREAMS == 65536
    assert define("MAX_CLASSES") == hh.MAX_CLASSES == hm.MAX_CLASSES == 64
    assert define("MAX_TOP") == hh.MAX_TOP == hm.MAX_TOP == 4096
    assert define("MAX_SEPARATION") == hh.MAX_SEPARATION == hm.MAX_SEPARATION == 4096
    assert define("NONE") == hh.NONE == hm.NONE == NONE
    assert [len(hh.SIGNATURES["cfhs_" + e]) for e in ("workspace_words", "peaks")] == [2, 16]
    words = clib.cfhs_workspace_words
    assert [words(*a) for a in ((0, 1), (1, 1), (4097, 3), (1 << 24, 64), (1 << 30, 1))] == [0, 1, 12291, 1 << 30, 1 << 30]
    assert [words(*a) for a in ((-1, 1), (5, 0), (5, -2), ((1 << 24) + 1, 64), ((1 << 30) + 1, 1))] == [-1] * 5
    assert hh.workspace_words(12, 3) == 36 and hh.MAX_PLANE == 1 << 30
    with pytest.raises(RuntimeError, match="no workspace for a plane of -1 windows x 3 classes"):
        hh.workspace_words(-1, 3)
    for other in _abi.LIBS:                       # its prefix hides no other library's, and none hides it
        assert not other.prefix.startswith(ROW.prefix) and not ROW.prefix.startswith(other.prefix), other.name
    for prefix in ("cfcs_", "cfev_", "cfbl_", "cfsh_", "cfps_", "cfal_", "cftp_", "cfed_", "cfsk_", "cfct_"):
        assert not prefix.startswith(ROW.prefix) and not ROW.prefix.startswith(prefix)


def test_abi_version_is_checked_at_load(clib, monkeypatch):
    check_abi_at_load(ROW, monkeypatch)


def test_the_kernels_are_the_listed_ones_and_use_no_scratch(clib):
    from clip_fsar_amd import build as b
    from clip_fsar_amd import history_hip as hh
    pl = b.PLUGIN_LIBS["history"]
    if not os.path.exists(pl.usage):
        b.build_plugin("history", force=True, verbose=False)
    usage = json.load(open(pl.usage))
    assert len(usage) == ROW.total == sum(KERNELS.values()) == 2, sorted(usage)
    for fragment, count in KERNELS.items():
        assert sum(fragment in n for n in usage) == count, (fragment, sorted(usage))
    for n, u in usage.items():
        assert u.get("scratch", 0) == 0 and u.get("spills", 0) == 0, (n, u)
    assert pl.lib == hh.LIB_PATH and pl.lib.endswith(os.sep + "libclipfsar_history.so") and os.path.exists(pl.lib)
    others = [b.USAGE] + [x.usage for reg in (b.SIDE_LIBS, b.EXT_LIBS, b.ADDON_LIBS) for x in reg.values()]
    others += [x.usage for n, x in b.PLUGIN_LIBS.items() if n != "history"]
    for path in others:                           # no other library's report names them, and they carry no other library's fragment
        if os.path.exists(path):
            assert not any(fragment in n for n in json.load(open(path)) for fragment in KERNELS), path
    import test_align_abi, test_baseline_abi, test_contest_abi, test_events_abi, test_evidence_abi, test_pool_select_abi
    import test_shortlist_abi, test_still_abi, test_tempo_abi
    claimed = [f for row in _abi.SIDE for f in row.kernels]
    claimed += [f for mod in (test_align_abi, test_baseline_abi, test_contest_abi, test_events_abi, test_evidence_abi, test_pool_select_abi,
                              test_shortlist_abi, test_still_abi, test_tempo_abi) for f in mod.KERNELS]
    claimed += ["event_", "evidence_", "still_", "tempo_"]
    for n in usage:
        assert not any(f in n for f in claimed), n


def test_the_source_follows_the_conventions_and_its_select_is_the_shared_headers():
    from clip_fsar_amd import build as b
    source = open(b.PLUGIN_LIBS["history"].source).read()
    # the shared error plumbing and its own header -- not select_keys.h, chunk_row.h or ring_rows.h, whose includers are pinned
    assert re.findall(r'^#include [<"]([^>"]+)[>"]', source, flags=re.M) == ["../csrc/side_lib.h", "../../include/ext/clipfsar_history.h",
                                                                            "math.h"]
    # plain C++, no assembly, no allocation, no stream, copy or wait of its own, no loop that could wait on another workgroup; the one
    # atomic is the histogram count in LDS; wave64 throughout; TWO launches
    for body in ("asm", "thread_local", "calloc", "malloc", "hipMalloc", "hipStreamCreate", "__builtin_amdgcn_mfma", "hipMemcpy", "hipMemset",
                 "hipDeviceSynchronize", "hipStreamSynchronize", "while", "warpSize", "__shfl_down(suffix, o, 32)"):
        assert body not in source, body
    assert len(re.findall(r"atomic\w*\(", source)) == source.count("atomicAdd(&hist[") == 1 and "__shared__ unsigned hist[" in source
    assert source.count("hipLaunchKernelGGL(") == 2 and "SIDE_REQUIRE(" in source and source.count("check_launch(") == 2
    assert source.count("__global__") == 2 and source.count("__launch_bounds__(SEL_WG)") == 2 and "SEL_WG = 256, SEL_WAVES = SEL_WG / 64" in source
    assert set(re.findall(r"__shfl\w*\([^;]*?, (\d+)\)", source)) == {"64"}
    # the select is the one of ext/select_keys.h: every line of the header's score_key, block_prefix, kth_largest_key and
    # compact_selected that does work is a line of the source, in the header's order -- but for what the header leaves to its
    # includers: the signatures (`count`, the template) and the comments
    shared = open(os.path.join(b.EXT, "select_keys.h")).read()
    start = shared.index("__device__ __forceinline__ unsigned score_key(")
    stop = shared.index("// the key of column c of a group")
    body = shared[start:stop] + shared[shared.index("__device__ __forceinline__ unsigned block_prefix("):]
    code = lambda line: re.sub(r"\s*//.*$", "", line).strip()
    ours = [code(l) for l in source.splitlines()]
    at, held = 0, 0
    for line in (code(l) for l in body.splitlines()):
        if not line or line.startswith(("template <", "__device__ __forceinline__ unsigned kth_largest_key(", "unsigned& left) {", "}  // namespace")):
            continue
        if "count(wave * 256" in line:             # the includer's `count`: here the atomic itself
            line = "if ((k & mask) == prefix) atomicAdd(&hist[wave * 256 + ((k >> shift) & 255u)], 1u);"
        assert line in ours[at:], line
        at += ours[at:].index(line) + 1
        held += 1
    assert held > 60
    for line in ("const unsigned u = v == 0.0f ? 0u : __float_as_uint(v);", "return (u & 0x80000000u) ? ~u : (u | 0x80000000u);",
                 "const int shift = 24 - 8 * pass;", "if (above < left && incl >= left) {", "const bool take = gt || (eq && eq_rank < need_eq);",
                 "const bool gt = k > thr, eq = thr && k == thr;", "return before + (unsigned)__popcll(m & ((1ull << lane) - 1ull));"):
        assert line in source and line in shared, line


def test_history_is_a_name_of_the_open_registry_and_follows_the_recipe():
    from clip_fsar_amd import build as b
    assert "history" in b.PLUGIN_LIBS and "history" in b.plugin_lib_names()
    assert all("history" not in reg for reg in (b.SIDE_LIBS, b.EXT_LIBS, b.ADDON_LIBS))
    pl = b.PLUGIN_LIBS["history"]
    assert isinstance(pl, b.ExtLib)
    assert pl.source == os.path.join(b.EXT, "history.hip") and os.path.exists(pl.source)
    assert pl.header == HEADER and os.path.exists(pl.header)
    assert pl.lib == os.path.join(b.HERE, "libclipfsar_history.so")
    assert pl.usage == os.path.join(b.HERE, "build", "history", "resource_usage.json")
    deps = b._plugin_deps("history")
    assert sorted(deps) == sorted([pl.source, pl.header, os.path.abspath(b.__file__), os.path.join(b.CSRC, "side_lib.h"),
                                   os.path.join(b.CSRC, "common.h"), os.path.join(ROOT, "include", "clipfsar_hip.h")])
    for call in (b.build_side, b._side_deps, b.build_ext, b._ext_deps, b.build_addon, b._addon_deps):       # the three closed registries
        with pytest.raises(KeyError):
            call("history")
    assert not os.path.exists(os.path.join(b.CSRC, "history.hip"))
    assert not any("clipfsar_history" in open(os.path.join(b.CSRC, f)).read() for f in os.listdir(b.CSRC))   # nothing of csrc/ knows it
    # the rule is pure Python and numpy on the CPU: no binding, no library, no torch
    sem = open(os.path.join(b.HERE, "history.py")).read()
    code = re.sub(r'""".*?"""', "", sem, flags=re.S)
    assert "history_hip" not in code and "ctypes" not in sem and ".cuda" not in sem and "import torch" not in sem


def test_staleness_of_the_history_library_and_of_no_other(monkeypatch):
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

    for edited in ("history.hip", "clipfsar_history.h"):                          # its own files: it alone
        assert stale_after(edited) == (set(), {"history"}), edited
    for edited in ("side_lib.h", "build.py", "common.h"):                         # what every library reaches
        old, plugins = stale_after(edited)
        assert STALE[edited] <= old and plugins == set(b.PLUGIN_LIBS), edited
    for edited in ("pool.hip", "clipfsar_pool.h", "enroll.hip", "clipfsar_enroll.h", "select_keys.h", "shortlist.hip", "pool_select.hip",
                   "contest.hip", "clipfsar_contest.h", "chunk_row.h", "ring_rows.h", "otam_tile.h", "tempo.hip", "gemm.hip", "history.py",
                   "history_hip.py", "pool.py"):
        assert "history" not in stale_after(edited)[1], edited
    assert stale_after("select_keys.h")[1] == {"shortlist", "pool_select"}        # the header's includers stay the two they were
    assert stale_after("no_such_file.h") == (set(), set())


# ------------------------------------------------------------------ validation, without a GPU
def _tbl(rows):
    flat = [v for r in rows for v in r]
    return (ctypes.c_int32 * len(flat))(*flat)


#        slot put n feat win_pos nW win_off has_state
GOOD = [[2, 5, 0, 0, 6, 3, 0, 0],
        [0, 3, 0, 0, 0, 0, 3, 0],
        [1, 9, 0, 0, 0, 4, 3, 0]]                 # NW 7


def _edit(row, col, value):
    rows = [list(r) for r in GOOD]
    rows[row][col] = value
    return _tbl(rows)


def test_peaks_validation_without_gpu(clib):
    base = 1 << 24
    ptrs0 = [ctypes.c_void_p(base * (i + 1)) for i in range(8)]       # far apart and never dereferenced: every call fails validation
    err, good = clib.cfhs_last_error, _tbl(GOOD)
    names = "scores work hit_rows hit_scores n_hits n_peaks table_host table_dev".split()

    # peaks(scores, work, hit_rows, hit_scores, n_hits, n_peaks, table_host, table_dev, S, NW, K, separation, has_min, min_score, top, stream)
    def call(table=good, S=3, NW=7, K=2, separation=1, has_min=0, min_score=0.0, top=4, **ptr):
        a = list(ptrs0)
        a[6] = table
        for name, v in ptr.items():
            a[names.index(name)] = v
        return clib.cfhs_peaks(*a, S, NW, K, separation, has_min, min_score, top, None)

    def refused(words, **kw):
        assert call(**kw) != 0, kw
        msg = err()
        assert msg.startswith(b"cfhs_peaks: ") and words in msg, (kw, msg)

    for name in names:
        refused(b"null pointer", **{name: None})
    for S in (0, -1, 65537):
        refused(b"a table of S=%d rows (1 .. 65536)" % S, S=S)
    refused(b"bad shape (NW=-1)", NW=-1)
    for K in (0, -1, 65):
        refused(b"K=%d classes (1 .. 64)" % K, K=K)
    for top in (0, -3, 4097):
        refused(b"top=%d outside 1 .. 4096" % top, top=top)
    for sep in (-1, 4097):
        refused(b"separation=%d outside 0 .. 4096" % sep, separation=sep)
    refused(b"min_score is NaN", has_min=1, min_score=NAN)
    refused(b"a plane of NW=%d x K=64 scores is too large for one launch" % ((1 << 24) + 1), NW=(1 << 24) + 1, K=64)
    # the table, row by row: NW and WIN_OFF tile the plane; nothing else of a row is looked at
    refused(b"row 1 has a negative count (nW=-1)", table=_edit(1, 5, -1))
    refused(b"row 1 has WIN_OFF=2, the nW of the rows before it add up to 3", table=_edit(1, 6, 2))
    refused(b"row 0 has WIN_OFF=1", table=_edit(0, 6, 1))
    refused(b"row 2 has WIN_OFF=3, the nW of the rows before it add up to 5", table=_edit(1, 5, 2))
    for NW in (6, 8, 0):
        refused(b"the table's nW sum to 7, not to NW=%d" % NW, NW=NW)
    refused(b"the table's nW sum to 9, not to NW=7", table=_edit(2, 5, 6))
    refused(b"the table's counts are too large for one launch (row 0)", table=_edit(0, 5, (1 << 30) + 1), K=1, NW=1 << 30)
    garbage = [[-7, -1, 99, 5, -3, 3, 0, 9], [70000, 1 << 30, -1, 2, 1 << 30, 4, 3, -1]]   # SLOT, PUT_POS, N, FEAT_OFF, WIN_POS, HAS_STATE: unread
    scores = ptrs0[0].value
    refused(b"work overlaps scores", table=_tbl(garbage), S=2, work=ctypes.c_void_p(scores))
    # the work buffer (7 x 2 words) inside scores, over its end, scores inside it; then over each output in turn
    for at in (0, 4, 7 * 2 * 4 - 4, -7 * 2 * 4 + 4):
        refused(b"work overlaps scores", work=ctypes.c_void_p(scores + at))
    for name, nbytes in (("hit_rows", 2 * 4 * 4), ("hit_scores", 2 * 4 * 4), ("n_hits", 2 * 4), ("n_peaks", 2 * 4)):
        out = ptrs0[names.index(name)].value
        for at in (0, nbytes - 4, -7 * 2 * 4 + 4):
            refused(b"work overlaps an output", work=ctypes.c_void_p(out + at))
    # has_min = 0 with any min_score passes as far as the overlap; so does -inf / +inf as a floor
    refused(b"work overlaps scores", min_score=NAN, work=ctypes.c_void_p(scores + 8))
    for floor in (-INF, INF, FMAX):
        refused(b"work overlaps scores", has_min=1, min_score=floor, work=ctypes.c_void_p(scores + 8))
    # no windows at all: the table is validated, nothing is launched
    assert call(table=_tbl([[0, 0, 0, 0, 0, 0, 0, 0]]), S=1, NW=0) == 0
    assert call(table=_tbl([[3, 1, 0, 0, 2, 0, 0, 0], [1, 0, 0, 0, 0, 0, 0, 0]]), S=2, NW=0, K=64, top=4096, separation=4096) == 0
    refused(b"row 0 has WIN_OFF=1", table=_tbl([[0, 0, 0, 0, 0, 0, 1, 0]]), S=1, NW=0)


def test_python_wrapper_rejects_cpu_tensors_and_bad_shapes(clib):
    from clip_fsar_amd import history_hip as hh
    host = torch.tensor(GOOD, dtype=torch.int32)
    table = hh.Table(host, host, 3)               # a device copy that is no device tensor
    i32 = dict(dtype=torch.int32)
    x, work = torch.zeros(7, 2), torch.zeros(14, **i32)
    rows, vals, n, p = torch.zeros(2, 4, **i32), torch.zeros(2, 4), torch.zeros(2, **i32), torch.zeros(2, **i32)
    with pytest.raises(RuntimeError, match="HIP device tensor"):
        hh.peaks(x, work, rows, vals, n, p, table, 1, None, 4)
    with pytest.raises(RuntimeError, match="HIP device tensor"):          # an empty plane too
        hh.peaks(x[:0], work[:0], rows, vals, n, p, hh.Table(host[:1] * 0, host[:1], 1), 1, None, 4)
    with pytest.raises(RuntimeError, match=r"scores must be \[NW, K\] and work flat"):
        hh.peaks(x.view(-1), work, rows, vals, n, p, table, 1, None, 4)
    with pytest.raises(RuntimeError, match=r"scores must be \[NW, K\] and work flat"):
        hh.peaks(x, work.view(7, 2), rows, vals, n, p, table, 1, None, 4)
    with pytest.raises(RuntimeError, match=r"hit_rows has shape \(2, 4\), expected \(2, 5\)"):
        hh.peaks(x, work, rows, vals, n, p, table, 1, None, 5)
    with pytest.raises(RuntimeError, match=r"hit_scores has shape \(2, 3\), expected \(2, 4\)"):
        hh.peaks(x, work, rows, vals[:, :3], n, p, table, 1, None, 4)
    with pytest.raises(RuntimeError, match=r"n_hits has shape \(1,\), expected \(2,\)"):
        hh.peaks(x, work, rows, vals, n[:1], p, table, 1, None, 4)
    with pytest.raises(RuntimeError, match=r"n_peaks has shape \(1,\), expected \(2,\)"):
        hh.peaks(x, work, rows, vals, n, p[:1], table, 1, None, 4)
    with pytest.raises(RuntimeError, match="work holds 13 words, a plane of 7 x 2 scores needs 14"):
        hh.peaks(x, work[:13], rows, vals, n, p, table, 1, None, 4)
    for top in (0, 4097, True, 2.0):
        with pytest.raises(RuntimeError, match=r"top must be an integer in \[1, 4096\]"):
            hh.peaks(x, work, rows, vals, n, p, table, 1, None, top)
    for sep in (-1, 4097, False, 1.0):
        with pytest.raises(RuntimeError, match=r"separation must be an integer in \[0, 4096\]"):
            hh.peaks(x, work, rows, vals, n, p, table, sep, None, 4)
    with pytest.raises(RuntimeError, match="scores has K = 65 columns, the search takes 1 .. 64 classes"):
        hh.peaks(torch.zeros(7, 65), work, rows, vals, n, p, table, 1, None, 4)
    with pytest.raises(RuntimeError, match="min_score is NaN"):
        hh.peaks(x, work, rows, vals, n, p, table, 1, NAN, 4)
    with pytest.raises(RuntimeError, match="Table"):
        hh.peaks(x, work, rows, vals, n, p, hh.Table(host[:, :6], host, 3), 1, None, 4)


# ------------------------------------------------------------------ the option's type, the plan and the rule
def test_history_refusals_name_the_field():
    from clip_fsar_amd.history import History, check_min_score, check_separation, check_top, device_separation, largest_frames
    assert History(4096) == (4096,) and History(frames=1).frames == 1
    for bad in (0, -5, 2.0, True, "4096", None, (4096,)):
        with pytest.raises(ValueError, match=r"History: frames must be an integer >= 1"):
            History(bad)
    assert largest_frames(64, 512) == 65535 and largest_frames(1, 1) == (1 << 31) - 1 and largest_frames(65536, 1024) == 31
    assert 64 * 65535 * 512 <= (1 << 31) - 1 < 64 * 65536 * 512
    for bad in (0, 4097, True, 1.0, None):
        with pytest.raises(ValueError, match=r"X: top must be an integer in \[1, 4096\]"):
            check_top(bad, "X")
    for bad in (-1, True, 1.0, "3"):
        with pytest.raises(ValueError, match="X: separation must be an integer >= 0"):
            check_separation(bad, "X")
    for bad in (NAN, True, "0.5", (0.5,)):
        with pytest.raises(ValueError, match="X: min_score must be None or a number that is not NaN"):
            check_min_score(bad, "X")
    assert check_min_score(None) is None and check_min_score(0.1) == float(np.float32(0.1)) and check_min_score(-INF) == -INF
    assert check_min_score(1e39) == INF and check_min_score(3) == 3.0                     # as fp32
    assert [device_separation(s, [5, 0, 9]) for s in (0, 3, 8, 9, 10 ** 9)] == [0, 3, 8, 8, 8]
    assert device_separation(7, []) == 0 and device_separation(7, [0, 0]) == 0 and device_separation(7, [1]) == 0
    assert device_separation(10 ** 9, [4097]) == 4096
    with pytest.raises(ValueError, match=r"X: separation = 5000 over a longest row of 4098 windows -- the search stages at most 4096"):
        device_separation(5000, [3, 4098], "X")


def test_plan_search_on_hand_written_sessions():
    from clip_fsar_amd.history import held_windows, plan_search
    from clip_fsar_amd.pool import enrolable_windows, plan_enroll, tempo_positions
    T, stride, F = 4, 2, 10
    # 25 frames: the store holds frames 15 .. 24, so windows 8 .. 10 (frames 16 .. 19, .., 20 .. 23); it has wrapped twice
    plan = plan_search([(2, 25), (0, 3), (1, 9), (3, 10), (5, 11)], T, stride, 1, F)
    assert plan.rows == [[2, 5, 0, 0, 6, 3, 0, 0],            # PUT_POS 25 mod 10, WIN_POS 16 mod 10
                         [0, 3, 0, 0, 0, 0, 3, 0],            # three frames: no window yet; its next window will be number 0
                         [1, 9, 0, 0, 0, 3, 3, 0],            # nine frames, nothing has left: windows 0 .. 2
                         [3, 0, 0, 0, 0, 4, 6, 0],            # exactly full: PUT_POS wraps to 0, windows 0 .. 3
                         [5, 1, 0, 0, 2, 3, 10, 0]]           # frame 0 is gone, so window 0 is: windows 1 .. 3 from position 2
    assert (plan.first_window, plan.n_windows, plan.offsets) == ([8, 0, 0, 0, 1], [3, 0, 3, 4, 3], [0, 3, 3, 6, 10, 13])
    for (slot, t), first, n in zip([(2, 25), (0, 3), (1, 9), (3, 10), (5, 11)], plan.first_window, plan.n_windows):
        ws = enrolable_windows(t, T, stride, 1, F)
        assert held_windows(t, T, stride, 1, F) == ws and n == len(ws) and (not n or first == ws.start)
        if n:                                     # the *_hit methods read where the search gathered
            assert plan_enroll([(slot, t)], [(0, first)], T, stride, 1, F).positions == [plan.rows[[r[0] for r in plan.rows].index(slot)][4]]
    # the gather's own validation admits the rows: a row's windows span at most F positions
    for row in plan.rows:
        assert row[5] == 0 or (row[5] - 1) * stride + (T - 1) + 1 <= F
    # last=n: the windows completed by one of the newest n frames; window w is completed by frame 2 w + 3
    assert [len(held_windows(25, T, stride, 1, F, last)) for last in (1, 2, 3, 4, 9, 10, 99)] == [0, 1, 1, 2, 3, 3, 3]
    assert held_windows(25, T, stride, 1, F, 2) == range(10, 11) and held_windows(24, T, stride, 1, F, 1) == range(10, 11)
    plan = plan_search([(2, 25), (1, 9)], T, stride, 1, F, last=4)
    assert plan.rows == [[2, 5, 0, 0, 8, 2, 0, 0], [1, 9, 0, 0, 2, 2, 2, 0]] and plan.first_window == [9, 1]
    assert plan_search([(2, 25)], T, stride, 1, F, last=1).rows == [[2, 5, 0, 0, 2, 0, 0, 0]]       # none: first_window = the next one
    assert plan_search([(2, 25)], T, stride, 1, F, last=1).first_window == [11]
    # a pool with rates = (1, 3): it plans with rate 3, cap F = 12; tempo 0 is read `shift` = (T - 1) * (3 - 1) frames further on
    rates, F = (1, 3), 12
    slow = plan_search([(0, 30)], T, stride, 3, F)
    fast = plan_search([(0, 30)], T, stride, 3, F, shift=(T - 1) * 2)
    assert slow.rows == [[0, 6, 0, 0, 6, 2, 0, 0]] and slow.first_window == [9]                # windows 9, 10: frames 18 .. 27, 20 .. 29
    assert fast.rows == [[0, 6, 0, 0, 0, 2, 0, 0]] and fast.first_window == [9]                # frames 24 .. 27, 26 .. 29
    for w in range(2):
        at = tempo_positions(slow.rows[0][4], w, stride, T, rates, F)
        assert at[1] == [(slow.rows[0][4] + w * stride + j * 3) % F for j in range(T)]
        assert at[0] == [(fast.rows[0][4] + w * stride + j * 1) % F for j in range(T)]
    assert plan_search([], T, stride, 1, F) == ([], [], [], [0])


def _search(rows, sep, floor=None, top=99):
    """rows: per session row its scores of ONE class -> (the kept plane rows, the peak count)"""
    from clip_fsar_amd.history import reference_search
    plane = np.array([[v] for r in rows for v in r], dtype=np.float32).reshape(-1, 1)
    hits, peaks = reference_search(plane, [len(r) for r in rows], sep, floor, top)
    return hits[0], peaks[0]


def test_reference_search_hand_rows():
    from clip_fsar_amd.history import reference_search
    # a local maximum within the distance; a tie goes to the earlier window; a plateau yields its first window only
    assert _search([[0.1, 0.5, 0.2, 0.4, 0.3]], 1) == ([1, 3], 2)
    assert _search([[0.1, 0.5, 0.2, 0.4, 0.3]], 2) == ([1], 1)
    assert _search([[0.5, 0.1, 0.5]], 2) == ([0], 1) and _search([[0.5, 0.1, 0.5]], 1) == ([0, 2], 2)
    assert _search([[0.5, 0.5, 0.5, 0.5]], 1) == ([0], 1)             # 2 is beaten by 1, which is no peak itself: a filter, not suppression
    assert _search([[0.3, 0.2, 0.1]], 1) == ([0], 1) and _search([[0.1, 0.2, 0.3]], 1) == ([2], 1)
    # -0.0 against +0.0: equal, so the earlier window wins
    assert _search([[-0.0, 0.0]], 1) == ([0], 1) and _search([[0.0, -0.0]], 1) == ([0], 1) and _search([[-1.0, -0.0, 0.0]], 2) == ([1], 1)
    # NaN and -inf neighbours neither count nor suppress
    assert _search([[NAN, 0.5, NAN]], 1) == ([1], 1) and _search([[-INF, -FMAX, -INF]], 1) == ([1], 1)
    assert _search([[NAN, -INF, NAN]], 1) == ([], 0)
    assert _search([[0.5, NAN, 0.4]], 1) == ([0, 2], 2) and _search([[0.5, NAN, 0.4]], 2) == ([0], 1)      # the distance counts windows, not candidates
    # +inf is a candidate like any other, and two of them tie
    assert _search([[FMAX, INF, INF, FMAX]], 1) == ([1], 1) and _search([[INF, 0.0, INF]], 1) == ([0, 2], 2)
    # separation = 0: every candidate is a peak; separation >= the row length: one peak per row, whatever the number
    assert _search([[0.5, 0.5, NAN, 0.1]], 0) == ([0, 1, 3], 3)
    assert _search([[0.1, 0.9, 0.5, 0.9]], 3) == _search([[0.1, 0.9, 0.5, 0.9]], 4) == _search([[0.1, 0.9, 0.5, 0.9]], 10 ** 6) == ([1], 1)
    # a row boundary separates two adjacent maxima: rows never see each other's windows
    assert _search([[0.1, 0.9], [0.8, 0.2]], 3) == ([1, 2], 2) and _search([[0.1, 0.9, 0.8, 0.2]], 3) == ([1], 1)
    assert _search([[0.9], [], [0.9], [NAN]], 5) == ([0, 1], 2)
    # min_score equal to a score keeps it (>= as fp32); below it nothing counts or suppresses
    assert _search([[0.5, 0.25, 0.75]], 1, 0.75) == ([2], 1) and _search([[0.5, 0.25, 0.75]], 1, 0.5) == ([0, 2], 2)
    assert _search([[0.1, 0.25, 0.2]], 1, 0.1) == ([1], 1)
    assert _search([[0.1, 0.25, 0.2]], 1, float(np.float32(0.1)) * (1 + 2 ** -20)) == ([1], 1)
    third = float(np.float32(1 / 3))
    assert _search([[third]], 0, 1 / 3) == ([0], 1) and _search([[third]], 0, float(np.nextafter(np.float32(third), np.float32(1)))) == ([], 0)
    assert _search([[0.5, -INF]], 0, -INF) == ([0], 1) and _search([[INF, FMAX]], 0, INF) == ([0], 1)
    # top: the highest peaks, returned in ascending plane-row order; a tie at the last place goes to the lower row
    rows = [[0.5, 0.0, 0.9, 0.0, 0.5], [0.5, 0.0, 0.7]]
    assert _search(rows, 1) == ([0, 2, 4, 5, 7], 5)
    assert _search(rows, 1, top=1) == ([2], 5) and _search(rows, 1, top=2) == ([2, 7], 5)
    assert _search(rows, 1, top=3) == ([0, 2, 7], 5) and _search(rows, 1, top=4) == ([0, 2, 4, 7], 5)
    assert _search([[0.0], [-0.0], [0.0]], 0, top=2) == ([0, 1], 3)
    # several classes at once, each on its own
    hits, peaks = reference_search(torch.tensor([[1.0, 0.0], [2.0, NAN], [3.0, 5.0], [0.5, 5.0]]), [2, 2], 1, None, 1)
    assert (hits, peaks) == ([[2], [2]], [2, 2])
    assert reference_search(np.zeros((0, 3), dtype=np.float32), [0, 0], 1, None, 4) == ([[], [], []], [0, 0, 0])
    for bad, words in (((np.zeros(3), [3], 1, None, 1), r"scores must be \[NW, K\]"), ((np.zeros((3, 1)), [2], 1, None, 1), "the rows hold"),
                       ((np.zeros((3, 1)), [3], -1, None, 1), "separation must be"), ((np.zeros((3, 1)), [3], 1, None, 0), "top must be"),
                       ((np.zeros((3, 1)), [3], 1, NAN, 1), "min_score must be")):
        with pytest.raises(ValueError, match="reference_search: " + words):
            reference_search(*bad)


# ------------------------------------------------------------------ the option
def test_the_history_option_on_stub_heads():
    from clip_fsar_amd.events import EventRule
    from clip_fsar_amd.history import History, Hit
    from clip_fsar_amd.live_text_gallery import LiveTextGallery
    from clip_fsar_amd.pool import StreamPool
    from clip_fsar_amd.still import StillGate
    g = _live()                                   # T = 4, E = 8, classes 0, 1, 2
    hist = History(frames=64)
    p = StreamPool(g, max_streams=3, stride=2, max_push=5, history=hist)          # TypeError without the feature
    assert p.cap == 8 and p._history == hist and p._hs_store is None and p._hs_X is None and p._hs_work is None      # nothing is allocated yet
    for bad in (64, (64,), "64", {"frames": 64}):
        with pytest.raises(TypeError, match="StreamPool: history must be a History"):
            StreamPool(g, history=bad)
    with pytest.raises(TypeError):
        StreamPool(g, 3, 1, 1, 5, 0.0, None, "column", None, None, hist)            # keyword-only: the eleventh positional argument
    with pytest.raises(ValueError, match=r"history.frames = 7 is below the ring's cap = \(T - 1\) \* rate \+ max_push = 8 .* give at least 8"):
        StreamPool(g, max_push=5, history=History(7))
    assert StreamPool(g, max_push=5, history=History(8))._history.frames == 8
    with pytest.raises(ValueError, match=r"history.frames = 12 is below the ring's cap .* = 14"):
        StreamPool(g, max_push=5, rates=(1, 3), history=History(12))                # the ring of a tempo pool is planned with the largest rate
    most = ((1 << 31) - 1) // (3 * 8)
    with pytest.raises(ValueError, match=r"history.frames = %d x max_streams = 3 rows of E = 8 floats break the pool library's 32-bit item "
                       r"limit -- the largest frames that fits is %d" % (most + 1, most)):
        StreamPool(g, max_streams=3, history=History(most + 1))
    for flags in (dict(COMBINE=True), dict(EVAL_TEXT=True)):
        text = LiveTextGallery(_stub_head(**flags), "cpu", capacity=4)
        with pytest.raises(ValueError, match="history= on a LiveTextGallery is not supported -- a softmax over the searched classes alone is "
                           "another quantity"):
            StreamPool(text, history=hist)
    # it combines with the other options and adds nothing to stats(); a pool without it is the pool as it was
    q = StreamPool(g, max_streams=3, smooth=0.5, smooth_by="class", events=EventRule(0.6, 0.4, 2, 2), rates=(1, 2), still=StillGate(), history=History(128))
    assert q.stats() == {"frames": 0, "tower_frames": 0, "windows": 0, "events": 0, "events_dropped": 0, "still_frames": 0, "open": 0}
    plain = StreamPool(g, max_streams=3, stride=2, max_push=5)
    assert plain._history is None and plain.stats() == p.stats()
    assert not any(hasattr(plain, a) for a in ("_hs_store", "_hs_tables", "_hs_X", "_hs_work"))
    hit = Hit(0, 1, 0, 0.5, None)
    for call, name in ((lambda: plain.search([0]), "search"), (lambda: plain.searchable(0), "searchable"), (lambda: plain.hit_features(hit), "hit_features"),
                       (lambda: plain.explain_hit(hit), "explain_hit"), (lambda: plain.enroll_hit(hit, 1), "enroll_hit")):
        with pytest.raises(ValueError, match=r"StreamPool.%s: this pool keeps no history \(build it with history=History" % name):
            call()
    # search: every refusal before anything is allocated or launched
    a, b = p.open(), p.open()
    for bad, words in (([], "classes= needs at least one class"), ([0, 0], r"a class appears twice in classes=: \[0, 0\]"), ([0, 7], "7")):
        with pytest.raises(ValueError, match="StreamPool.search: .*" + words):
            p.search(bad)
    for bad in (0, "01", None, {0, 1}):
        with pytest.raises(TypeError, match="StreamPool.search: classes must be a list of registered class ids"):
            p.search(bad)
    big = _live(capacity=80, ids=tuple(range(70)))
    with pytest.raises(ValueError, match="StreamPool.search: 65 classes -- one search takes 1 to 64"):
        StreamPool(big, max_push=5, history=hist).search(list(range(65)))
    with pytest.raises(ValueError, match=r"StreamPool.search: a session appears twice in sessions=: \[0, 1, 0\]"):
        p.search([0], sessions=[a, b, a])
    with pytest.raises(ValueError, match="session 9 is not open"):
        p.search([0], sessions=[a, 9])
    with pytest.raises(TypeError, match="StreamPool.search: sessions must be None or a list of open sessions"):
        p.search([0], sessions=a)
    for kw, words in ((dict(top=0), r"top must be an integer in \[1, 4096\], got 0"), (dict(top=4097), "top must be"), (dict(top=2.0), "top must be"),
                      (dict(separation=-1), "separation must be an integer >= 0, got -1"), (dict(separation=1.5), "separation must be"),
                      (dict(last=0), "last must be None or an integer >= 1"), (dict(last=True), "last must be"),
                      (dict(min_score=NAN), "min_score must be None or a number that is not NaN"), (dict(min_score="1"), "min_score must be"),
                      (dict(tempo=0), "tempo = 0 on a pool without rates=")):
        with pytest.raises(ValueError, match="StreamPool.search: " + words):
            p.search([0, 1], **kw)
    with pytest.raises(ValueError, match=r"StreamPool.search: tempo must be an index into rates = \(1, 2\), 0 .. 1"):
        q.search([0], tempo=2)
    # nothing is held yet: empty lists, nothing launched, nothing allocated
    assert p.searchable(a) == range(0) and p.searchable(b) == range(0)
    r = p.search([2, 0], top=3, min_score=0.5, separation=0, last=4)
    assert r.hits == {2: [], 0: []} and r.peaks == {2: 0, 0: 0} and r.windows == 0 and tuple(r.scores.shape) == (0, 2)
    assert (r.sessions, r.first_window, r.offsets) == ([a, b], [0, 0], [0, 0, 0])
    assert p.search([1], sessions=[]).sessions == [] and p._hs_store is None and p._hs_X is None and p._hs_work is None
    # the frame counters alone say what is held: open() and reset() start at frame 0, close() ends the session
    p._sessions[a].t = 70
    assert p.searchable(a) == range(3, 34) and len(p.searchable(a)) == 31
    with pytest.raises(ValueError, match=r"StreamPool.search: separation = 5000 over a longest row of 4999 windows"):
        big_pool = StreamPool(g, stride=2, max_push=5, history=History(10000))
        big_pool.open()
        big_pool._sessions[0].t = 12000
        big_pool.search([0], separation=5000, sessions=[0])
    p.reset(a)
    assert p.searchable(a) == range(0)
    p._sessions[a].t = 70
    # the *_hit methods: a Hit of an open session whose window the history still holds, read at the hit's tempo
    for bad in ((a, 1, 3, 0.5, None), None, 3):
        with pytest.raises(TypeError, match="StreamPool.hit_features: takes a Hit that search"):
            p.hit_features(bad)
    with pytest.raises(ValueError, match="session 9 is not open"):
        p.explain_hit(Hit(9, 1, 3, 0.5, None))
    with pytest.raises(ValueError, match=r"StreamPool: session %d: window 2 is not enrolable -- the ring holds its windows range\(3, 34\) "
                       r"\(70 frames since open\(\) / reset\(\), cap = 64\)" % a):
        p.enroll_hit(Hit(a, 1, 2, 0.5, None), 1)
    with pytest.raises(ValueError, match=r"window 34 is not enrolable"):
        p.hit_features(Hit(a, 1, 34, 0.5, None))
    with pytest.raises(ValueError, match="StreamPool.hit_features: tempo = 1 on a pool without rates="):
        p.hit_features(Hit(a, 1, 5, 0.5, 1))
    p.close(a)
    with pytest.raises(ValueError, match="session %d is not open" % a):
        p.searchable(a)
    assert p.search([0]).sessions == [b]
