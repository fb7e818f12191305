"""CPU: the shortlist (libclipfsar_shortlist.so, include/ext/clipfsar_shortlist.h, clip_fsar_amd.shortlist_hip, clip_fsar_amd.shortlist)
-- the plug-in library's exports, ABI check at load, resource report and place in the build (one more name of the open registry,
build.PLUGIN_LIBS); the host validation of its three entry points without a GPU; reference_select on hand-written cases; the bound of
the coarse scores, derived here and pinned to the reference evaluated in float32; LiveGallery.slot_revision and Shortlist's refresh
bookkeeping on stub heads; every Shortlist argument error.

The bound of a coarse score against the float64 reference (tests/test_gpu_shortlist.py holds the kernels to it).  S = <u_q, u_p>, u the
mean of a sequence's unit-normalised rows, so |u| <= rho, rho = the largest |x_t| / d_t over the rows (d_t is the fp32 norm the kernel is
given: rho = 1 up to the rounding of that norm; every case asserts rho <= 1.0005).  Two parts:
  * the dot product is the exact-fp32 tile GEMM behind tests/test_gpu_otam.py's e_d = 1e-6 * max(1, sqrt(E / 1024)) on operands of norm
    at most 1;
  * the fp32 rounding of the two mean rows.  An element is fl(inv * sum_t fl(x_te / d_t)), inv = fl(1 / T): every term passes through
    at most T + 2 roundings (its quotient, T - 1 rounded adds -- the first add, to 0, is exact --, inv, the product), so
    |du_e| <= (T + 2) u a_e with u = 2^-24 and a_e = (1 / T) sum_t |x_te| / d_t, and |a| <= rho by the triangle inequality.  By
    Cauchy-Schwarz |<du_q, u_p>| + |<u_q, du_p>| <= 2 (T + 2) u rho^2.
bound(T, E) = 1.01 * (e_d(E) + 2 (T + 2) 2^-24); the 1 % covers rho^2, the second-order terms and operands of norm rho instead of 1.
A mean row on its own is held to the second part alone, element by element: row_bound = 1.01 * (T + 2) 2^-24 a_e (+ (T + 2) 2^-149: a
quotient or a sum in the denormals is rounded to that absolute step instead)."""
import ctypes
import json
import math
import os
import re
from types import SimpleNamespace as NS

import pytest

import _abi
from _abi import check_abi_at_load, check_exports

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ext", "clipfsar_shortlist.h")
KERNELS = {"mean_unit_rows_kernel": 1, "coarse_scores_kernel": 1, "select_kernel": 1}
ROW = _abi._row("shortlist", "shortlist_hip", "cfsh_", "ext/clipfsar_shortlist.h",
                "version abi_version last_error mean_unit_rows coarse_scores workspace_floats select", KERNELS, 3)
INF, NAN = float("inf"), float("nan")
NONE = 0x7fffffff


def bound(T, E):
    return 1.01 * (1e-6 * max(1.0, math.sqrt(E / 1024.0)) + 2 * (T + 2) * 2.0 ** -24)


def row_bound(X, norms, tiny=1e-12):
    """[n, E] float64: the bound of a mean unit row's elements against reference_mean_unit_rows, from X [n, T, E] and the norms as given"""
    n, T, _ = X.shape
    a = (X.double().abs() / norms.double().reshape(n, T, 1).clamp_min(tiny)).sum(1) / T
    return 1.01 * (T + 2) * 2.0 ** -24 * a + (T + 2) * 2.0 ** -149


def sequences(family, n, T, E, seed):
    """(X [n, T, E] fp32, norms [n * T] fp32: the rows' norms evaluated in fp32) of a family: gauss -- independent rows, coarse scores near
    0; near -- every row of every sequence close to one direction, coarse scores near 1, the like-signed sums the tile GEMM was fixed for;
    scale -- gauss rows of lengths 1e-3 .. 1e3"""
    import torch
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(n, T, E, generator=g)
    if family == "near":
        X = torch.ones(E)[None, None, :] / math.sqrt(E) + 0.05 * X / math.sqrt(E)
    elif family == "scale":
        X = X * (10.0 ** (torch.rand(n, T, 1, generator=g) * 6 - 3))
    X = X.float().contiguous()
    return X, X.norm(dim=-1).reshape(-1).contiguous()


def rho(X, norms):
    n, T, _ = X.shape
    return float((X.double().norm(dim=-1) / norms.double().reshape(n, T)).max())


@pytest.fixture(scope="module")
def clib():
    import __graft_entry__ as ge
    ge.build()                                    # builds every library (no-op when up to date)
    from clip_fsar_amd import shortlist_hip
    return shortlist_hip.lib()


# ------------------------------------------------------------------ the library and its place in the build
def test_header_exported_exactly_and_arity_matches(clib):
    check_exports(ROW)
    assert ROW.exports == {"cfsh_" + e for e in ("version", "abi_version", "last_error", "mean_unit_rows", "coarse_scores",
                                                 "workspace_floats", "select")}
    from clip_fsar_amd import shortlist as sl
    from clip_fsar_amd import shortlist_hip as sh
    text = open(HEADER).read()
    for name in ("MAX_T", "MAX_KEEP", "MAX_GROUPS", "TABLE_COLS", "Q0", "NQ"):
        assert int(re.search(r"#define CFSH_%s (\d+)" % name, text).group(1)) == getattr(sh, name), name
    assert sh.MAX_KEEP == sl.MAX_KEEP == 4096 and sh.MAX_GROUPS == 65536
    assert int(re.search(r"#define CFSH_NONE (0x[0-9a-f]+)", text).group(1), 16) == sh.NONE == sl.NONE == NONE
    assert float(re.search(r"#define CFSH_TINY ([0-9.e-]+)f", text).group(1)) == sh.TINY == sl.TINY
    assert [len(sh.SIGNATURES["cfsh_" + e]) for e in ("mean_unit_rows", "coarse_scores", "workspace_floats", "select")] == [9, 9, 2, 12]
    for other in _abi.LIBS:                       # its prefix hides no other library's, and none hides it
        assert not other.prefix.startswith(ROW.prefix) and not ROW.prefix.startswith(other.prefix), other.name
    for prefix in ("cfcs_", "cfev_", "cfbl_"):
        assert not prefix.startswith(ROW.prefix) and not ROW.prefix.startswith(prefix)
    assert clib.cfsh_workspace_floats(3, 5) == 15 == sh.workspace_floats(3, 5)
    for G, NC in ((0, 5), (65537, 5), (3, 0), (65536, 1 << 15), (-1, -1)):
        assert clib.cfsh_workspace_floats(G, NC) == -1, (G, NC)
        with pytest.raises(RuntimeError, match="no workspace"):
            sh.workspace_floats(G, NC)
    assert clib.cfsh_workspace_floats(65536, (1 << 15) - 1) == 65536 * ((1 << 15) - 1)


def test_abi_version_is_checked_at_load(clib, monkeypatch):
    check_abi_at_load(ROW, monkeypatch)


def test_the_kernels_are_the_listed_ones_and_use_no_scratch(clib):
    from clip_fsar_amd import build as b
    from clip_fsar_amd import shortlist_hip as sh
    pl = b.PLUGIN_LIBS["shortlist"]
    if not os.path.exists(pl.usage):
        b.build_plugin("shortlist", force=True, verbose=False)
    usage = json.load(open(pl.usage))
    assert len(usage) == ROW.total == sum(KERNELS.values()), sorted(usage)
    for fragment, count in KERNELS.items():
        assert sum(fragment in n for n in usage) == count, (fragment, sorted(usage))
    for n, u in usage.items():
        assert u.get("scratch", 0) == 0 and u.get("spills", 0) == 0, (n, u)
    assert os.path.normpath(pl.usage).endswith(os.path.join("build", "shortlist", "resource_usage.json"))
    assert pl.lib == sh.LIB_PATH and pl.lib.endswith(os.sep + "libclipfsar_shortlist.so") and os.path.exists(pl.lib)
    others = [b.USAGE] + [x.usage for reg in (b.SIDE_LIBS, b.EXT_LIBS, b.ADDON_LIBS) for x in reg.values()]
    others += [x.usage for n, x in b.PLUGIN_LIBS.items() if n != "shortlist"]
    for path in others:                           # and no other library's report names them
        if os.path.exists(path):
            assert not any(fragment in n for n in json.load(open(path)) for fragment in KERNELS), path
    # the conventions: the shared error plumbing, the tree's tile GEMM and slot arithmetic; no assembly, no allocation, no stream of its
    # own, no second MFMA; the only atomics are the histogram counts in LDS
    source = open(pl.source).read()
    assert '#include "../csrc/otam_tile.h"' in source and '#include "../../include/ext/clipfsar_shortlist.h"' in source
    assert source.count("fp32_tile_gemm_rows(") == 1 and source.count("store_slot_row(") == 2 and "LookedUpRow{" in source
    for body in ("asm", "thread_local", "calloc", "malloc", "hipMalloc", "hipStreamCreate", "__builtin_amdgcn_mfma", "hipMemcpy",
                 "hipDeviceSynchronize", "hipStreamSynchronize", "while"):
        assert body not in source, body
    assert len(re.findall(r"atomic\w*\(", source)) == source.count("atomicAdd(&hist[") == 1 and "__shared__ unsigned hist[" in source
    assert "contract(off)" in source and "__fdiv_rn" in source and "fmaf" not in source


def test_shortlist_is_a_name_of_the_open_registry_and_follows_the_recipe():
    from clip_fsar_amd import build as b
    assert "shortlist" in b.PLUGIN_LIBS and "shortlist" in b.plugin_lib_names()
    assert all("shortlist" not in reg for reg in (b.SIDE_LIBS, b.EXT_LIBS, b.ADDON_LIBS))
    pl = b.PLUGIN_LIBS["shortlist"]
    assert isinstance(pl, b.ExtLib)
    assert pl.source == os.path.join(b.EXT, "shortlist.hip") and os.path.exists(pl.source)
    assert pl.header == HEADER and os.path.exists(pl.header)
    assert pl.lib == os.path.join(b.HERE, "libclipfsar_shortlist.so")
    assert pl.usage == os.path.join(b.HERE, "build", "shortlist", "resource_usage.json")
    deps = b._plugin_deps("shortlist")
    for f in (pl.source, pl.header, os.path.abspath(b.__file__), os.path.join(b.CSRC, "otam_tile.h"), os.path.join(b.CSRC, "side_lib.h"),
              os.path.join(b.CSRC, "fp32_tile_gemm.h")):
        assert f in deps, f
    for call in (b.build_side, b._side_deps, b.build_ext, b._ext_deps, b.build_addon, b._addon_deps):       # the three closed registries
        with pytest.raises(KeyError):
            call("shortlist")
    assert not os.path.exists(os.path.join(b.CSRC, "shortlist.hip"))
    assert not any("shortlist" in open(os.path.join(b.CSRC, f)).read() for f in os.listdir(b.CSRC))        # nothing of csrc/ knows it


def test_staleness_of_the_shortlist_and_of_nothing_else(monkeypatch):
    from clip_fsar_amd import build as b
    from test_build_recipe import NAMES, STALE, P
    monkeypatch.setattr(b.os.path, "exists", lambda p: True)

    def stale_after(edited):
        monkeypatch.setattr(b.os.path, "getmtime", lambda p: 2.0 if p.endswith(os.sep + edited) else 1.0)
        old = {P} if b._stale(b.LIB, b._product_deps()) else set()
        old |= {n for n in NAMES if b._stale(b.SIDE_LIBS[n].lib, b._side_deps(n))}
        return old, b._stale(b.PLUGIN_LIBS["baseline"].lib, b._plugin_deps("baseline")), \
            b._stale(b.PLUGIN_LIBS["shortlist"].lib, b._plugin_deps("shortlist"))

    for edited in ("shortlist.hip", "clipfsar_shortlist.h"):                      # its own files: it alone
        assert stale_after(edited) == (set(), False, True), edited
    for edited in ("otam_tile.h", "fp32_tile_gemm.h", "otam_dp.h"):               # the tile code it shares with the OTAM libraries
        assert stale_after(edited) == (STALE[edited], False, True), edited
    for edited in ("side_lib.h", "build.py", "common.h", "clipfsar_hip.h"):       # what every library reaches
        assert stale_after(edited) == (STALE[edited], True, True), edited
    for edited in ("baseline.hip", "clipfsar_baseline.h", "chunk_row.h", "ring_rows.h"):
        assert stale_after(edited)[1:] == (True, False), edited
    for edited in ("groups.hip", "clipfsar_groups.h", "topk_wave.h", "text_softmax.h", "gemm.hip", "class_smooth.hip", "events.hip"):
        assert stale_after(edited)[1:] == (False, False), edited
    assert stale_after("no_such_file.h") == (set(), False, False)


# ------------------------------------------------------------------ validation, without a GPU
def _tbl(rows):
    flat = [v for r in rows for v in r]
    return (ctypes.c_int32 * len(flat))(*flat)


def test_mean_unit_rows_validation_without_gpu(clib):
    p, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4100)   # never dereferenced: every call below fails validation before any device work
    err = clib.cfsh_last_error

    def call(X=p, norms=p, slots=p, out=p, n=3, cap=5, T=8, E=64):
        return clib.cfsh_mean_unit_rows(X, norms, slots, out, n, cap, T, E, None)

    for kw in ({"X": None}, {"norms": None}, {"out": None}):
        assert call(**kw) != 0 and b"null pointer" in err(), kw
    for n in (0, -1):
        assert call(n=n) != 0 and b" n=" in err(), n
    for cap in (0, -4):
        assert call(cap=cap) != 0 and b"cap=" in err(), cap
    for T in (0, -1, 33):
        assert call(T=T) != 0 and b"T=" in err(), T
    for E in (0, 2, 6, 63, 8196, -4):
        assert call(E=E) != 0 and b"E=" in err(), E
    assert call(cap=1 << 27, T=32) != 0 and b"cap * T" in err()
    assert call(slots=None, n=6, cap=5) != 0 and b"without a slot list" in err()
    assert call(n=6, cap=5, X=odd) != 0 and b"16-byte aligned" in err()          # with a list n may exceed cap
    assert call(out=odd) != 0 and b"16-byte aligned" in err()


def test_coarse_scores_validation_without_gpu(clib):
    p, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4104)
    err = clib.cfsh_last_error

    def call(U=p, C=p, cols=p, S=p, NQ=3, NC=5, cap=7, E=64):
        return clib.cfsh_coarse_scores(U, C, cols, S, NQ, NC, cap, E, None)

    for kw in ({"U": None}, {"C": None}, {"cols": None}, {"S": None}):
        assert call(**kw) != 0 and b"null pointer" in err(), kw
    for NQ in (0, -1):
        assert call(NQ=NQ) != 0 and b"NQ=" in err(), NQ
    for NC in (0, -1):
        assert call(NC=NC) != 0 and b"NC=" in err(), NC
    for cap in (0, -1):
        assert call(cap=cap) != 0 and b"cap=" in err(), cap
    for E in (0, 2, 6, 63, 8196):
        assert call(E=E) != 0 and b"E=" in err(), E
    assert call(NQ=1 << 16, NC=1 << 15) != 0 and b"NQ * NC" in err()
    assert call(NQ=65535 * 64 + 1, NC=1) != 0 and b"too large for one launch" in err()
    assert call(U=odd) != 0 and b"16-byte aligned" in err()
    assert call(C=odd) != 0 and b"16-byte aligned" in err()


GOOD = [[0, 3], [3, 0], [3, 17], [20, 1]]            # (Q0, NQ): NQ = 21


def test_select_validation_without_gpu(clib):
    p = ctypes.c_void_p(4096)
    err, good = clib.cfsh_last_error, _tbl(GOOD)

    # select(S, cols, table_host, table_dev, G, NQ, NC, keep, sel_cols, sel_slots, work, stream)
    def call(t=good, G=4, NQ=21, NC=100, keep=8, ptrs=None):
        a = ptrs or [p, p, t, p, p, p, p]
        return clib.cfsh_select(a[0], a[1], a[2], a[3], G, NQ, NC, keep, a[4], a[5], a[6], None)

    for i in range(7):
        ptrs = [p, p, good, p, p, p, p]
        ptrs[i] = None
        assert call(ptrs=ptrs) != 0 and b"null pointer" in err(), i
    for G in (0, -1, 65537):
        assert call(G=G) != 0 and b"G=" in err(), G
    for NQ in (0, -5):
        assert call(NQ=NQ) != 0 and b"NQ=" in err(), NQ
    for NC in (0, -1):
        assert call(NC=NC) != 0 and b"NC=" in err(), NC
    for keep in (0, -1, 4097):
        assert call(keep=keep) != 0 and b"keep=" in err(), keep
    assert call(t=_tbl([[0, 1 << 16]]), G=1, NQ=1 << 16, NC=1 << 15) != 0 and b"NQ * NC" in err()
    big = _tbl([[0, 1]] + [[1, 0]] * 65535)
    assert call(t=big, G=65536, NQ=1, NC=1 << 15) != 0 and b"G * NC" in err()

    def edit(row, col, value):
        rows = [list(r) for r in GOOD]
        rows[row][col] = value
        return _tbl(rows)

    assert call(t=edit(1, 1, -1)) != 0 and b"group 1" in err() and b"NQ=-1" in err()
    assert call(t=edit(2, 0, 4)) != 0 and b"group 2" in err() and b"Q0=4" in err()
    assert call(t=edit(0, 0, 1)) != 0 and b"group 0" in err() and b"Q0=1" in err()
    assert call(t=edit(3, 1, 2)) != 0 and b"add up to 22 queries, not to NQ = 21" in err()
    assert call(NQ=20) != 0 and b"not to NQ = 20" in err()


def test_python_wrappers_reject_cpu_tensors_and_bad_shapes(clib):
    import torch
    from clip_fsar_amd import shortlist_hip as sh
    i32 = dict(dtype=torch.int32)
    X, norms, out, slots = torch.zeros(5, 8, 64), torch.zeros(40), torch.zeros(5, 64), torch.zeros(2, **i32)
    with pytest.raises(RuntimeError, match="HIP device tensor"):
        sh.mean_unit_rows(X, norms, slots, out)
    for args in ((X, norms[:39], slots, out), (X, norms, slots, out[:4]), (X, norms, slots.view(1, 2), out)):
        with pytest.raises(RuntimeError, match="shape"):
            sh.mean_unit_rows(*args)
    U, C, cols, S = torch.zeros(3, 64), torch.zeros(7, 64), torch.zeros(5, **i32), torch.zeros(3, 5)
    with pytest.raises(RuntimeError, match="HIP device tensor"):
        sh.coarse_scores(U, C, cols, S)
    for args in ((U, C[:, :60], cols, S), (U, C, cols.view(5, 1), S), (U, C, cols, S[:, :4])):
        with pytest.raises(RuntimeError, match="shape"):
            sh.coarse_scores(*args)
    host = torch.tensor([[0, 2], [2, 1]], **i32)
    table = sh.Table(host, host, 2)
    sc, ss, work = torch.zeros(2, 4, **i32), torch.zeros(2, 4, **i32), torch.zeros(10)
    with pytest.raises(RuntimeError, match="HIP device tensor"):
        sh.select(S, cols, table, 4, sc, ss, work)
    for args in ((S, cols[:4], table, 4, sc, ss, work), (S, cols, table, 4, sc[:, :3], ss, work), (S, cols, table, 9, sc, ss, work),
                 (S, cols, table, 4, sc, ss[:1], work), (S, cols, table, 4, sc, ss, work[:9])):
        with pytest.raises(RuntimeError, match="shape"):
            sh.select(*args)
    with pytest.raises(RuntimeError, match="table must be a Table"):
        sh.select(S, cols, sh.Table(host[:, :1], host[:, :1], 2), 4, sc, ss, work)
    assert sh.table_rows([3, 0, 17, 1]) == (GOOD, 21)


# ------------------------------------------------------------------ the selection rule, on hand-written cases
def _sel(S, counts, keep):
    from clip_fsar_amd.shortlist import reference_select
    return reference_select(S, counts, keep)


def test_reference_select_ties_at_the_threshold():
    # scores 5 3 3 3 1 3: keep 3 takes the 5 and the first two of the four 3s, in column order
    assert _sel([[5.0, 3.0, 3.0, 3.0, 1.0, 3.0]], [1], 3) == [[0, 1, 2]]
    assert _sel([[3.0, 1.0, 3.0, 5.0, 3.0, 3.0]], [1], 3) == [[0, 2, 3]]
    assert _sel([[3.0, 1.0, 3.0, 5.0, 3.0, 3.0]], [1], 4) == [[0, 2, 3, 4]]
    assert _sel([[3.0, 1.0, 3.0, 5.0, 3.0, 3.0]], [1], 5) == [[0, 2, 3, 4, 5]]


def test_reference_select_both_zeros_compare_equal():
    assert _sel([[-0.0, 0.0, -0.0, 0.0]], [1], 2) == [[0, 1]]                  # a key that ranked +0.0 above -0.0 would give [1, 3]
    assert _sel([[0.0, -0.0, -1.0, 0.0]], [1], 2) == [[0, 1]]
    assert _sel([[-1e-45, -0.0, 1e-45, 0.0]], [1], 2) == [[1, 2]]             # the denormals beside them do differ


def test_reference_select_all_equal_rows():
    assert _sel([[2.5] * 7], [1], 3) == [[0, 1, 2]]
    assert _sel([[2.5] * 7, [2.5] * 7], [2], 7) == [list(range(7))]
    assert _sel([[-INF] * 4], [1], 2) == [[NONE, NONE]]


def test_reference_select_nan_and_minus_inf_are_never_selected():
    assert _sel([[NAN, 1.0, -INF, 2.0, NAN]], [1], 4) == [[1, 3, NONE, NONE]]
    assert _sel([[NAN, -3e38, -INF, INF]], [1], 2) == [[1, 3]]                # the most negative float and +inf are scores like others
    assert _sel([[NAN, NAN]], [1], 1) == [[NONE]]


def test_reference_select_keep_at_least_nc():
    S = [[1.0, 3.0, 2.0]]
    assert _sel(S, [1], 3) == _sel(S, [1], 8) == _sel(S, [1], 4096) == [[0, 1, 2]]          # K = NC: every column, in column order


def test_reference_select_fewer_selectable_columns_than_k():
    assert _sel([[NAN, 4.0, NAN, -INF, 1.0, NAN]], [1], 4) == [[1, 4, NONE, NONE]]          # the padding is at the end


def test_reference_select_a_group_without_clips():
    assert _sel([[1.0, 2.0], [4.0, 3.0]], [1, 0, 1, 0], 1) == [[1], [NONE], [0], [NONE]]
    assert _sel([], [0], 3) == [[]]                                                           # no rows: no columns either
    with pytest.raises(ValueError, match="add up to"):
        _sel([[1.0]], [2], 1)


def test_reference_select_max_over_a_group_ignores_nan():
    S = [[NAN, 1.0, 5.0, NAN],
         [7.0, NAN, 2.0, NAN],
         [0.0, NAN, 9.0, 8.0]]
    assert _sel(S, [2, 1], 2) == [[0, 2], [2, 3]]                              # group 0: scores 7, 1, 5, none; group 1: 0, none, 9, 8
    assert _sel(S, [3], 3) == [[0, 2, 3]]                                      # 7, 1, 9, 8
    assert _sel(S, [1, 1, 1], 4) == [[1, 2, NONE, NONE], [0, 2, NONE, NONE], [0, 2, 3, NONE]]


# ------------------------------------------------------------------ the bound, pinned to the reference and not to the kernels
@pytest.mark.parametrize("family", ["gauss", "near", "scale"])
def test_the_reference_in_float32_stays_inside_the_bound(family):
    import torch
    from clip_fsar_amd.shortlist import TINY, reference_coarse, reference_mean_unit_rows
    worst = worst_row = 0.0
    for T in (1, 8, 32):
        for E in (4, 36, 512):
            Xq, qn = sequences(family, 65, T, E, seed=T * 1000 + E)
            P, pn = sequences(family, 65, T, E, seed=T * 1000 + E + 1)
            assert max(rho(Xq, qn), rho(P, pn)) <= 1.0005
            ref = reference_coarse(reference_mean_unit_rows(Xq, qn), reference_mean_unit_rows(P, pn))
            rows = []
            for X, d in ((Xq, qn), (P, pn)):                                    # the header's operation order, in fp32
                acc = torch.zeros(X.shape[0], E)
                for t in range(T):
                    acc = acc + X[:, t] / d.view(-1, T)[:, t:t + 1].clamp_min(TINY)
                rows.append(acc * (torch.tensor(1.0) / torch.tensor(float(T))))
            assert rows[0].dtype == torch.float32
            for row, (X, d) in zip(rows, ((Xq, qn), (P, pn))):                  # each mean row on its own, element by element
                over = (row.double() - reference_mean_unit_rows(X, d)).abs() / row_bound(X, d)
                worst_row = max(worst_row, float(over.max()))
                assert float(over.max()) <= 1.0, (family, T, E, float(over.max()))
            err = float((( rows[0] @ rows[1].T).double() - ref).abs().max())
            worst = max(worst, err / bound(T, E))
            assert err <= bound(T, E), (family, T, E, err, bound(T, E))
            if family == "near":
                assert float(ref.min()) > 0.97                                  # the sums of like-signed products
    print("%s: worst fp32-restatement err / bound %.2f, of a mean row's element %.2f" % (family, worst, worst_row))


# ------------------------------------------------------------------ slot_revision and the refresh bookkeeping, on a stub head
def _stub_head(T=4, n_test=16, **train):
    import torch
    engine = NS(arch={"embed": 8}, text_test=torch.zeros(n_test, 8))
    return NS(args=NS(TRAIN=NS(**train), DATA=NS(NUM_INPUT_FRAMES=T)), _get_engine=lambda dev: engine, _engine_key=("stub",),
              arch_name="stub", precision="fp32", depth=1)


def _host_gallery(monkeypatch, capacity=4):
    """a LiveGallery on the CPU whose device work is stubbed out: the kernels do nothing, the sequences are zeros, the store is host
    memory.  What remains is the host logic of every call -- the planning, _update_sequences' loop, _install."""
    import torch
    from clip_fsar_amd import live_gallery as lg
    g = lg.LiveGallery(_stub_head(), "cpu", capacity=capacity)
    monkeypatch.setattr(lg.lhip, "accumulate", lambda *a, **k: None)
    monkeypatch.setattr(lg.lhip, "slot_norms", lambda *a, **k: None)
    g._upload = lambda rows: rows
    g._context2_by_class = lambda eng, seqs, offs: seqs
    g._check_feats = lambda f: f

    def sequences_of(feats, ids_of_video, new_ids, trows):
        offs = [0]
        for c in new_ids:
            offs.append(offs[-1] + sum(1 for v in ids_of_video if v == c))
        return torch.zeros(feats.shape[0], g.T + 1, g.E), offs

    def ensure_store(cap):                        # _ensure_store without the event that guards the outgrown buffers
        old = g._store
        if old is None or g._store_cap() < cap:
            g._store = g._alloc(cap)
            for k, t in (old or {}).items():
                g._store[k][:t.shape[0]].copy_(t)
        return g._store

    g._sequences_of_features, g._ensure_store = sequences_of, ensure_store
    return g


def _revs(g):
    return [g.slot_revision(s) for s in range(g.capacity)]


def test_slot_revision_rises_when_a_slots_prototype_is_written(monkeypatch):
    import torch
    g = _host_gallery(monkeypatch)
    f = lambda n: torch.zeros(n, 4, 8)
    assert _revs(g) == [0, 0, 0, 0] and g._writes == 0                            # _writes: the gallery-wide count behind Shortlist's "no scan"
    assert g.add_classes_features(f(3), [0, 0, 1]) == [0, 1] and _revs(g) == [1, 1, 0, 0]
    gens = [g.slot_generation(s) for s in range(4)]
    assert g.add_shots_features(f(2), [1, 1]) == [3]                              # further shots: the generation stays, the revision moves
    assert _revs(g) == [1, 2, 0, 0] and [g.slot_generation(s) for s in range(4)] == gens and g._writes == 2
    g.remove_classes([0])                                                         # a removal writes no prototype
    assert _revs(g) == [1, 2, 0, 0] and g.slot_generation(0) == gens[0] + 1 and g._writes == 2
    assert g.add_classes_features(f(1), [2]) == [1] and g.slot_of(2) == 0         # the freed slot's next owner
    assert _revs(g) == [2, 2, 0, 0]
    assert g.add_classes_features(f(3), [3, 4, 5]) == [2, 3, 4]                   # a growth: 4 -> 6 slots, the old revisions stay
    assert g.capacity == 6 and [g.slot_of(c) for c in (3, 4, 5)] == [2, 3, 4] and _revs(g) == [2, 2, 1, 1, 1, 0]
    assert g.add_shots_features(f(3), [5, 1, 5]) == [3, 4] and _revs(g) == [2, 3, 1, 1, 2, 0]
    sd = g.state_dict()
    g.clear()                                                                     # every slot is renewed
    assert _revs(g) == [3, 4, 2, 2, 3, 1] and len(g) == 0 and g._writes == 6      # one per call that wrote, however many slots
    g.load_state_dict(sd)
    assert _revs(g) == [4, 5, 3, 3, 4, 2] and g.class_ids == [1, 2, 3, 4, 5]
    with pytest.raises(IndexError):
        g.slot_revision(6)


def test_refresh_recomputes_exactly_the_candidate_slots_whose_revision_moved(monkeypatch):
    import torch
    from clip_fsar_amd import shortlist as slm
    g = _host_gallery(monkeypatch)
    f = lambda n: torch.zeros(n, 4, 8)
    launches = []

    def mean_unit_rows(X, norms, slots, out):
        assert X is g._store["P"] and norms is g._store["pn"] and out.shape == (g._store_cap(), g.E)
        launches.append(slots.tolist())
        out[slots.long()] = float(len(launches))                                  # a mark: which launch wrote the row

    monkeypatch.setattr(slm.shhip, "mean_unit_rows", mean_unit_rows)
    g.add_classes_features(f(4), [0, 1, 2, 3])                                    # slots 0 .. 3
    sl = slm.Shortlist(g, keep=2)
    assert sl.stats == {"calls": 0, "refreshed": 0}
    pending = sl._stale([0, 2])                                                   # the host half: the list is uploaded, nothing launched
    assert launches == [] and sl._coarse is None and pending[2] == [0, 2] and pending[3].tolist() == [0, 2]
    assert sl._stale([0, 2])[2] == [0, 2]                                         # and nothing marked: a call that fails in between loses nothing
    sl._refresh(pending)                                                          # only the candidates: one launch over both
    sl._refresh(sl._stale([2, 0]))                                                # nothing moved: no launch
    assert launches == [[0, 2]] and sl.stats["refreshed"] == 2
    # no slot of the gallery written since, and the list that was clean last time (the same object, or an equal one): not even a scan
    sl._rev[0] = -1
    assert sl._stale([2, 0]) is None and sl._stale(sl._clean[0]) is None
    assert sl._stale([0, 2])[2] == [0]                                            # another list is scanned
    sl._rev[0] = g.slot_revision(0)
    sl._refresh(sl._stale([0, 1, 2, 3]))
    assert launches[1:] == [[1, 3]] and sl.stats["refreshed"] == 4
    g.add_shots_features(f(1), [2])                                               # further shots of one class
    sl._refresh(sl._stale([0, 1, 2, 3]))
    assert launches[2:] == [[2]] and sl.stats["refreshed"] == 5
    g.remove_classes([3])
    g.add_classes_features(f(1), [11])                                            # the freed slot's next owner
    assert g.slot_of(11) == 3
    sl._refresh(sl._stale([0, 1, 2, 3]))
    assert launches[3:] == [[3]] and sl.stats["refreshed"] == 6
    before = sl._coarse.clone()
    g.add_classes_features(f(2), [12, 13])                                        # a growth past capacity: the rows are copied, not recomputed
    assert g.capacity == 6
    sl._refresh(sl._stale([g.slot_of(c) for c in g.class_ids]))
    assert launches[4:] == [[4, 5]] and sl._coarse.shape[0] == 6 and torch.equal(sl._coarse[:4], before) and sl.stats["refreshed"] == 8
    g.clear()
    g.add_classes_features(f(1), [0])
    sl._refresh(sl._stale([0]))
    assert launches[5:] == [[0]] and sl.stats["refreshed"] == 9


# ------------------------------------------------------------------ every argument error, before the device is touched
def _registered(ids=(0, 1, 2), capacity=4, **train):
    from clip_fsar_amd import live_gallery as lg
    g = lg.LiveGallery(_stub_head(**train), "cpu", capacity=capacity)
    if ids:
        g._install(lg.plan_add(g._book, list(ids)).book)       # registered on the host alone: nothing below reaches the device
    return g


def _shape_check(g, feats):
    if feats.dim() != 3 or feats.shape[1] != g.T or feats.shape[2] != g.E:
        raise ValueError("%s: feats must be [N, T=%d, E=%d], got %s" % (g._name, g.T, g.E, tuple(feats.shape)))
    return feats


def test_shortlist_argument_errors_are_raised_before_the_device_is_touched():
    import torch
    from clip_fsar_amd.gallery import SupportGallery
    from clip_fsar_amd.live_text_gallery import LiveTextGallery
    from clip_fsar_amd.shortlist import Shortlist
    g = _registered()
    for keep in (0, -1, 4097, True, 2.0, "3", None):
        with pytest.raises(ValueError, match=r"Shortlist: keep must be an integer in \[1, 4096\]"):
            Shortlist(g, keep=keep)
    assert Shortlist(g).keep == 64 and Shortlist(g, keep=4096).keep == 4096 and Shortlist(g, 1).keep == 1
    with pytest.raises(ValueError, match="Shortlist: a LiveTextGallery is refused -- its softmaxes are defined over the listed classes"):
        Shortlist(LiveTextGallery(_stub_head(COMBINE=True), "cpu", capacity=4))
    for other in (SupportGallery(_stub_head(), "cpu"), "gallery", None):
        with pytest.raises(TypeError, match="Shortlist: needs a LiveGallery"):
            Shortlist(other)
    sl = Shortlist(g, keep=2)
    feats, vids = torch.zeros(3, 4, 8), torch.zeros(3, 4, 3, 8, 8)
    calls = (lambda **kw: sl.classify_features(feats, **kw), lambda **kw: sl.classify(vids, **kw),
             lambda **kw: sl.topk_features(feats, k=1, **kw), lambda **kw: sl.topk(vids, k=1, **kw))
    for call in calls:
        with pytest.raises(RuntimeError, match="must be a HIP device tensor"):
            call()
        with pytest.raises(ValueError, match=r"Shortlist: class 7 is not registered \(classes=\)"):
            call(classes=[0, 7])
        with pytest.raises(ValueError, match="Shortlist: a class appears twice in classes="):
            call(classes=[1, 0, 1])
        with pytest.raises(ValueError, match="Shortlist: classes= needs at least one class"):
            call(classes=[])
        for counts in ([], [2, -1, 2], [1.0, 2], [True, 2], ["3"]):
            with pytest.raises(ValueError, match="Shortlist: counts must be a non-empty list of integers >= 0"):
                call(counts=counts)
    with pytest.raises(RuntimeError, match="must be a HIP device tensor"):
        sl.coarse_features(feats)
    with pytest.raises(ValueError, match="class 'x' is not registered"):
        sl.coarse_features(feats, classes=["x"])
    # k: at most min(16, K), K = min(keep, number of candidates)
    for topk in (sl.topk_features, sl.topk):
        for k, kw in ((0, {}), (3, {}), (2, {"classes": [1]}), (True, {}), (1.0, {})):
            with pytest.raises(ValueError, match=r"Shortlist.topk: k must be in \[1, min\(16, K = \d+"):
                topk(feats, k=k, **kw)
    many = Shortlist(_registered(ids=range(40), capacity=64), keep=64)
    with pytest.raises(ValueError, match=r"k must be in \[1, min\(16, K = 40"):
        many.topk_features(feats, k=17)
    # the device check aside: what follows it, still before any launch
    g._check_feats = lambda f: _shape_check(g, f)
    for counts in ([1, 1], [4], [2, 0, 2], torch.tensor([1, 1])):
        with pytest.raises(ValueError, match=r"Shortlist: the groups' counts add up to \d, the call holds 3 clips"):
            sl.classify_features(feats, counts=counts)
    with pytest.raises(ValueError, match="Shortlist: 65537 groups, at most 65536 are scored per call"):
        sl.classify_features(feats, counts=[0] * 65534 + [1, 1, 1])
    with pytest.raises(ValueError, match="the call holds 0 clips"):
        sl.classify_features(feats[:0])
    with pytest.raises(ValueError, match=r"feats must be \[N, T=4, E=8\]"):
        sl.classify_features(torch.zeros(3, 5, 8))
    # an empty gallery, and a stale engine
    with pytest.raises(RuntimeError, match="Shortlist: no classes registered"):
        Shortlist(_registered(ids=())).classify_features(feats)
    g.head._engine_key = ("other",)
    with pytest.raises(RuntimeError, match="changed since these prototypes"):
        sl.classify_features(feats)
    g.head._engine_key = ("stub",)
    assert g._store is None and sl._coarse is None and sl._tables is None and sl.stats == {"calls": 0, "refreshed": 0}
