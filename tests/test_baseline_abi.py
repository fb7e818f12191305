"""CPU: adaptive baselines (libclipfsar_baseline.so, include/ext/clipfsar_baseline.h, clip_fsar_amd.baseline_hip, clip_fsar_amd.baseline)
-- the plug-in library's exports, ABI check at load, resource report and place in the build (a fourth, open registry,
build.PLUGIN_LIBS); the host validation of cfbl_normalize without a GPU; Baseline; reference_baseline on hand-written cases; StreamPool's
baseline= option on stub heads."""
import ctypes
import json
import os
import random
import re
import struct
from types import SimpleNamespace as NS

import pytest

import _abi
from _abi import check_abi_at_load, check_exports

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ext", "clipfsar_baseline.h")
KERNELS = {"baseline_kernel": 1}
ROW = _abi._row("baseline", "baseline_hip", "cfbl_", "ext/clipfsar_baseline.h", "version abi_version last_error normalize", KERNELS, 1)
INF, NAN = float("inf"), float("nan")


@pytest.fixture(scope="module")
def clib():
    import __graft_entry__ as ge
    ge.build()                                    # builds every library (no-op when up to date)
    from clip_fsar_amd import baseline_hip
    return baseline_hip.lib()


def _f32(v):
    return struct.unpack("f", struct.pack("f", v))[0]


def _bits(values):
    """fp32 bit patterns: NaN-proof, sign-of-zero-proof equality"""
    return [struct.pack("f", v) for v in values]


# ------------------------------------------------------------------ the library and its place in the build
def test_header_exported_exactly_and_arity_matches(clib):
    check_exports(ROW)
    assert ROW.exports == {"cfbl_version", "cfbl_abi_version", "cfbl_last_error", "cfbl_normalize"}
    from clip_fsar_amd import baseline as bl
    from clip_fsar_amd import baseline_hip as bh
    from clip_fsar_amd import class_smooth_hip as ch
    text = open(HEADER).read()
    smooth = open(os.path.join(ROOT, "include", "ext", "clipfsar_class_smooth.h")).read()
    for name in ("MAX_STREAMS", "CHUNK", "TABLE_COLS", "SLOT", "NW", "OUT0", "NC", "KEY0", "CHUNK0"):       # the table is CFCS_*'s, redeclared
        mine = int(re.search(r"#define CFBL_%s (\d+)" % name, text).group(1))
        assert mine == int(re.search(r"#define CFCS_%s (\d+)" % name, smooth).group(1)) == getattr(bh, name) == getattr(ch, name), name
    assert int(re.search(r"#define CFBL_MAX_WARMUP (\d+)", text).group(1)) == bh.MAX_WARMUP == bl.MAX_WARMUP == 1 << 20
    assert bh.plan_rows is ch.plan_rows and bh.MAX_CELLS == ch.MAX_CELLS == (1 << 31) - 1
    assert len(bh.SIGNATURES["cfbl_normalize"]) == 21
    for other in _abi.LIBS:                       # its prefix hides no other library's, and none hides it
        assert not other.prefix.startswith(ROW.prefix) and not ROW.prefix.startswith(other.prefix), other.name
    for prefix in ("cfcs_", "cfev_"):
        assert not prefix.startswith(ROW.prefix) and not ROW.prefix.startswith(prefix)


def test_abi_version_is_checked_at_load(clib, monkeypatch):
    check_abi_at_load(ROW, monkeypatch)


def test_the_kernel_is_the_listed_one_and_uses_no_scratch(clib):
    from clip_fsar_amd import baseline_hip as bh
    from clip_fsar_amd import build as b
    pl = b.PLUGIN_LIBS["baseline"]
    if not os.path.exists(pl.usage):
        b.build_plugin("baseline", force=True, verbose=False)
    usage = json.load(open(pl.usage))
    assert len(usage) == ROW.total == 1, sorted(usage)
    for fragment, count in KERNELS.items():
        assert sum(fragment in n for n in usage) == count, (fragment, sorted(usage))
    for n, u in usage.items():
        assert u.get("scratch", 0) == 0 and u.get("spills", 0) == 0, (n, u)
    assert os.path.normpath(pl.usage).endswith(os.path.join("build", "baseline", "resource_usage.json"))
    assert pl.lib == bh.LIB_PATH and pl.lib.endswith(os.sep + "libclipfsar_baseline.so") and os.path.exists(pl.lib)
    assert os.path.normpath(pl.source).endswith(os.path.join("clip-fsar_amd", "ext", "baseline.hip")) and pl.header == HEADER
    others = [b.USAGE] + [x.usage for reg in (b.SIDE_LIBS, b.EXT_LIBS, b.ADDON_LIBS) for x in reg.values()]
    others += [x.usage for n, x in b.PLUGIN_LIBS.items() if n != "baseline"]
    for path in others:                           # and no other library's report names it
        names = json.load(open(path))
        assert not any(fragment in n for n in names for fragment in KERNELS), path
    source = open(pl.source).read()               # plain C++ on the shared error plumbing: no assembly, no allocation, no stream, no atomics, no LDS
    assert '#include "../csrc/side_lib.h"' in source and '#include "../../include/ext/clipfsar_baseline.h"' in source
    assert '#include "chunk_row.h"' in source and os.path.exists(os.path.join(b.EXT, "chunk_row.h"))
    for body in ("asm", "thread_local", "calloc", "hipMalloc", "hipStreamCreate", "atomic", "__builtin_amdgcn", "__shared__", "fmaf", "fma("):
        assert body not in source, body
    for op in ("__fsub_rn", "__fmul_rn", "__fdiv_rn", "contract(off)"):
        assert op in source, op


def test_the_fourth_registry_is_open():
    from clip_fsar_amd import build as b
    assert "baseline" in b.PLUGIN_LIBS and list(b.PLUGIN_LIBS) == b.plugin_lib_names()
    assert all(b.PLUGIN_LIBS is not reg and not set(b.PLUGIN_LIBS) & set(reg) for reg in (b.SIDE_LIBS, b.EXT_LIBS, b.ADDON_LIBS))
    assert all(isinstance(v, b.ExtLib) for v in b.PLUGIN_LIBS.values())
    for name, pl in b.PLUGIN_LIBS.items():        # the recipe, for every name there is and will be
        assert pl.source == os.path.join(b.EXT, name + ".hip") and os.path.exists(pl.source), name
        assert pl.header == os.path.join(ROOT, "include", "ext", "clipfsar_%s.h" % name) and os.path.exists(pl.header), name
        assert pl.lib == os.path.join(b.HERE, "libclipfsar_%s.so" % name), name
        assert pl.usage == os.path.join(b.HERE, "build", name, "resource_usage.json"), name
        assert pl.source in b._plugin_deps(name) and pl.header in b._plugin_deps(name) and os.path.abspath(b.__file__) in b._plugin_deps(name)
    for call in (b._plugin_deps, b.build_plugin):
        for foreign in ("pool", "class_smooth", "events"):
            with pytest.raises(KeyError):
                call(foreign)
    for call in (b.build_side, b._side_deps, b.build_ext, b._ext_deps, b.build_addon, b._addon_deps):       # the three older registries
        with pytest.raises(KeyError):
            call("baseline")
    assert not os.path.exists(os.path.join(b.CSRC, "baseline.hip")) and not os.path.exists(os.path.join(b.CSRC, "chunk_row.h"))
    text = open(b.__file__).read()
    assert "PLUGIN_LIBS" in text and "OPEN" in text
    order = [text.index("build_%s(name, force=force" % tier) for tier in ("side", "ext", "addon", "plugin")]
    assert order == sorted(order)                 # built after the add-ons


def test_staleness_of_the_plug_in_and_of_nothing_else(monkeypatch):
    from clip_fsar_amd import build as b
    from test_build_recipe import NAMES, STALE, P
    monkeypatch.setattr(b.os.path, "exists", lambda p: True)

    def stale_after(edited):
        monkeypatch.setattr(b.os.path, "getmtime", lambda p: 2.0 if p.endswith(os.sep + edited) else 1.0)
        old = {P} if b._stale(b.LIB, b._product_deps()) else set()
        old |= {n for n in NAMES if b._stale(b.SIDE_LIBS[n].lib, b._side_deps(n))}
        old |= {n for n in b.EXT_LIBS if b._stale(b.EXT_LIBS[n].lib, b._ext_deps(n))}
        old |= {n for n in b.ADDON_LIBS if b._stale(b.ADDON_LIBS[n].lib, b._addon_deps(n))}
        return old, b._stale(b.PLUGIN_LIBS["baseline"].lib, b._plugin_deps("baseline"))

    for edited in ("baseline.hip", "clipfsar_baseline.h", "chunk_row.h"):         # the plug-in's own files: it alone
        assert stale_after(edited) == (set(), True), edited
    for edited in ("side_lib.h", "build.py", "common.h", "ring_rows.h"):          # shared: the others as their matrix has it
        assert stale_after(edited) == (STALE[edited] | {"class_smooth", "events"}, True), edited
    for edited in ("pool.hip", "clipfsar_pool.h", "otam_tile.h", "gemm.hip"):
        assert stale_after(edited) == (STALE[edited], False), edited
    for edited, whose in (("class_smooth.hip", "class_smooth"), ("clipfsar_class_smooth.h", "class_smooth"), ("events.hip", "events"),
                          ("clipfsar_events.h", "events")):                       # the older tiers' own files leave the plug-in alone
        assert stale_after(edited) == ({whose}, False), edited
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
    err, good = clib.cfbl_last_error, _tbl(GOOD)
    # normalize(scores, mean, dev, count, marks, gens, keys, out, table_host, table_dev,
    #           S, NOUT, NKEYS, max_streams, cap, rate, warm_rate, warmup, gate, floor, stream)

    def call(t, S=3, nout=NOUT, nkeys=NKEYS, ms=4, cap=300, rate=1 / 32, warm_rate=0.25, warmup=16, gate=3.0, floor=1e-6):
        return clib.cfbl_normalize(p, p, p, p, p, p, p, p, t, p, S, nout, nkeys, ms, cap, rate, warm_rate, warmup, gate, floor, None)

    for i in range(10):
        args = [p] * 8 + [good, p]
        args[i] = None
        assert clib.cfbl_normalize(*args, 3, NOUT, NKEYS, 4, 300, 1 / 32, 0.25, 16, 3.0, 1e-6, None) != 0 and b"null" in err(), i
    for rate in (0.0, 1.0, -0.5, 1.5, NAN, INF):
        assert call(good, rate=rate) != 0 and b" rate=" in err(), rate
    for warm_rate in (0.0, -0.25, 1.0000001, NAN, INF):
        assert call(good, warm_rate=warm_rate) != 0 and b"warm_rate=" in err(), warm_rate
    for warmup in (0, -3, (1 << 20) + 1):
        assert call(good, warmup=warmup) != 0 and b"warmup=" in err(), warmup
    for gate in (0.0, -1.0, NAN, -INF):
        assert call(good, gate=gate) != 0 and b"gate=" in err(), gate
    for floor in (0.0, -1e-6, NAN, INF):
        assert call(good, floor=floor) != 0 and b"floor=" in err(), floor
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
    # a table without a window is valid and launches nothing; so are the parameters' edges: warm_rate 1, warmup 1 and 2^20, gate +inf
    empty = _tbl([[3, 0, 0, 7, 0, 0]])
    assert call(empty, S=1, nout=0, nkeys=7) == 0, err()
    assert call(empty, S=1, nout=0, nkeys=7, warm_rate=1.0, warmup=1, gate=INF, floor=1e-30) == 0, err()
    assert call(empty, S=1, nout=0, nkeys=7, warmup=1 << 20, rate=0.999, gate=1e-30) == 0, err()


def test_python_wrapper_rejects_cpu_tensors_and_bad_shapes(clib):
    import torch
    from clip_fsar_amd import baseline_hip as bh
    host = torch.tensor(GOOD, dtype=torch.int32)
    table = bh.Table(host, host, 3)
    i32 = dict(dtype=torch.int32)
    x, mean, dev, cnt, mk = torch.zeros(NOUT), torch.zeros(4, 300), torch.zeros(4, 300), torch.zeros(4, 300, **i32), torch.zeros(4, 300, **i32)
    gens, keys, out = torch.ones(300, **i32), torch.zeros(NKEYS, **i32), torch.zeros(NOUT)
    good = [x, mean, dev, cnt, mk, gens, keys, out]
    rule = (1 / 32, 0.25, 16, 3.0, 1e-6)
    with pytest.raises(RuntimeError, match="HIP device tensor"):
        bh.normalize(*good, table, *rule)
    for at, bad in ((0, x.view(2, -1)), (2, dev[:3]), (3, cnt[:, :299]), (4, mk[:3]), (5, gens[:299]), (6, keys.view(1, -1)), (7, out[:-1])):
        args = list(good)
        args[at] = bad
        with pytest.raises(RuntimeError, match="shape|flat"):
            bh.normalize(*args, table, *rule)
    with pytest.raises(RuntimeError, match="table must be a Table"):
        bh.normalize(*good, bh.Table(host[:, :5], host[:, :5], 3), *rule)


# ------------------------------------------------------------------ the parameters and the reference
def test_baseline_errors_name_the_field():
    from clip_fsar_amd.baseline import Baseline
    b = Baseline()
    assert b == (1 / 32, 0.25, 16, 3.0, 1e-6) and b._fields == ("rate", "warm_rate", "warmup", "gate", "floor")
    assert Baseline(rate=0.5, warm_rate=1, warmup=1, gate=INF, floor=1) == (0.5, 1.0, 1, INF, 1.0)
    assert Baseline(gate=1e39).gate == 1e39       # +inf as fp32: allowed
    for kw, field in (({"rate": 0}, "rate"), ({"rate": 1}, "rate"), ({"rate": 1 - 1e-9}, "rate"), ({"rate": 1e-46}, "rate"),
                      ({"rate": NAN}, "rate"), ({"rate": "0.1"}, "rate"), ({"rate": True}, "rate"), ({"warm_rate": 0}, "warm_rate"),
                      ({"warm_rate": 1.001}, "warm_rate"), ({"warm_rate": NAN}, "warm_rate"), ({"warm_rate": None}, "warm_rate"),
                      ({"warmup": 0}, "warmup"), ({"warmup": 8.0}, "warmup"), ({"warmup": True}, "warmup"),
                      ({"warmup": (1 << 20) + 1}, "warmup"), ({"gate": 0}, "gate"), ({"gate": -3.0}, "gate"), ({"gate": NAN}, "gate"),
                      ({"gate": 1e-46}, "gate"), ({"floor": 0}, "floor"), ({"floor": -1e-6}, "floor"), ({"floor": INF}, "floor"),
                      ({"floor": 1e39}, "floor"), ({"floor": 1e-46}, "floor"), ({"floor": NAN}, "floor")):
        with pytest.raises(ValueError, match="Baseline: %s " % field):
            Baseline(**kw)


def _ref(scores, rule, cell=None):
    from clip_fsar_amd.baseline import reference_baseline
    z, cell = reference_baseline(scores, rule, cell)
    return z, tuple(cell)


def test_reference_baseline_on_hand_written_cases():
    from clip_fsar_amd.baseline import Baseline, Cell
    rule = Baseline(rate=0.25, warm_rate=0.5, warmup=3, gate=3.0, floor=0.125)
    # warm-up: exactly `warmup` windows without a deviation; window 0 sets the mean, windows 1 and 2 fold at warm_rate
    z, cell = _ref([4.0, 8.0, 4.0, 6.0], rule)
    assert all(v != v for v in z[:3]) and len(z) == 4
    # after 4, 8: m = 6, d = 0.5 * 0 + 0.5 * 4 = 2; after 4: a = 2, m = 5, d = 2; window 3: z = (6 - 5) / 2, not gated: a = 1, m = 5.25, d = 1.75
    assert z[3] == 0.5 and cell == (5.25, 1.75, 3)
    for warmup in (1, 2, 5):
        z, cell = _ref([1.0] * 7, Baseline(warmup=warmup))
        assert [v != v for v in z] == [True] * warmup + [False] * (7 - warmup) and cell[2] == warmup
    # a gated window leaves the cell's bits unchanged, and gets its z all the same; the next window is judged against the same cell
    z, cell = _ref([100.0, 5.25], rule, Cell(5.25, 1.75, 3))
    assert z[0] == _f32((100.0 - 5.25) / 1.75) and z[0] >= rule.gate and z[1] == 0.0
    assert _bits(cell[:2]) == _bits([_f32(0.75 * 5.25 + 0.25 * 5.25), _f32(0.75 * 1.75)]) and cell[2] == 3
    z, cell = _ref([100.0], rule, Cell(5.25, 1.75, 3))
    assert _bits(cell[:2]) == _bits((5.25, 1.75)) and cell[2] == 3
    # z == gate is gated; just below is folded in; gate = +inf gates nothing; a large negative z is never gated
    assert _ref([5.25 + 3 * 1.75], rule, Cell(5.25, 1.75, 3))[1] == (5.25, 1.75, 3)
    assert _ref([5.25 + 2.5 * 1.75], rule, Cell(5.25, 1.75, 3))[1] != (5.25, 1.75, 3)
    assert _ref([100.0], rule._replace(gate=INF), Cell(5.25, 1.75, 3))[1] != (5.25, 1.75, 3)
    z, cell = _ref([-100.0], rule, Cell(5.25, 1.75, 3))
    assert z[0] < -50 and cell != (5.25, 1.75, 3)
    # floor is taken when d == 0 (a constant series), and when d lies below it
    z, cell = _ref([2.0, 2.0, 2.0, 2.25, 2.0], rule)
    assert z[3] == 0.25 / 0.125 and cell[0] == _f32(0.75 * _f32(0.75 * 2.0 + 0.25 * 2.25) + 0.25 * 2.0)
    assert z[4] == (2.0 - 2.0625) / 0.125         # d = 0.0625, still below the floor
    # non-finite scores: z = NaN, the cell is untouched -- before the first window, in warm-up and after it
    for bad in (NAN, INF, -INF):
        z, cell = _ref([bad, 4.0, bad, 8.0, 4.0, bad, 6.0, bad], rule)
        assert [v != v for v in z] == [True] * 6 + [False, True] and z[6] == 0.5 and cell == (5.25, 1.75, 3), bad
    # every operation is rounded to fp32: 0.1 folds as fp32(0.1), and the result differs from the double computation
    rule = Baseline(rate=0.1, warm_rate=0.3, warmup=2, gate=3.0, floor=1e-6)
    z, cell = _ref([0.1, 0.7, 0.2], rule)
    f = _f32
    keep, r = f(1.0 - f(0.3)), f(0.3)
    a = abs(f(f(0.7) - f(0.1)))
    m = f(f(keep * f(0.1)) + f(r * f(0.7)))
    d = f(f(keep * 0.0) + f(r * a))
    assert _bits(z[2:]) == _bits([f(f(f(0.2) - m) / d)])
    assert _ref([], rule) == ([], (0.0, 0.0, 0)) and _ref([], rule, Cell(1.5, 0.5, 2)) == ([], (1.5, 0.5, 2))


def _series(rng, mu, sigma, n=12, event=(5, 8)):
    """an N(mu, sigma) series with a plateau of +8 sigma over `event`, as fp32 values"""
    return [_f32(rng.gauss(mu, sigma) + (8 * sigma if event[0] <= k < event[1] else 0.0)) for k in range(n)]


def test_reference_baseline_does_not_depend_on_the_split():
    """12 windows as one call, as 12 calls and as 5 + 0 + 7, on the three scales of the pool's scores; the series gate some windows and
    fold others after warm-up, so the split is tested on every branch"""
    from clip_fsar_amd.baseline import Baseline
    rng = random.Random(3)
    rule = Baseline(rate=1 / 16, warm_rate=0.25, warmup=4, gate=3.0, floor=1e-6)
    gated = folded = 0
    for mu, sigma in ((-8.0, 0.5), (0.02, 0.004), (-40.0, 3.0)):
        for _ in range(40):
            col = _series(rng, mu, sigma)
            whole, cell = _ref(col, rule)
            for cuts in ((12,), tuple(range(1, 13)), (5, 5, 12)):
                got, c, k0 = [], None, 0
                for k1 in cuts:
                    part, c = _ref(col[k0:k1], rule, c)
                    got += part
                    k0 = k1
                assert _bits(got) == _bits(whole) and _bits(c[:2]) == _bits(cell[:2]) and c[2] == cell[2], cuts
            gated += sum(v >= rule.gate for v in whole)
            folded += sum(v < rule.gate for v in whole)
    assert gated >= 100 and folded >= 300, (gated, folded)


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


def test_the_baseline_option_on_stub_heads():
    import inspect
    from clip_fsar_amd import pool as pm
    from clip_fsar_amd.baseline import Baseline
    from clip_fsar_amd.events import EventRule
    from clip_fsar_amd.gallery import SupportGallery
    from clip_fsar_amd.pool import StreamPool
    from clip_fsar_amd.stream import StreamOutput
    from clip_fsar_amd.text_gallery import TextGallery
    params = list(inspect.signature(StreamPool.__init__).parameters)
    assert params[-2:] == ["events", "baseline"]                      # a new LAST keyword
    base, rule = Baseline(), EventRule(4, 2, 2, 2)
    live = _live("live", 4)
    p = StreamPool(live, max_streams=3, smooth=0.5, smooth_by="class", events=rule, baseline=base)       # TypeError without the feature
    h = p.open()
    assert p.baseline(h) == [] and p._bl_cells.forgotten == {0} == p._ev_cells.forgotten == p._smooth_cells.forgotten
    p.reset(h)
    assert p._bl_cells.forgotten == {0}
    q = StreamPool(_live("live_text", 4), baseline=base)              # no smoothing, no rule: the logits' deviations alone
    assert q._by_class is False and q._events is None and q._keyed and q.baseline(q.open()) == []
    assert StreamPool(live, smooth=0.0, smooth_by="column", baseline=base)._keyed
    plain = StreamPool(live, smooth=0.5, smooth_by="class", events=rule)
    assert not hasattr(plain, "_bl_cells") and plain._baseline is None
    assert not StreamPool(live)._keyed
    with pytest.raises(ValueError, match="keeps no baselines"):
        plain.baseline(plain.open())
    for g in (SupportGallery(_stub_head(), "cpu"), TextGallery(_stub_head(COMBINE=True), "cpu")):
        with pytest.raises(ValueError, match="baseline=.*slot store.*%s" % type(g).__name__):
            StreamPool(g, baseline=base)
    for smooth_by in ({}, {"smooth_by": "column"}):
        with pytest.raises(ValueError, match="baseline=.*smooth > 0.*smooth_by=\"class\""):
            StreamPool(live, smooth=0.5, baseline=base, **smooth_by)
    with pytest.raises(ValueError, match="baseline= keeps a state cell.*2\\^31"):
        StreamPool(_live("live", 1 << 15), max_streams=1 << 16, baseline=base)
    for bad in ((1 / 32, 0.25, 16, 3.0, 1e-6), "base", 1, {"rate": 0.1}, rule):
        with pytest.raises(TypeError, match="Baseline"):
            StreamPool(live, baseline=bad)
    with pytest.raises(ValueError, match="session 99 is not open"):
        p.baseline(99)
    # the output types: a pool without the option returns the plain ones; the subclasses keep the pinned tuples and add one attribute
    for plain_type, mine in ((pm.PackedOutput, pm.DeviationPackedOutput), (pm.GroupedPackedOutput, pm.DeviationGroupedPackedOutput),
                             (StreamOutput, pm.DeviationStreamOutput)):
        assert issubclass(mine, plain_type) and mine is not plain_type and mine._fields == plain_type._fields
        fields = tuple(range(len(plain_type._fields)))
        out = mine(*fields, deviation="z")
        assert tuple(out) == fields == tuple(plain_type(*fields)) and out == plain_type(*fields) and out.deviation == "z"
        assert not hasattr(plain_type(*fields), "deviation")
    po = pm.PackedOutput([7, 8], [0, 3], [0, 2, 3], list("abc"), None)
    split = StreamPool._split(po)
    assert all(type(o) is StreamOutput for o in split.values()) and split[8] == (3, ["c"], None)
    split = StreamPool._split(pm.DeviationPackedOutput(*po, deviation=list("xyz")))
    assert all(type(o) is pm.DeviationStreamOutput for o in split.values())
    assert split[7] == (0, ["a", "b"], None) and split[7].deviation == ["x", "y"] and split[8].deviation == ["z"]
