"""CPU: tempo windows (libclipfsar_tempo.so, include/ext/clipfsar_tempo.h, clip_fsar_amd.tempo_hip, StreamPool(rates=...)) -- the plug-in
library's exports, ABI check at load, resource report and place in the build (one more name of the open registry, build.PLUGIN_LIBS);
every host validation of cftp_window_sequences and cftp_reduce without a GPU, the table refusals word for word cfsp_window_sequences's;
tempo_positions against a brute-force ring; reference_reduce on hand-written cases; every refusal of StreamPool(rates=...) and of
tempo= on stub heads."""
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
HEADER = os.path.join(ROOT, "include", "ext", "clipfsar_tempo.h")
KERNELS = {"tempo_gather_kernel": 2, "tempo_reduce_kernel": 2}                   # each in its 16-byte and its 4-byte form
ROW = _abi._row("tempo", "tempo_hip", "cftp_", "ext/clipfsar_tempo.h", "version abi_version last_error window_sequences reduce", KERNELS, 4)
INF, NAN = float("inf"), float("nan")


@pytest.fixture(scope="module")
def clib():
    import __graft_entry__ as ge
    ge.build()                                    # builds every library (no-op when up to date)
    from clip_fsar_amd import tempo_hip
    return tempo_hip.lib()


# ------------------------------------------------------------------ the library and its place in the build
def test_header_exported_exactly_and_arity_matches(clib):
    check_exports(ROW)
    assert ROW.exports == {"cftp_" + e for e in ("version", "abi_version", "last_error", "window_sequences", "reduce")}
    from clip_fsar_amd import tempo_hip as th
    text = open(HEADER).read()
    assert int(re.search(r"#define CFTP_MAX_RATES (\d+)", text).group(1)) == th.MAX_RATES == 8
    assert [len(th.SIGNATURES["cftp_" + e]) for e in ("window_sequences", "reduce")] == [16, 7]
    for other in _abi.LIBS:                       # its prefix hides no other library's, and none hides it
        assert not other.prefix.startswith(ROW.prefix) and not ROW.prefix.startswith(other.prefix), other.name
    for prefix in ("cfcs_", "cfev_", "cfbl_", "cfsh_", "cfps_", "cfal_"):
        assert not prefix.startswith(ROW.prefix) and not ROW.prefix.startswith(prefix)


def test_abi_version_is_checked_at_load(clib, monkeypatch):
    check_abi_at_load(ROW, monkeypatch)


def test_the_kernels_are_the_listed_ones_and_use_no_scratch(clib):
    from clip_fsar_amd import build as b
    from clip_fsar_amd import tempo_hip as th
    pl = b.PLUGIN_LIBS["tempo"]
    if not os.path.exists(pl.usage):
        b.build_plugin("tempo", force=True, verbose=False)
    usage = json.load(open(pl.usage))
    assert len(usage) == ROW.total == sum(KERNELS.values()), sorted(usage)
    for fragment, count in KERNELS.items():
        assert sum(fragment in n for n in usage) == count, (fragment, sorted(usage))
    for n, u in usage.items():
        assert u.get("scratch", 0) == 0 and u.get("spills", 0) == 0, (n, u)
    assert pl.lib == th.LIB_PATH and pl.lib.endswith(os.sep + "libclipfsar_tempo.so") and os.path.exists(pl.lib)
    others = [b.USAGE] + [x.usage for reg in (b.SIDE_LIBS, b.EXT_LIBS, b.ADDON_LIBS) for x in reg.values()]
    others += [x.usage for n, x in b.PLUGIN_LIBS.items() if n != "tempo"]
    for path in others:                           # no other library's report names them, and they carry no other library's fragment
        if os.path.exists(path):
            assert not any(fragment in n for n in json.load(open(path)) for fragment in KERNELS), path
    import test_align_abi, test_baseline_abi, test_events_abi, test_pool_select_abi, test_shortlist_abi
    claimed = [f for row in _abi.SIDE for f in row.kernels]
    claimed += [f for mod in (test_align_abi, test_baseline_abi, test_events_abi, test_pool_select_abi, test_shortlist_abi) for f in mod.KERNELS]
    for n in usage:
        assert not any(f in n for f in claimed), n
    # the conventions: the ring libraries' row pieces, the shared error plumbing, the pool's table columns and its own header -- nothing
    # else; plain C++, no allocation, no copy or wait of its own
    source = open(pl.source).read()
    assert re.findall(r'^#include [<"]([^>"]+)[>"]', source, flags=re.M) == ["../csrc/ring_rows.h", "../csrc/side_lib.h",
                                                                            "../../include/clipfsar_pool.h",
                                                                            "../../include/ext/clipfsar_tempo.h"]
    for body in ("asm", "atomic", "malloc", "hipMalloc", "hipMemcpy", "hipDeviceSynchronize", "__shared__", "__syncthreads"):
        assert body not in source, body
    for shared in ("Piece<VEC>", "vec_ok(", "blocks_for(", "MAX_ITEMS", "SIDE_REQUIRE(", "check_launch(", "CFSP_WIN_OFF", "CFSP_MAX_T"):
        assert shared in source, shared
    assert "RESTATED" in source and "pool.hip" in source             # find_row and the table check: said so where they are restated
    assert "rates_dev" not in source and "Rates rates" in source     # the rates travel by value


def test_tempo_is_a_name_of_the_open_registry_and_follows_the_recipe():
    from clip_fsar_amd import build as b
    assert "tempo" in b.PLUGIN_LIBS and "tempo" in b.plugin_lib_names()
    assert all("tempo" not in reg for reg in (b.SIDE_LIBS, b.EXT_LIBS, b.ADDON_LIBS))
    pl = b.PLUGIN_LIBS["tempo"]
    assert isinstance(pl, b.ExtLib)
    assert pl.source == os.path.join(b.EXT, "tempo.hip") and os.path.exists(pl.source)
    assert pl.header == HEADER and os.path.exists(pl.header)
    assert pl.lib == os.path.join(b.HERE, "libclipfsar_tempo.so")
    assert pl.usage == os.path.join(b.HERE, "build", "tempo", "resource_usage.json")
    deps = b._plugin_deps("tempo")
    assert sorted(deps) == sorted([pl.source, pl.header, os.path.abspath(b.__file__), os.path.join(b.CSRC, "ring_rows.h"),
                                   os.path.join(b.CSRC, "side_lib.h"), os.path.join(b.CSRC, "common.h"),
                                   os.path.join(ROOT, "include", "clipfsar_pool.h"), os.path.join(ROOT, "include", "clipfsar_hip.h")])
    for call in (b.build_side, b._side_deps, b.build_ext, b._ext_deps, b.build_addon, b._addon_deps):       # the three closed registries
        with pytest.raises(KeyError):
            call("tempo")
    assert not os.path.exists(os.path.join(b.CSRC, "tempo.hip"))
    assert not any("clipfsar_tempo" in open(os.path.join(b.CSRC, f)).read() for f in os.listdir(b.CSRC))    # nothing of csrc/ knows it


def test_staleness_of_the_tempo_library_and_of_no_other(monkeypatch):
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

    for edited in ("tempo.hip", "clipfsar_tempo.h"):                              # its own files: it alone
        assert stale_after(edited) == (set(), {"tempo"}), edited
    assert stale_after("clipfsar_pool.h") == (STALE["clipfsar_pool.h"], {"tempo"})     # the table's columns: the pool's users and it
    old, plugins = stale_after("ring_rows.h")                                     # the row pieces: the ring libraries, the recurrence's users
    assert STALE["ring_rows.h"] <= old and "tempo" in plugins and "align" not in plugins
    for edited in ("side_lib.h", "build.py", "common.h"):                         # what every library reaches
        old, plugins = stale_after(edited)
        assert STALE[edited] <= old and plugins == set(b.PLUGIN_LIBS), edited
    for edited in ("pool.hip", "select_keys.h", "chunk_row.h", "otam_tile.h", "otam_dp.h", "fp32_tile_gemm.h", "align.hip", "gemm.hip"):
        assert "tempo" not in stale_after(edited)[1], edited
    assert stale_after("no_such_file.h") == (set(), set())


# ------------------------------------------------------------------ validation, without a GPU
def _tbl(rows):
    flat = [v for r in rows for v in r]
    return (ctypes.c_int32 * len(flat))(*flat)


def _rates(*r):
    return (ctypes.c_int32 * max(1, len(r)))(*r)


#        slot put_pos n feat_off win_pos nW win_off has_state
GOOD = [[2, 5, 3, 0, 1, 1, 0, 0],
        [0, 0, 4, 3, 0, 0, 1, 0],
        [1, 9, 2, 7, 6, 2, 1, 1]]               # N = 9, NW = 3; cap 16, max_streams 4 (tests/test_pool_abi.py's table)


def _edit(row, col, value):
    rows = [list(r) for r in GOOD]
    rows[row][col] = value
    return _tbl(rows)


def test_window_sequences_validation_without_gpu(clib):
    from clip_fsar_amd import pool_hip
    p = ctypes.c_void_p(4096)                     # never dereferenced: every call below fails validation before any device work
    err, good, r12 = clib.cftp_last_error, _tbl(GOOD), _rates(1, 2)
    pool, pool_err = pool_hip.lib().cfsp_window_sequences, pool_hip.lib().cfsp_last_error

    # window_sequences(ring, X, table_host, table_dev, S, NW, w0, w1, T, E, max_streams, cap, stride, rates_host, R, stream)
    def call(ptrs=None, S=3, NW=3, w0=0, w1=3, T=4, E=64, ms=4, cap=16, stride=2, rates=r12, R=2):
        a = ptrs or [p, p, good, p]
        return clib.cftp_window_sequences(*a, S, NW, w0, w1, T, E, ms, cap, stride, rates, R, None)

    def same_words_as_the_pool(table=good, **kw):
        """the refusal of cfsp_window_sequences on the same arguments (rate = 2, this call's rmax), and the same words after the name"""
        a = dict(S=3, NW=3, w0=0, w1=3, T=4, E=64, ms=4, cap=16, stride=2)
        a.update(kw)
        assert pool(p, p, table, p, a["S"], a["NW"], a["w0"], a["w1"], a["T"], a["E"], a["ms"], a["cap"], a["stride"], 2, None) != 0
        assert call(ptrs=[p, p, table, p], **kw) != 0
        theirs, mine = pool_err().decode(), err().decode()
        assert theirs.startswith("cfsp_window_sequences: ") and mine.startswith("cftp_window_sequences: "), (theirs, mine)
        assert mine.split(": ", 1)[1] == theirs.split(": ", 1)[1], (theirs, mine)
        return err()

    for i in range(4):
        ptrs = [p, p, good, p]
        ptrs[i] = None
        assert call(ptrs=ptrs) != 0 and b"null pointer" in err(), i
    assert call(rates=None) != 0 and b"null pointer" in err()
    assert b"null pointer" in same_words_as_the_pool(table=None)
    for kw in ({"NW": 0}, {"E": 0}, {"cap": 0}, {"NW": -1}):
        assert b"bad shape" in same_words_as_the_pool(**kw), kw
    for T in (0, 33, -1):
        assert b"T=%d outside 1 .. 32" % T in same_words_as_the_pool(T=T), T
    for stride in (0, -3):
        assert b"stride=%d must be at least 1" % stride in same_words_as_the_pool(stride=stride)
    for w0, w1 in ((-1, 2), (2, 2), (3, 2), (0, 4)):
        assert b"window range" in same_words_as_the_pool(w0=w0, w1=w1), (w0, w1)
    # the rates: 1 .. 8 of them, strictly ascending, the first at least 1
    for R in (0, -1, 9):
        assert call(rates=_rates(1, 2, 3, 4, 5, 6, 7, 8, 9), R=R) != 0 and b"R=%d rates outside 1 .. 8" % R in err(), R
    for first in (0, -2):
        assert call(rates=_rates(first, 2)) != 0 and b"rates[0]=%d must be at least 1" % first in err(), first
    for bad in ((2, 2), (3, 2), (1, 2, 2), (1, 3, 2), (1, 2, 3, 4, 5, 6, 7, 7)):
        assert call(rates=_rates(*bad), R=len(bad)) != 0 and b"strictly ascending" in err(), bad
    # the table: slots, positions, counts and prefix sums, in the pool's words
    for slot in (-1, 4):
        assert b"outside 0 .. 3" in same_words_as_the_pool(_edit(1, 0, slot))
    assert b"slot 2 appears twice" in same_words_as_the_pool(_edit(2, 0, 2))
    for col in (2, 5):
        assert b"negative count" in same_words_as_the_pool(_edit(0, col, -1))
    for col in (3, 6):
        assert b"prefix sums" in same_words_as_the_pool(_edit(2, col, 5))
    assert b"has_state=2" in same_words_as_the_pool(_edit(1, 7, 2))
    for col in (1, 4):
        for pos in (-1, 16):
            assert b"ring position" in same_words_as_the_pool(_edit(1, col, pos))
    assert b"row 0: n=17 frames do not fit" in same_words_as_the_pool(_tbl([[0, 0, 17, 0, 0, 0, 0, 0]]), S=1, NW=1, w1=1)
    assert b"not to NW=4" in same_words_as_the_pool(NW=4)
    for ms in (0, 1 << 20):
        assert b"max_streams=" in same_words_as_the_pool(ms=ms)
    for S in (0, 5):
        assert b"rows for max_streams=4" in same_words_as_the_pool(S=S)
    # a row's windows in the ring, judged at rmax: two windows at stride 2 of T = 4 frames at rate 5 span 2 + 15 + 1 = 18 > cap = 16 --
    # whatever the slower tempos would need
    assert call(rates=_rates(1, 5)) != 0 and b"row 2: the 18 frames of nW=2 windows do not fit a ring of cap=16" in err()
    assert b"do not fit" in same_words_as_the_pool(stride=1 << 30)
    # sizes: (w1 - w0) * R * T row pieces, and the ring's, below 2^31
    assert call(E=1 << 22, cap=2047) != 0 and b"too large for one launch" in err()
    big = _tbl([[0, 0, 0, 0, 0, 1 << 20, 0, 0]])
    # 2^20 windows of one 1024-float frame are 2^28 pieces, the ring as many: only the R = 8 tempos of each make it too many
    assert call(ptrs=[p, p, big, p], S=1, NW=1 << 20, w1=1 << 20, T=1, E=1024, ms=1, cap=(1 << 20) + 8, stride=1,
                rates=_rates(1, 2, 3, 4, 5, 6, 7, 8), R=8) != 0 and b"too large" in err() and b"R=8" in err()


def test_reduce_validation_without_gpu(clib):
    err = clib.cftp_last_error
    s, o, t = ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 30), ctypes.c_void_p(1 << 31)       # far apart: nothing overlaps

    # reduce(scores, out, tempo, NW, R, C, stream)
    def call(ptrs=(s, o, t), NW=5, R=3, C=7):
        return clib.cftp_reduce(*ptrs, NW, R, C, None)

    for i in range(3):
        ptrs = [s, o, t]
        ptrs[i] = None
        assert call(ptrs=ptrs) != 0 and b"null pointer" in err(), i
    for kw in ({"NW": 0}, {"C": 0}, {"NW": -3}, {"C": -1}):
        assert call(**kw) != 0 and b"bad shape" in err(), kw
    for R in (0, -1, 9):
        assert call(R=R) != 0 and b"R=%d rates outside 1 .. 8" % R in err(), R
    assert call(NW=1 << 15, R=8, C=1 << 13) != 0 and b"too large for one launch" in err()         # 2^31 scores
    # out inside scores, at its start, overlapping its end, and scores inside out; the byte behind scores is free
    size = 5 * 3 * 7 * 4
    for at in (0, 4, size - 4):
        assert call(ptrs=(s, ctypes.c_void_p(s.value + at), t)) != 0 and b"out overlaps scores" in err() and b"of its own" in err(), at
    assert call(ptrs=(s, ctypes.c_void_p(s.value - 4), t)) != 0 and b"out overlaps scores" in err()
    for ptrs in ((s, o, ctypes.c_void_p(s.value + 8)), (s, o, ctypes.c_void_p(o.value + 5 * 7 * 4 - 4)), (s, o, o)):
        assert call(ptrs=ptrs) != 0 and b"tempo overlaps scores or out" in err(), ptrs


def test_python_wrappers_reject_cpu_tensors_and_bad_shapes(clib):
    from clip_fsar_amd import tempo_hip as th
    host = torch.tensor(GOOD, dtype=torch.int32)
    table = th.Table(host, host, 3)               # a device copy that is no device tensor
    with pytest.raises(RuntimeError, match="HIP device tensor"):
        th.window_sequences(torch.zeros(4, 16, 8), torch.zeros(6, 4, 8), table, 3, 0, 3, 4, 2, (1, 2))
    with pytest.raises(RuntimeError, match="shape"):
        th.window_sequences(torch.zeros(4, 16, 8), torch.zeros(5, 4, 8), table, 3, 0, 3, 4, 2, (1, 2))       # 3 windows x 2 tempos
    with pytest.raises(RuntimeError, match="shape"):
        th.window_sequences(torch.zeros(4, 16, 8), torch.zeros(6, 4, 4), table, 3, 0, 3, 4, 2, (1, 2))
    with pytest.raises(RuntimeError, match="Table"):
        th.window_sequences(torch.zeros(4, 16, 8), torch.zeros(6, 4, 8), th.Table(host[:, :7], host, 3), 3, 0, 3, 4, 2, (1, 2))
    i32 = dict(dtype=torch.int32)
    with pytest.raises(RuntimeError, match="HIP device tensor"):
        th.reduce(torch.zeros(6, 5), torch.zeros(2, 5), torch.zeros(2, 5, **i32), 3)
    with pytest.raises(RuntimeError, match="no multiple of R"):
        th.reduce(torch.zeros(7, 5), torch.zeros(2, 5), torch.zeros(2, 5, **i32), 3)
    for out, tempo in ((torch.zeros(3, 5), torch.zeros(2, 5, **i32)), (torch.zeros(2, 5), torch.zeros(2, 4, **i32))):
        with pytest.raises(RuntimeError, match="shape"):
            th.reduce(torch.zeros(6, 5), out, tempo, 3)


# ------------------------------------------------------------------ tempo_positions against a brute-force ring
@pytest.mark.parametrize("T", [1, 2, 5, 32])
@pytest.mark.parametrize("stride", [1, 2, 8])
def test_tempo_positions_against_a_brute_force_ring(T, stride):
    """The ring as a list: frame f of the session lies at f mod cap once pushed.  Every tempo of every window still in the ring after t
    frames reads the frames e - (T - 1 - j) * rate, e the window's last frame; tempo R - 1 is the row pool_window_sequences_kernel
    documents for rate = rmax, (win_pos + w * stride + j * rmax) mod cap."""
    from clip_fsar_amd.pool import enrolable_windows, tempo_positions
    from clip_fsar_amd.stream import window_plan
    max_push = 6
    for rates in ((1,), (3,), (1, 3), (1, 2, 4), (1, 2, 3, 4, 5, 6, 7, 8)):
        rmax = rates[-1]
        cap = (T - 1) * rmax + max_push
        wrapped = 0
        for t in (cap, cap + 3, 3 * cap + 1):                                      # frames pushed so far: a full ring, and wrapped ones
            ring = [None] * cap
            for f in range(t):
                ring[f % cap] = f
            for n in (1, 3, max_push):                                             # the windows a push of the last n frames completed
                first, nW = window_plan(t - n, n, T, stride, rmax)
                win_pos = (first * stride) % cap
                for w in range(nW):
                    k = first + w
                    assert k in enrolable_windows(t, T, stride, rmax, cap)
                    e = k * stride + (T - 1) * rmax
                    got = tempo_positions(win_pos, w, stride, T, rates, cap)
                    assert len(got) == len(rates) and all(len(row) == T for row in got)
                    for i, rate in enumerate(rates):
                        assert [ring[pos] for pos in got[i]] == [e - (T - 1 - j) * rate for j in range(T)], (rates, t, k, i)
                        assert got[i][-1] == e % cap                               # every tempo ends on the window's newest frame
                    assert got[-1] == [(win_pos + w * stride + j * rmax) % cap for j in range(T)]
                    wrapped += t > cap
        assert wrapped, rates


# ------------------------------------------------------------------ reference_reduce on hand-written cases
def _bits(t):
    return t.contiguous().view(torch.int32)


def test_reference_reduce_hand_cases():
    from clip_fsar_amd.pool import reference_reduce
    # one window, R = 3, a column per case
    S = torch.tensor([[5.0, 2.0, NAN, 1.0, 1.0, -INF, -INF, 0.0, -0.0, INF],
                      [1.0, 2.0, 9.0, NAN, 7.0, -INF, -3.0, -0.0, 0.0, NAN],
                      [5.0, 2.0, 9.5, 8.0, NAN, -INF, -INF, 0.0, 0.0, INF]])
    out, tempo = reference_reduce(S, 3)
    assert tempo.dtype == torch.int32 and out.dtype == torch.float32 and tuple(out.shape) == tuple(tempo.shape) == (1, 10)
    #                          tie 0/2  all   NaN first  middle  last  all -inf  one finite  zeros  -0 first  NaN beats inf
    assert tempo[0].tolist() == [0,      0,    0,         1,      2,    0,        1,          0,     0,        1]
    want = torch.tensor([5.0, 2.0, NAN, NAN, NAN, -INF, -3.0, 0.0, -0.0, NAN])
    assert torch.equal(_bits(out[0]), _bits(want))                                 # bit for bit: the NaNs stay, and -0.0 is tempo 0's
    # the result is one of the inputs: a NaN keeps its payload
    odd = torch.tensor([0x7fc12345, 0x3f800000], dtype=torch.int32).view(torch.float32).view(2, 1)
    out, tempo = reference_reduce(odd, 2)
    assert _bits(out).item() == 0x7fc12345 and tempo.item() == 0
    out, tempo = reference_reduce(odd.flip(0), 2)
    assert _bits(out).item() == 0x7fc12345 and tempo.item() == 1
    # R = 1: a copy and a plane of zeros
    one = torch.tensor([[1.0, NAN, -INF], [4.0, -0.0, INF]])
    out, tempo = reference_reduce(one, 1)
    assert torch.equal(_bits(out), _bits(one)) and not tempo.any() and tuple(tempo.shape) == (2, 3)
    # several windows: rows ordered (window, tempo)
    S = torch.tensor([[1.0], [2.0], [4.0], [3.0], [NAN], [9.0]])
    out, tempo = reference_reduce(S, 2)
    assert tempo.view(-1).tolist() == [1, 0, 0] and torch.equal(_bits(out.view(-1)), _bits(torch.tensor([2.0, 4.0, NAN])))
    g = torch.Generator().manual_seed(3)
    S = torch.randn(5 * 4, 6, generator=g)
    out, tempo = reference_reduce(S, 4)
    assert torch.equal(out, S.view(5, 4, 6).max(1).values) and torch.equal(tempo.long(), S.view(5, 4, 6).argmax(1))
    for bad, R in ((torch.zeros(5, 2), 2), (torch.zeros(4), 2), (torch.zeros(4, 2), 0)):
        with pytest.raises(ValueError, match="scores must be"):
            reference_reduce(bad, R)


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


def test_stream_pool_rates_refusals_are_raised_before_the_device_is_touched():
    from clip_fsar_amd import pool as pm
    from clip_fsar_amd.baseline import Baseline
    from clip_fsar_amd.events import EventRule
    from clip_fsar_amd.gallery import SupportGallery
    from clip_fsar_amd.live_text_gallery import LiveTextGallery
    from clip_fsar_amd.pool import StreamPool
    from clip_fsar_amd.shortlist import Shortlist
    from clip_fsar_amd.stream import StreamOutput
    from clip_fsar_amd.text_gallery import TextGallery
    g = _live()
    rule, base = EventRule(0.6, 0.4, 2, 2), Baseline()
    # the pool plans, sizes its ring and numbers its windows as the rate = rmax pool: T = 4, rmax = 3, cap = 9 + 5
    p = StreamPool(g, max_streams=3, stride=2, max_push=5, smooth=0.5, smooth_by="class", events=rule, baseline=base, rates=(1, 2, 3))
    q = StreamPool(g, max_streams=3, stride=2, rate=3, max_push=5)
    assert p.rates == (1, 2, 3) and p.rate == 3 == q.rate and p.cap == q.cap == 14 and p._ring.shape == q._ring.shape
    assert q.rates is None and StreamPool(g, rates=[2, 5]).rates == (2, 5) and StreamPool(g, rates=(4,)).rate == 4
    assert StreamPool(SupportGallery(_stub_head(), "cpu"), smooth=0.5, rates=(1, 2)).rates == (1, 2)     # both kinds are served
    assert StreamPool(g, rates=tuple(range(1, 9))).rate == 8
    with pytest.raises(TypeError):
        StreamPool(g, 3, 2, 1, 5, 0.0, None, "column", None, None, (1, 2))          # keyword-only
    for bad in (3, "12", 1.5, {1, 2}):
        with pytest.raises(TypeError, match="StreamPool: rates must be a tuple of integers"):
            StreamPool(g, rates=bad)
    for rate in (2, 3):
        with pytest.raises(ValueError, match="rates= is given together with rate = %d -- leave rate at its default" % rate):
            StreamPool(g, rate=rate, rates=(1, 2, 3))
    for bad in ((), tuple(range(1, 10))):
        with pytest.raises(ValueError, match="rates holds %d values -- give 1 to 8" % len(bad)):
            StreamPool(g, rates=bad)
    for bad in ((1, 2.0), (0, 1), (-1,), (1, True), (1, "2")):
        with pytest.raises(ValueError, match="rates must hold integers >= 1"):
            StreamPool(g, rates=bad)
    for bad in ((2, 1), (1, 1), (1, 3, 3), (1, 3, 2)):
        with pytest.raises(ValueError, match="rates must be strictly ascending.*sort them"):
            StreamPool(g, rates=bad)
    with pytest.raises(ValueError, match="rates= on a TextGallery is not supported.*softmax.*use a SupportGallery or a LiveGallery"):
        StreamPool(TextGallery(_stub_head(COMBINE=True), "cpu"), rates=(1, 2))
    text = LiveTextGallery.__new__(LiveTextGallery)
    text.T, text.E, text.dev = 4, 8, torch.device("cpu")
    with pytest.raises(ValueError, match="rates= on a LiveTextGallery is not supported"):
        StreamPool(text, rates=(1, 2))
    with pytest.raises(ValueError, match="rates= together with shortlist= is not supported.*one of the two"):
        StreamPool(g, shortlist=Shortlist(g, keep=2), rates=(1, 2))
    with pytest.raises(ValueError, match=r"open\(classes=\) on a pool with rates= is not supported.*without a list"):
        p.open(classes=[0, 1])
    assert q.open(classes=[0, 1]) == 0            # a pool without the option is the pool as it was
    h = p.open()
    assert p.stats(h) == {"frames": 0, "tower_frames": 0, "windows": 0}
    # tempo=: an index into rates; None is the last one.  T = 4, stride 2, rmax 3: window w spans frames 2 w .. 2 w + 9
    p._sessions[h].t = 31                         # frames 17 .. 30 retained: windows 9 (18 .. 27) and 10 (20 .. 29)
    assert p.enrolable(h) == range(9, 11) == q_enrolable(q, 31)
    assert p._tempo(None, "x") == (3, 0) == p._tempo(2, "x") and p._tempo(1, "x") == (2, 3) and p._tempo(0, "x") == (1, 6)
    for bad in (3, -1, True, 1.0, "1"):
        for call, name in ((lambda t: p.enroll(h, 7, tempo=t), "enroll_windows"), (lambda t: p.enroll_windows([(h, None, 7)], tempo=t),
                           "enroll_windows"), (lambda t: p.explain(h, [0], tempo=t), "explain")):
            with pytest.raises(ValueError, match=r"StreamPool.%s: tempo must be an index into rates = \(1, 2, 3\), 0 .. 2, or None"
                               % name):
                call(bad)
    hq = q.open()
    for call, name in ((lambda: q.enroll(hq, 7, tempo=0), "enroll_windows"), (lambda: q.enroll_windows([(hq, None, 7)], tempo=0),
                       "enroll_windows"), (lambda: q.explain(hq, [0], tempo=0), "explain")):
        with pytest.raises(ValueError, match=r"StreamPool.%s: tempo = 0 on a pool without rates= -- build the pool with rates=" % name):
            call()
    before = dict(p.stats(h)), p._sessions[h].t
    for tempo in (None, 0, 1, 2):                 # a good tempo: the call gets as far as the device
        with pytest.raises(RuntimeError, match="HIP device tensor"):
            p.explain(h, k=2, window=9, tempo=tempo)
    with pytest.raises(ValueError, match="window 11 is not enrolable"):
        p.explain(h, [0], window=11, tempo=0)
    assert (dict(p.stats(h)), p._sessions[h].t) == before and g._store is None
    # the output types: subclasses of the plain ones with the same tuple
    for plain_type, mine, both in ((pm.PackedOutput, pm.TempoPackedOutput, pm.DeviationTempoPackedOutput),
                                   (StreamOutput, pm.TempoStreamOutput, pm.DeviationTempoStreamOutput)):
        assert issubclass(mine, plain_type) and issubclass(both, mine) and mine._fields == both._fields == plain_type._fields
        assert mine.__name__ == "Tempo" + plain_type.__name__ and both.__name__ == "DeviationTempo" + plain_type.__name__
        n = len(plain_type._fields)
        o = both(*range(n), deviation="d", tempo="t", rates=(1, 2))
        assert tuple(o) == tuple(range(n)) and (o.deviation, o.tempo, o.rates) == ("d", "t", (1, 2))
        o = mine(*range(n), tempo="t", rates=(3,))
        assert tuple(o) == tuple(range(n)) and (o.tempo, o.rates) == ("t", (3,)) and not hasattr(o, "deviation")
    # _split hands each session its block of the plane
    po = pm.DeviationTempoPackedOutput([7, 9], [0, 4], [0, 2, 5], torch.arange(15.0).view(5, 3), None, deviation=torch.zeros(5, 3),
                                       tempo=torch.arange(15, dtype=torch.int32).view(5, 3), rates=(1, 2))
    parts = StreamPool._split(po)
    assert isinstance(parts[7], pm.DeviationTempoStreamOutput) and parts[9].rates == (1, 2) and parts[9].first_window == 4
    assert parts[7].tempo.tolist() == [[0, 1, 2], [3, 4, 5]] and parts[9].tempo.tolist() == [[6, 7, 8], [9, 10, 11], [12, 13, 14]]
    assert tuple(parts[9].deviation.shape) == (3, 3) and parts[9].logits.tolist() == po.logits[2:].tolist()
    parts = StreamPool._split(pm.TempoPackedOutput([7], [0], [0, 0], torch.zeros(0, 3), None, tempo=torch.zeros(0, 3, dtype=torch.int32),
                                                   rates=(2,)))
    assert type(parts[7]) is pm.TempoStreamOutput and tuple(parts[7].tempo.shape) == (0, 3)


def q_enrolable(q, t):
    from clip_fsar_amd.pool import enrolable_windows
    return enrolable_windows(t, q.T, q.stride, q.rate, q.cap)
