"""CPU: the enrolment library (libclipfsar_enroll.so, include/clipfsar_enroll.h) validates its enrolment list without a GPU and takes its copy-
kernel plumbing from ring_rows.h; pool.plan_enroll against a brute-force ring; misuse of StreamPool.enroll / enroll_windows and of
LiveGallery's registration from features on a stub head.  Its exports, kernels and place in the build are checked with every library's in
tests/test_build_recipe.py."""
import ctypes
import os
import random
import re
from types import SimpleNamespace as NS

import pytest

from _abi import _prototypes, check_abi_at_load, check_exports, lib_row

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "clipfsar_enroll.h")


@pytest.fixture(scope="module")
def elib():
    import __graft_entry__ as ge
    ge.build()                                    # builds every library (no-op when up to date)
    from clip_fsar_amd import enroll_hip
    return enroll_hip.lib()


# ------------------------------------------------------------------ what is particular to this library's header and source
def test_header_exported_exactly_and_arity_matches(elib):
    check_exports(lib_row("enroll"))                 # the checks every library gets; below, what is particular to this one
    from clip_fsar_amd import enroll_hip as eh
    from clip_fsar_amd import pool_hip as ph
    protos = _prototypes(HEADER, "cfen_")
    assert protos["cfen_ring_sequences"] == 13
    text = open(HEADER).read()
    assert int(re.search(r"#define CFEN_TABLE_COLS (\d+)", text).group(1)) == eh.TABLE_COLS == 4
    for i, col in enumerate(("SLOT", "POS", "CLS", "PAD")):                       # the binding's column order is the header's
        assert int(re.search(r"#define CFEN_%s (\d+)" % col, text).group(1)) == getattr(eh, col) == i
    assert '#include "clipfsar_pool.h"' in text and eh.MAX_T == ph.MAX_T == 32    # the windows are the pool's: CFSP_MAX_T
    assert eh.table_rows([3, 0], [7, 1], [0, 1]) == [[3, 7, 0, 0], [0, 1, 1, 0]]
    assert eh.table_uploader("cpu", 4).cols == eh.TABLE_COLS


def test_abi_version_is_checked_at_load(elib, monkeypatch):
    check_abi_at_load(lib_row("enroll"), monkeypatch)


def test_the_source_takes_its_copy_kernel_plumbing_from_ring_rows():
    from clip_fsar_amd import build as b
    src = open(os.path.join(b.CSRC, b.SIDE_LIBS["enroll"].source)).read()
    for body in ("__shared__", "asm", "struct Piece", "MAX_BLOCKS =", "MAX_ITEMS =", "unsigned blocks_for", "thread_local"):
        assert body not in src, body
    assert '#include "ring_rows.h"' in src and "Piece<VEC>" in src and "blocks_for(" in src


# ------------------------------------------------------------------ the enrolment list, without a GPU
def _tbl(rows):
    flat = [v for r in rows for v in r]
    return (ctypes.c_int32 * len(flat))(*flat)


#        SLOT POS CLS PAD       max_streams 3, cap 14 (T 5, rate 3, max_push 2), 2 classes
GOOD = [[0,   0,  0,  0],
        [2,  13,  1,  0],
        [2,  13,  1,  0],      # the same slot and window twice
        [0,   5,  1,  0]]


def _edit(row, col, value):
    rows = [list(r) for r in GOOD]
    rows[row][col] = value
    return _tbl(rows)


def test_table_validation_without_gpu(elib):
    p = ctypes.c_void_p(4096)                     # never dereferenced: every call below fails validation before any device work
    err, good = elib.cfen_last_error, _tbl(GOOD)

    # ring_sequences(ring, text, table_host, table_dev, n, T, E, max_streams, cap, rate, n_cls, X0, stream)
    def seq(table=good, n=4, T=5, E=64, M=3, cap=14, rate=3, n_cls=2, **ptr):
        a = dict(ring=p, text=p, tdev=p, X0=p)
        a.update(ptr)
        return elib.cfen_ring_sequences(a["ring"], a["text"], table, a["tdev"], n, T, E, M, cap, rate, n_cls, a["X0"], None)

    for name in ("ring", "text", "tdev", "X0"):
        assert seq(**{name: None}) != 0 and b"null" in err(), name
    assert seq(table=None) != 0 and b"null" in err()
    for kw in ({"n": 0}, {"n": -1}, {"E": 0}, {"M": 0}, {"cap": 0}, {"n_cls": 0}):
        assert seq(**kw) != 0 and b"bad shape" in err(), kw
    for T in (0, -1, 33):
        assert seq(T=T) != 0 and b"outside 1 .. 32" in err(), T
    for rate in (0, -3):
        assert seq(rate=rate) != 0 and b"rate=" in err(), rate
    assert seq(cap=12, table=_tbl([[0, 0, 0, 0]]), n=1) != 0 and b"the 13 frames of a window do not fit a ring of cap=12" in err()
    assert seq(rate=4) != 0 and b"do not fit" in err()
    # each column, once below and once above its range, in a first, a middle and the last row
    for row in (0, 1, 3):
        for col, bad, msg in ((0, -1, b"slot"), (0, 3, b"slot"), (1, -1, b"ring position"), (1, 14, b"ring position"),
                              (2, -1, b"class"), (2, 2, b"class")):
            assert seq(table=_edit(row, col, bad)) != 0 and msg in err() and (b"row %d " % row) in err(), (row, col, bad)
    # 32-bit: every element count
    assert seq(M=65536, cap=40000, E=64) != 0 and b"too large for one launch" in err()            # the ring
    assert seq(n_cls=1 << 28, E=64) != 0 and b"too large for one launch" in err()                 # the text rows
    assert seq(T=32, rate=1, cap=32, E=8192, table=_tbl([[0, 0, 0, 0]] * 33000), n=33000) != 0 and b"too large for one launch" in err()


def test_python_wrapper_rejects_cpu_tensors_and_bad_shapes(elib):
    import torch
    from clip_fsar_amd import enroll_hip as eh
    from clip_fsar_amd import pool_hip as ph
    host = torch.tensor(GOOD, dtype=torch.int32)
    table = ph.Table(host, host, 4)               # a device copy that is no device tensor
    ring, text, X0 = torch.zeros(3, 14, 64), torch.zeros(2, 64), torch.zeros(4, 6, 64)
    with pytest.raises(RuntimeError, match="HIP device tensor"):
        eh.ring_sequences(ring, text, table, X0, 3)
    with pytest.raises(RuntimeError, match="text has shape"):
        eh.ring_sequences(ring, text[:, :32], table, X0, 3)
    with pytest.raises(RuntimeError, match="X0 has shape"):
        eh.ring_sequences(ring, text, table, X0[:, :1], 3)
    with pytest.raises(RuntimeError, match="Table"):
        eh.ring_sequences(ring, text, ph.Table(host[:, :3], host, 4), X0, 3)


# ------------------------------------------------------------------ plan_enroll against a brute-force ring
@pytest.mark.parametrize("T", [1, 5, 8])
@pytest.mark.parametrize("stride", [1, 2, 3])
@pytest.mark.parametrize("rate", [1, 3])
@pytest.mark.parametrize("max_push", [1, 2, 64])
def test_plan_enroll_against_a_ring_of_frame_numbers(T, stride, rate, max_push):
    """the ring as the pool writes it: frame f of a session at position f mod cap.  Whatever the planner accepts is in the ring, frame
    by frame; the windows one below and one above the range are refused."""
    from clip_fsar_amd.pool import enrolable_windows, plan_enroll
    from clip_fsar_amd.stream import window_plan
    rng = random.Random(1000 * T + 100 * stride + 10 * rate + max_push)
    cap = (T - 1) * rate + max_push
    ring, t = [None] * cap, 0
    assert enrolable_windows(0, T, stride, rate, cap) == range(0)                # after open() / reset(): nothing
    with pytest.raises(ValueError, match="not enrolable"):
        plan_enroll([(4, 0)], [(0, None)], T, stride, rate, cap)
    accepted = wrapped = 0
    for step in range(60):
        for _ in range(rng.randint(1, max_push)):                                 # one push
            ring[t % cap] = t
            t += 1
        ok = enrolable_windows(t, T, stride, rate, cap)
        nW = window_plan(0, t, T, stride, rate)[1]
        assert ok.stop == nW or not len(ok)
        if nW and stride <= max_push:
            assert nW - 1 in ok                                                   # the newest complete window is always there
        if len(ok):
            plan = plan_enroll([(9, 10 ** 9), (4, t)], [(1, w) for w in ok] + [(1, None)], T, stride, rate, cap)
            assert plan.windows == list(ok) + [nW - 1] and plan.slots == [4] * (len(ok) + 1)
            for w, pos in zip(plan.windows, plan.positions):
                assert 0 <= pos < cap
                assert [ring[(pos + j * rate) % cap] for j in range(T)] == [w * stride + j * rate for j in range(T)], (t, w)
                wrapped += pos + (T - 1) * rate >= cap
            accepted += len(ok)
        lo, hi = (ok.start - 1, ok.stop) if len(ok) else (nW - 1, nW)
        for w in (lo, hi, -1, True, 1.0, "0"):
            with pytest.raises(ValueError, match=r"session 1: window .* is not enrolable -- the ring holds its windows range\(\d+, \d+\)"):
                plan_enroll([(9, 10 ** 9), (4, t)], [(1, w)], T, stride, rate, cap)
        if lo >= 0 and lo < nW:                                                   # the window below: complete, its first frame overwritten
            assert ring[(lo * stride) % cap] != lo * stride
    assert t > 2 * cap
    assert accepted >= 10 and (wrapped or T == 1)
    with pytest.raises(ValueError, match="kite cam: window 0 is not enrolable"):
        plan_enroll([(0, 0)], [(0, 0)], T, stride, rate, cap, names=["kite cam"])


# ------------------------------------------------------------------ StreamPool and LiveGallery on a stub head: misuse, before any launch
def _stub_head(T=4, n_test=3, **train):
    import torch
    engine = NS(arch={"embed": 8}, text_test=torch.zeros(n_test, 8))
    return NS(args=NS(TRAIN=NS(**train), DATA=NS(NUM_INPUT_FRAMES=T)), _get_engine=lambda dev: engine, _engine_key=("stub",),
              arch_name="stub", precision="fp32", depth=1)


def _stub_gallery(ids=("a", "b", 1)):
    from clip_fsar_amd import live_gallery as lg
    g = lg.LiveGallery(_stub_head(), "cpu", capacity=4)
    if ids:
        g._install(lg.plan_add(g._book, list(ids)).book)       # registered on the host alone: nothing below reaches the device
    return g


def _snapshot(g):
    b = g._book
    return (b.cap, list(b.free), list(b.order), dict(b.slot_of), dict(b.shots), b.version, g._store, g.class_ids)


def test_registration_from_features_rejects_misuse_before_any_launch():
    import torch
    g = _stub_gallery()
    before = _snapshot(g)
    feats = torch.zeros(2, 4, 8)
    for call in (lambda f, ids: g.add_classes_features(f, ids), lambda f, ids: g.add_shots_features(f, ids)):
        with pytest.raises(RuntimeError, match="feats must be a HIP device tensor"):
            call(feats, ["a", "a"])
        with pytest.raises(RuntimeError, match="feats must be a HIP device tensor"):
            call([[0.0]], ["a"])
    g._check_feats = lambda f: lg_check(g, f)                   # the device check aside: what follows it, still before any launch
    for bad in (torch.zeros(2, 3, 8), torch.zeros(2, 4, 9), torch.zeros(2, 4, 3, 8, 8), torch.zeros(8)):
        with pytest.raises(ValueError, match=r"feats must be \[N, T=4, E=8\]"):
            g.add_classes_features(bad, ["x", "y"])
        with pytest.raises(ValueError, match=r"feats must be \[N, T=4, E=8\]"):
            g.add_shots_features(bad, ["a", "b"])
    # add_classes' errors
    with pytest.raises(ValueError, match="class 'a' is already registered"):
        g.add_classes_features(feats, ["x", "a"], text={"x": [0.0] * 8})
    with pytest.raises(ValueError, match="2 videos but 3 class ids"):
        g.add_classes_features(feats, ["x", "y", "z"])
    with pytest.raises(TypeError, match="`text` must map"):
        g.add_classes_features(feats, ["x", "y"], text=["x"])
    with pytest.raises(ValueError, match="class 'x' is not an index into TEST.CLASS_NAME"):
        g.add_classes_features(feats, ["x", "x"])
    with pytest.raises(ValueError, match="class 3 is not an index into TEST.CLASS_NAME"):
        g.add_classes_features(feats, [2, 3])
    with pytest.raises(ValueError, match="text row of class 'x' has 7 values, expected 8"):
        g.add_classes_features(feats, ["x", "x"], text={"x": [0.0] * 7})
    # add_shots' errors
    with pytest.raises(ValueError, match=r"class 'z' is not registered \(add_shots"):
        g.add_shots_features(feats, ["a", "z"])
    with pytest.raises(ValueError, match="2 videos but 1 class ids"):
        g.add_shots_features(feats, ["a"])
    with pytest.raises(ValueError, match="at least one video"):
        g.add_shots_features(feats[:0], [])
    g._book = g._book._replace(shots=dict(g._book.shots, b=0))
    before = _snapshot(g)
    with pytest.raises(ValueError, match="class 'b' was loaded without its sum"):
        g.add_shots_features(feats, ["a", "b"])
    assert _snapshot(g) == before and g._store is None and g._tables is None


def lg_check(g, feats):
    if feats.dim() != 3 or feats.shape[1] != g.T or feats.shape[2] != g.E:
        raise ValueError("%s: feats must be [N, T=%d, E=%d], got %s" % (g._name, g.T, g.E, tuple(feats.shape)))
    return feats


def _pool(g, frames=None, **kw):
    """a pool over the stub gallery with sessions whose frame counters are set by hand: nothing was pushed, nothing reaches the device"""
    from clip_fsar_amd.pool import StreamPool
    p = StreamPool(g, max_streams=3, **kw)
    hs = []
    for t in frames or ():
        hs.append(p.open())
        p._sessions[hs[-1]].t = t
    return p, hs


def test_stream_pool_rejects_enrolment_misuse_before_any_launch():
    from clip_fsar_amd.gallery import SupportGallery
    from clip_fsar_amd.pool import StreamPool
    sup = StreamPool(SupportGallery(_stub_head(), "cpu"), max_streams=2)
    h = sup.open()
    for call in (lambda: sup.enroll(h, 0), lambda: sup.enroll_windows([(h, None, 0)]), lambda: sup.enrolable(h)):
        with pytest.raises(ValueError, match=r"enrolment needs a gallery that registers from features \(a LiveGallery\), not a SupportGallery"):
            call()
    g = _stub_gallery()
    # T 4, stride 2, max_push 3: cap 6.  a: 11 frames -> windows 0 .. 3 complete, frames 5 .. 10 kept: window 3; b: 3 frames: none
    p, (a, b, c) = _pool(g, frames=(11, 3, 6), stride=2, max_push=3)
    assert p.cap == 6 and p.enrolable(a) == range(3, 4) and p.enrolable(b) == range(0) and p.enrolable(c) == range(0, 2)
    before, stats = _snapshot(g), (p.stats(), p.stats(a), p.stats(c))
    for items in ([], None, [(a, None)], [(a, None, "a", 1)], "abc", [a, None, "a"]):
        with pytest.raises(ValueError, match="non-empty list of"):
            p.enroll_windows(items)
    with pytest.raises(TypeError, match="`text` must map"):
        p.enroll_windows([(a, None, "x")], text=["x"])
    p.close(c)
    for bad in (c, 17, -1, True, "a", None):
        with pytest.raises(ValueError, match="is not open"):
            p.enroll_windows([(a, None, "a"), (bad, None, "a")])
        with pytest.raises(ValueError, match="is not open"):
            p.enroll(bad, "a")
    c = p.open()
    p._sessions[c].t = 6
    for w in (2, 4, -1, 3.0, True):
        with pytest.raises(ValueError, match=r"session %d: window .* is not enrolable -- the ring holds its windows range\(3, 4\)" % a):
            p.enroll_windows([(c, 1, "a"), (a, w, "a")])
        with pytest.raises(ValueError, match=r"range\(3, 4\)"):
            p.enroll(a, "a", window=w)
    with pytest.raises(ValueError, match=r"session %d: window None \(the newest complete one\) is not enrolable -- .* range\(0, 0\)" % b):
        p.enroll(b, "a")
    p.reset(a)
    with pytest.raises(ValueError, match=r"range\(0, 0\)"):                       # after reset() nothing is enrolable
        p.enroll(a, "a")
    p._sessions[a].t = 11
    # unknown classes need text, as in add_classes; a class that is known is no new class
    with pytest.raises(ValueError, match="class 'x' is not an index into TEST.CLASS_NAME .* and has no entry in `text`"):
        p.enroll_windows([(a, None, "a"), (c, 0, "x")])
    with pytest.raises(ValueError, match="class 7 is not an index into TEST.CLASS_NAME"):
        p.enroll(a, 7)
    with pytest.raises(ValueError, match="text row of class 'x' has 3 values, expected 8"):
        p.enroll(a, "x", text={"x": [1.0, 2.0, 3.0]})
    g._book = g._book._replace(shots=dict(g._book.shots, b=0))
    before = _snapshot(g)
    with pytest.raises(ValueError, match="class 'b' was loaded without its sum"):
        p.enroll_windows([(a, None, "a"), (c, 0, "b"), (c, 1, 2)])
    # a stale engine
    eng = g.head._get_engine("cpu")
    g.head._engine_key = ("other",)
    with pytest.raises(RuntimeError, match="changed since these prototypes"):
        p.enroll(a, "a")
    g.head._engine_key = ("stub",)
    assert g.head._get_engine("cpu") is eng
    # nothing moved: the gallery, the sessions, the pool's totals; no table, no store
    assert _snapshot(g) == before and g._store is None and g._tables is None and p._enroll_tables is None
    assert (p.stats(), p.stats(a), p.stats(c)) == stats
    assert p._sessions[a].classes is None


def test_enroll_returns_and_join_without_a_device(monkeypatch):
    """the host half of a successful call, with the two device steps of the gallery replaced: the plans, the order of the sequences in
    each launch, the returned counts, join"""
    import torch
    from clip_fsar_amd import enroll_hip as eh
    g = _stub_gallery()
    p, (a, b) = _pool(g, frames=(11, 8), stride=2, max_push=3)
    p._sessions[b].classes = ["a"]
    launches = []
    monkeypatch.setattr(p, "_ring_sequences", lambda trows, slots, positions, classes: launches.append((slots, positions, classes)) or "X0")
    monkeypatch.setattr(g, "_shots_sequences", lambda eng, plan, seq: (launches.append(("shots", plan.classes, seq("T"))),
                                                                       setattr(g, "_book", plan.book),
                                                                       [plan.book.shots[c] for c in plan.classes])[2])
    monkeypatch.setattr(g, "_register_sequences", lambda eng, trows, counts, plan, seq: (
        launches.append(("classes", counts, tuple(trows.shape), seq(trows))), g._install(plan.book)))
    sa, sb = p._sessions[a].slot, p._sessions[b].slot
    assert p.enrolable(b) == range(1, 3)
    # class 2 is new (a TEST.CLASS_NAME index) with two shots, "k" is new with a text row; "a" takes two further shots, 1 one
    out = p.enroll_windows([(a, None, 2), (b, 1, "a"), (b, 2, "k"), (a, 3, 1), (b, None, 2), (b, 2, "a")], text={"k": [0.5] * 8})
    assert out == {2: 2, "a": 3, "k": 1, 1: 2} and list(out) == [2, "a", "k", 1]
    pos = lambda w: (w * 2) % p.cap
    assert launches == [([sb, sb, sa], [pos(1), pos(2), pos(3)], [0, 0, 1]), ("shots", ["a", 1], ("X0", [0, 2, 3])),
                        ([sa, sb, sb], [pos(3), pos(2), pos(2)], [0, 0, 1]), ("classes", [2, 1], (2, 8), ("X0", [0, 2, 3]))]
    assert g.class_ids == ["a", "b", 1, 2, "k"] and [g.shots(c) for c in g.class_ids] == [3, 1, 2, 2, 1]
    assert p._sessions[b].classes == ["a"]                                         # no join asked for
    assert p.enroll(b, "k", join=True) == 2 and p._sessions[b].classes == ["a", "k"]
    assert p.enroll(b, "a", window=1, join=True) == 4 and p._sessions[b].classes == ["a", "k"]      # already in the list
    assert p.enroll(a, 0, join=True) == 1 and p._sessions[a].classes is None        # no list: the session sees every class anyway
    assert eh.TABLE_COLS == 4
