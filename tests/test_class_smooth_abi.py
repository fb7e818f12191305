"""CPU: per-class smoothing (libclipfsar_class_smooth.so, include/ext/clipfsar_class_smooth.h, clip_fsar_amd.class_smooth_hip) -- the
extension library's exports, ABI check at load, resource report and place in the build (a second registry, build.EXT_LIBS, beside the ten
side libraries'); its host validation without a GPU; the pure host planner against a brute-force model; LiveGallery's slot generations
against a dict model over random schedules; and StreamPool's smooth_by option on stub heads."""
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
HEADER = os.path.join(ROOT, "include", "ext", "clipfsar_class_smooth.h")
ROW = _abi._row("class_smooth", "class_smooth_hip", "cfcs_", "ext/clipfsar_class_smooth.h", "version abi_version last_error smooth_classes",
                {"class_smooth_kernel": 1}, 1)


@pytest.fixture(scope="module")
def clib():
    import __graft_entry__ as ge
    ge.build()                                    # builds every library (no-op when up to date)
    from clip_fsar_amd import class_smooth_hip
    return class_smooth_hip.lib()


# ------------------------------------------------------------------ the library and its place in the build
def test_header_exported_exactly_and_arity_matches(clib):
    check_exports(ROW)
    assert ROW.exports == {"cfcs_version", "cfcs_abi_version", "cfcs_last_error", "cfcs_smooth_classes"}
    from clip_fsar_amd import class_smooth_hip as ch
    text = open(HEADER).read()
    assert int(re.search(r"#define CFCS_MAX_STREAMS (\d+)", text).group(1)) == ch.MAX_STREAMS
    assert int(re.search(r"#define CFCS_CHUNK (\d+)", text).group(1)) == ch.CHUNK
    assert int(re.search(r"#define CFCS_TABLE_COLS (\d+)", text).group(1)) == ch.TABLE_COLS == 6
    for i, col in enumerate(("SLOT", "NW", "OUT0", "NC", "KEY0", "CHUNK0")):      # the binding's column order is the header's
        assert int(re.search(r"#define CFCS_%s (\d+)" % col, text).group(1)) == getattr(ch, col) == i
    assert len(ch.SIGNATURES["cfcs_smooth_classes"]) == 15
    for other in _abi.LIBS:                       # its prefix hides no other library's, and none hides it
        assert not other.prefix.startswith(ROW.prefix) and not ROW.prefix.startswith(other.prefix), other.name


def test_abi_version_is_checked_at_load(clib, monkeypatch):
    check_abi_at_load(ROW, monkeypatch)


def test_the_kernel_is_the_listed_one_and_uses_no_scratch(clib):
    from clip_fsar_amd import build as b
    from clip_fsar_amd import class_smooth_hip as ch
    el = b.EXT_LIBS["class_smooth"]
    if not os.path.exists(el.usage):
        b.build_ext("class_smooth", force=True, verbose=False)
    usage = json.load(open(el.usage))
    assert len(usage) == ROW.total == 1 and all("class_smooth_kernel" in n for n in usage), sorted(usage)
    for n, u in usage.items():
        assert u.get("scratch", 0) == 0 and u.get("spills", 0) == 0, (n, u)
    assert os.path.normpath(el.usage).endswith(os.path.join("build", "class_smooth", "resource_usage.json"))
    assert el.lib == ch.LIB_PATH and el.lib.endswith(os.sep + "libclipfsar_class_smooth.so") and os.path.exists(el.lib)
    assert os.path.normpath(el.source).endswith(os.path.join("clip-fsar_amd", "ext", "class_smooth.hip")) and el.header == HEADER
    for row in _abi.SIDE:                         # and no report of a side library holds it
        assert not any("class_smooth_kernel" in n for n in json.load(open(b.SIDE_LIBS[row.name].usage))), row.name
    source = open(el.source).read()               # the recurrence and the error plumbing are the shared ones; plain C++
    assert '#include "../csrc/ring_rows.h"' in source and '#include "../csrc/side_lib.h"' in source and source.count("smooth_run(") == 1
    for body in ("__fmaf_rn", "asm", "thread_local", "calloc", "hipMalloc", "hipStreamCreate"):
        assert body not in source, body


def test_two_registries_ten_side_libraries_and_one_extension():
    from clip_fsar_amd import build as b
    assert list(b.SIDE_LIBS) == ["gallery", "gallery_text", "stream", "pool", "ingest", "live", "groups", "lastblock", "enroll", "live_text"]
    assert list(b.EXT_LIBS) == b.ext_lib_names() == ["class_smooth"] and b.EXT_LIBS is not b.SIDE_LIBS
    assert not set(b.EXT_LIBS) & set(b.SIDE_LIBS)
    assert b.ExtLib is not b.SideLib and all(isinstance(v, b.ExtLib) and not isinstance(v, b.SideLib) for v in b.EXT_LIBS.values())
    for call in (b._ext_deps, b.build_ext):
        with pytest.raises(KeyError):
            call("pool")
    with pytest.raises(KeyError):
        b.build_side("class_smooth")
    libs = [b.LIB] + [sl.lib for sl in b.SIDE_LIBS.values()] + [el.lib for el in b.EXT_LIBS.values()]
    reports = [b.USAGE] + [sl.usage for sl in b.SIDE_LIBS.values()] + [el.usage for el in b.EXT_LIBS.values()]
    assert len(set(libs)) == len(set(reports)) == 12
    assert not os.path.exists(os.path.join(b.CSRC, "class_smooth.hip"))


def test_staleness_of_the_extension_and_of_nothing_else(monkeypatch):
    from clip_fsar_amd import build as b
    from test_build_recipe import NAMES, STALE, P
    monkeypatch.setattr(b.os.path, "exists", lambda p: True)

    def stale_after(edited):
        monkeypatch.setattr(b.os.path, "getmtime", lambda p: 2.0 if p.endswith(os.sep + edited) else 1.0)
        old = {P} if b._stale(b.LIB, b._product_deps()) else set()
        old |= {n for n in NAMES if b._stale(b.SIDE_LIBS[n].lib, b._side_deps(n))}
        return old, b._stale(b.EXT_LIBS["class_smooth"].lib, b._ext_deps("class_smooth"))

    for edited in ("class_smooth.hip", "clipfsar_class_smooth.h"):                # the extension's own files: it alone
        assert stale_after(edited) == (set(), True), edited
    for edited in ("ring_rows.h", "side_lib.h", "common.h", "clipfsar_hip.h", "build.py"):       # shared: the others as their matrix has it
        assert stale_after(edited) == (STALE[edited], True), edited
    for edited in ("pool.hip", "clipfsar_pool.h", "otam_tile.h", "topk_wave.h", "gemm.hip", "live.hip"):
        assert stale_after(edited) == (STALE[edited], False), edited
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
    err, good = clib.cfcs_last_error, _tbl(GOOD)
    # smooth_classes(logits, state, marks, gens, keys, out, table_host, table_dev, S, NOUT, NKEYS, max_streams, cap, alpha, stream)
    call = lambda t, S=3, nout=NOUT, nkeys=NKEYS, ms=4, cap=300, alpha=0.5: clib.cfcs_smooth_classes(p, p, p, p, p, p, t, p, S, nout, nkeys,
                                                                                                    ms, cap, alpha, None)
    for i in range(8):
        args = [p, p, p, p, p, p, good, p]
        args[i] = None
        assert clib.cfcs_smooth_classes(*args, 3, NOUT, NKEYS, 4, 300, 0.5, None) != 0 and b"null" in err(), i
    for alpha in (1.0, 1.5, -0.1, float("nan"), float("inf")):
        assert call(good, alpha=alpha) != 0 and b"alpha" in err(), alpha
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
    assert clib.cfcs_smooth_classes(p, p, p, p, p, p, big, p, 1, 0, 60000, 4, 60000, 0.5, None) != 0 and b"too large" in err() \
        and b"row 0" in err()
    # a table without a window is valid and launches nothing
    assert clib.cfcs_smooth_classes(p, p, p, p, p, p, _tbl([[3, 0, 0, 7, 0, 0]]), p, 1, 0, 7, 4, 300, 0.5, None) == 0


def test_python_wrapper_rejects_cpu_tensors_and_bad_shapes(clib):
    import torch
    from clip_fsar_amd import class_smooth_hip as ch
    host = torch.tensor(GOOD, dtype=torch.int32)
    table = ch.Table(host, host, 3)
    x, st, mk, gens, keys = torch.zeros(NOUT), torch.zeros(4, 300), torch.zeros(4, 300, dtype=torch.int32), \
        torch.ones(300, dtype=torch.int32), torch.zeros(NKEYS, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="HIP device tensor"):
        ch.smooth_classes(x, st, mk, gens, keys, x, table, 0.5)
    for bad in ((x, st, mk[:3], gens, keys, x), (x, st, mk, gens[:299], keys, x), (x, st, mk, gens, keys, x[:5]),
                (x.view(2, -1), st, mk, gens, keys, x.view(2, -1))):
        with pytest.raises(RuntimeError, match="shape|flat"):
            ch.smooth_classes(*bad, table, 0.5)
    with pytest.raises(RuntimeError, match="1 .. 4 rows of 6"):
        ch.table_uploader("cpu", 4).upload([[0] * 8])


# ------------------------------------------------------------------ the host planner against a brute-force model
def test_planner_against_a_brute_force_model(clib):
    """random pushes: sessions with lists of their own (some equal, some overlapping), without one, and without windows.  The model walks
    the plan as the kernel does -- workgroup by workgroup -- and must visit every (session, window, column) once, at its place in the
    session-major flat layout, under the store slot the session's list names; and the library accepts the table."""
    from clip_fsar_amd import class_smooth_hip as ch
    rng = random.Random(7)
    p = ctypes.c_void_p(4096)
    shared = 0
    for trial in range(200):
        cap = rng.choice((5, 300, 700))
        every = rng.sample(range(cap), rng.randint(1, cap))
        S = rng.randint(1, 6)
        slots = rng.sample(range(8), S)
        n_windows = [rng.choice((0, 0, 1, 2, 5)) for _ in range(S)]
        pool_of_lists = [rng.sample(every, rng.randint(1, len(every))) for _ in range(2)]
        lists = [rng.choice([None, None] + pool_of_lists + [rng.sample(every, rng.randint(1, min(3, len(every))))]) for _ in range(S)]
        plan = ch.plan_rows(slots, n_windows, lists, len(every))
        assert len(plan.rows) == S and all(len(r) == ch.TABLE_COLS for r in plan.rows)
        # the planner holds the own lists, every distinct one once; the "every class" list, if a session points at it, leads the device
        # keys once: a push uploads O(C + the lists' lengths) keys
        distinct = {tuple(l) for l in lists if l is not None}
        assert len(plan.keys) == sum(len(d) for d in distinct) and plan.every == (None in lists)
        shared += len(distinct) + plan.every < S
        keys = (every if plan.every else []) + plan.keys
        # the model: the flat layout a push's logits have
        want, at = {}, 0
        for i in range(S):
            seg = every if lists[i] is None else lists[i]
            for k in range(n_windows[i]):
                for j, key in enumerate(seg):
                    want[at] = (slots[i], k, key)
                    at += 1
        assert plan.n_out == at
        got = {}
        for b in range(plan.n_chunks):
            row = [r for r in plan.rows if r[ch.CHUNK0] <= b][-1]                  # CHUNK0 rises strictly: the last row at or below b
            for t in range(ch.CHUNK):
                j = (b - row[ch.CHUNK0]) * ch.CHUNK + t
                if j >= row[ch.NC]:
                    continue
                for k in range(row[ch.NW]):
                    index = row[ch.OUT0] + k * row[ch.NC] + j
                    assert index not in got
                    got[index] = (row[ch.SLOT], k, keys[row[ch.KEY0] + j])
        assert got == want
        if plan.n_out == 0:                       # without windows nothing is launched: the library's own verdict on the table
            assert clib.cfcs_smooth_classes(p, p, p, p, p, p, _tbl(plan.rows), p, S, 0, len(keys), 8, cap, 0.5, None) == 0, \
                clib.cfcs_last_error()
            assert clib.cfcs_smooth_classes(p, p, p, p, p, p, _tbl(plan.rows), p, S, 0, len(keys) - 1, 8, cap, 0.5, None) != 0
    assert shared > 50
    with pytest.raises(ValueError, match="empty"):
        ch.plan_rows([0], [1], [[]], 2)
    with pytest.raises(ValueError, match="empty"):
        ch.plan_rows([0], [1], [None], 0)
    plan = ch.plan_rows(list(range(64)), [8] * 64, [None] * 64, 3200)            # a dense push: no key to upload, 13 workgroups a session
    assert plan.keys == [] and plan.every and plan.n_out == 64 * 8 * 3200 and plan.n_chunks == 64 * 13
    assert all(r[ch.KEY0] == 0 and r[ch.NC] == 3200 for r in plan.rows)


# ------------------------------------------------------------------ slot generations against a dict model
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


@pytest.mark.parametrize("kind,seed", [("live", 1), ("live", 2), ("live_text", 3)])
def test_slot_generations_against_a_dict_model(kind, seed, monkeypatch):
    """add, remove, further shots, growth, clear() and load_state_dict in random order, the registrations installed as the device paths
    install them (plan_* -> _install).  Model: gen[slot] starts at 1; + 1 when the slot is freed or its class is replaced by another;
    clear() and load_state_dict: + 1 everywhere.  And what the generations are for: no two registrations that ever held a slot share its
    generation."""
    import torch
    from clip_fsar_amd.live_gallery import plan_add, plan_remove, plan_shots
    rng = random.Random(seed)
    g = _live(kind, 3)
    monkeypatch.setattr(g, "_ensure_store", lambda cap: g.__dict__.update(_store=g._alloc(cap)) or g._store)     # no device: no copies
    gen, owner, held = {s: 1 for s in range(3)}, {}, {}                           # held: slot -> {generation: registration number}
    next_id, registration, grew, ops = 0, 0, 0, set()

    def check():
        assert g.capacity == len(gen) and [g.slot_generation(s) for s in range(g.capacity)] == [gen[s] for s in range(len(gen))]
        dev = g.slot_generations()
        assert dev.dtype == torch.int32 and dev.tolist() == [gen[s] for s in range(len(gen))] and min(dev.tolist()) >= 1
        assert {g.slot_of(c): c for c in g.class_ids} == {s: c for s, (c, _) in owner.items()}
        for s, (c, reg) in owner.items():
            assert held.setdefault(s, {}).setdefault(gen[s], reg) == reg, (s, c, gen[s])

    def register(ids):
        nonlocal registration, grew
        plan = plan_add(g._book, ids)
        grew += plan.book.cap > g.capacity
        for s in range(len(gen), plan.book.cap):
            gen[s] = 1
        g._ensure_store(plan.book.cap)            # as _register_sequences: the store follows the book
        g._install(plan.book)
        for c, s in zip(ids, plan.slots):
            registration += 1
            owner[s] = (c, registration)

    check()
    for step in range(500):
        op = rng.random()
        ids = g.class_ids
        if op < 0.35:
            n = rng.randint(1, 3)
            if ids and rng.random() < 0.3:        # a class that was there before comes back (after its removal below), among new ones
                back = rng.choice(ids)
                slot = g.slot_of(back)
                g.remove_classes([back])
                gen[slot] += 1
                del owner[slot]
                check()
                new = [back] + list(range(next_id, next_id + n - 1))
            else:
                new = list(range(next_id, next_id + n))
            next_id += n
            register(new)
            ops.add("add")
        elif op < 0.6 and ids:
            gone = rng.sample(ids, rng.randint(1, min(3, len(ids))))
            plan = plan_remove(g._book, gone)
            for s in plan.slots:
                gen[s] += 1
                del owner[s]
            g.remove_classes(gone)
            ops.add("remove")
        elif op < 0.8 and ids:
            g._book = plan_shots(g._book, [rng.choice(ids) for _ in range(rng.randint(1, 4))]).book      # as _shots_sequences installs
            ops.add("shots")
        elif op < 0.85:
            g.clear()
            gen = {s: v + 1 for s, v in gen.items()}
            owner = {}
            ops.add("clear")
        elif op < 0.9 and ids:
            keep = rng.sample(ids, rng.randint(1, len(ids)))
            g._ensure_store(g.capacity)           # (a gallery that registered on the device has it)
            sd = g.state_dict()
            at = torch.tensor([sd["class_ids"].index(c) for c in keep])
            sub = {k: (v[at] if isinstance(v, torch.Tensor) and k != "norms" else v) for k, v in sd.items()}
            sub["class_ids"], sub["counts"] = keep, [sd["counts"][i] for i in at.tolist()]
            sub["norms"] = sd["norms"].view(len(ids), -1)[at].reshape(-1)
            g.load_state_dict(sub)
            gen = {s: v + 1 for s, v in gen.items()}
            owner = {}
            for s, c in enumerate(keep):          # a load fills the lowest slots in the state's order
                registration += 1
                owner[s] = (c, registration)
            ops.add("load")
        check()
    assert ops == {"add", "remove", "shots", "clear", "load"} and grew >= 2, (ops, grew)


# ------------------------------------------------------------------ StreamPool's option, on stub heads
def test_smooth_by_on_stub_heads():
    import torch
    from clip_fsar_amd.gallery import SupportGallery
    from clip_fsar_amd.pool import GroupedPackedOutput, StreamPool
    from clip_fsar_amd.text_gallery import TextGallery
    live = _live("live", 4)
    p = StreamPool(live, max_streams=3, smooth=0.5, smooth_by="class")            # TypeError without the feature
    assert p.smooth_by == "class" and p.alpha == 0.5 and p._state is None and p._smooth_cells.planes is None
    assert StreamPool(_live("live_text", 4), smooth=0.25, smooth_by="class").smooth_by == "class"
    assert StreamPool(live, smooth=0.5).smooth_by == "column" == StreamPool(live, smooth=0.5, smooth_by="column").smooth_by
    for g in (SupportGallery(_stub_head(), "cpu"), TextGallery(_stub_head(COMBINE=True), "cpu")):
        for smooth in (0.5, 0.0):
            with pytest.raises(ValueError, match="slot store.*%s" % type(g).__name__):
                StreamPool(g, smooth=smooth, smooth_by="class")
    for bad in ("rows", "", None, "Class", 1):
        with pytest.raises(ValueError, match="smooth_by"):
            StreamPool(live, smooth=0.5, smooth_by=bad)
    with pytest.raises(ValueError, match="2\\^31"):
        StreamPool(_live("live", 1 << 15), max_streams=1 << 16, smooth=0.5, smooth_by="class")
    inert = StreamPool(live, smooth=0.0, smooth_by="class")                       # smooth = 0: nothing of the class mode is there
    assert inert._by_class is False and inert._state is None and inert._smooth_cells is None
    # six-argument construction of the grouped output keeps working; the new field trails and defaults to None
    out = GroupedPackedOutput([0], [0], [0, 0], torch.zeros(0), [0, 0], [2])
    assert out.smoothed is None and GroupedPackedOutput._fields[-1] == "smoothed" and len(GroupedPackedOutput._fields) == 7
    # class lists: accepted in class mode; the column mode keeps its refusal, word for word
    from clip_fsar_amd.live_gallery import plan_add
    live._install(plan_add(live._book, [9, 2, 4]).book)
    h = p.open(classes=[9, 2])
    assert p._sessions[h].classes == [9, 2]
    with pytest.raises(ValueError, match="class 5 is not registered"):
        p.open(classes=[5])
    with pytest.raises(ValueError, match="smoothing with per-session class lists is out of scope; build the pool with smooth = 0"):
        StreamPool(live, smooth=0.5).open(classes=[9, 2])
    # a listed class that left: the existing error, in class mode too, before any launch
    live.remove_classes([2])
    with pytest.raises(ValueError, match="session %d.*class 2 is not registered" % h):
        p._check_state([h], [p._sessions[h]])


def test_the_column_mode_keeps_its_guards():
    """the default mode's two stale-state errors with their texts (the third, class lists, is above): state made at another class count,
    and state made before a removal"""
    from clip_fsar_amd.live_gallery import plan_add
    from clip_fsar_amd.pool import StreamPool
    live = _live("live", 8)
    live._install(plan_add(live._book, [0, 1, 2]).book)
    for by_class in (False, True):
        pool = StreamPool(live, smooth=0.5, **({"smooth_by": "class"} if by_class else {}))
        h = pool.open()
        s = pool._sessions[h]
        pool._state, s.state_gen, s.state_layout = NS(shape=(64, 2)), pool._state_gen, live.layout_version       # made with 2 classes
        if by_class:
            pool._check_state([h], [s])
            continue
        with pytest.raises(RuntimeError, match=r"the gallery has 3 classes, the smoothing state of session 0 was made with another count "
                                               r"-- reset\(\) the session after adding classes when smoothing is on"):
            pool._check_state([h], [s])
        pool._state, s.state_layout = NS(shape=(64, 3)), live.layout_version - 1
        with pytest.raises(RuntimeError, match=r"classes were removed from the gallery since the smoothing state of session 0 was made, "
                                               r"its columns mean other classes now -- reset\(\) the session after removing classes"):
            pool._check_state([h], [s])
