"""CPU: the grouped-scoring library (libclipfsar_groups.so, include/clipfsar_groups.h) validates its descriptor table without a GPU;
LiveGallery.plan_groups against a list model; misuse of the grouped calls of LiveGallery and StreamPool on a stub head.  Its exports,
kernels and place in the build are checked with every library's in tests/test_build_recipe.py."""
import ctypes
import os
import random
import re
from types import SimpleNamespace as NS

import pytest

from _abi import _prototypes, check_abi_at_load, check_exports, lib_row

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "clipfsar_groups.h")


@pytest.fixture(scope="module")
def glib():
    import __graft_entry__ as ge
    ge.build()                                    # builds every library (no-op when up to date)
    from clip_fsar_amd import groups_hip
    return groups_hip.lib()


def test_header_exported_exactly_and_arity_matches(glib):
    check_exports(lib_row("groups"))                 # the checks every library gets; below, what is particular to this one
    from clip_fsar_amd import groups_hip as gh
    protos = _prototypes(HEADER, "cfgr_")
    assert protos["cfgr_otam_grouped"] == 18 and protos["cfgr_topk_grouped"] == 10
    text = open(HEADER).read()
    assert int(re.search(r"#define CFGR_MAX_T (\d+)", text).group(1)) == gh.MAX_T == 32
    assert int(re.search(r"#define CFGR_MAX_GROUPS (\d+)", text).group(1)) == gh.MAX_GROUPS
    assert int(re.search(r"#define CFGR_TOPK_MAX (\d+)", text).group(1)) == gh.TOPK_MAX == 16
    assert int(re.search(r"#define CFGR_TABLE_COLS (\d+)", text).group(1)) == gh.TABLE_COLS == 6
    for i, col in enumerate(("Q0", "NQ", "C0", "NC", "TILE0", "OUT0")):          # the binding's column order is the header's
        assert int(re.search(r"#define CFGR_%s (\d+)" % col, text).group(1)) == getattr(gh, col) == i


def test_abi_version_is_checked_at_load(glib, monkeypatch):
    check_abi_at_load(lib_row("groups"), monkeypatch)


# ------------------------------------------------------------------ table validation, without a GPU
def _tbl(rows):
    flat = [v for r in rows for v in r]
    return (ctypes.c_int32 * len(flat))(*flat)


#        Q0 NQ  C0  NC TILE0 OUT0          T = 8: QB = 8
GOOD = [[0,  1,  0,  1,  0,    0],       # 1 x 1 tiles
        [1,  9,  1,  8,  1,    1],       # 2 x 1
        [10, 0,  9,  3,  3,   73],       # no queries: no tiles, no logits
        [10, 17, 12, 65, 3,   73]]       # 3 x 9
NQ, NCOLS, NOUT = 27, 77, 73 + 17 * 65


def _edit(row, col, value):
    rows = [list(r) for r in GOOD]
    rows[row][col] = value
    return _tbl(rows)


def test_good_table_is_what_the_binding_plans():
    from clip_fsar_amd import groups_hip as gh
    rows, totals = gh.table_rows([1, 9, 0, 17], [1, 8, 3, 65], 8)
    assert rows == GOOD and totals == (NQ, NCOLS, 3 + 27, NOUT)
    assert [gh.tile_videos(T) for T in (1, 2, 4, 5, 8, 16, 32)] == [16, 16, 16, 12, 8, 4, 2]


def test_table_validation_without_gpu(glib):
    p = ctypes.c_void_p(4096)                     # never dereferenced: every call below fails validation before any device work
    err, good = glib.cfgr_last_error, _tbl(GOOD)

    # otam_grouped(Xq, qn, P_store, pn_store, cols, logits, table_host, table_dev, G, NQ, NCOLS, NOUT, cap, T, E, lambda, sd, stream)
    def otam(table=good, G=4, nq=NQ, ncols=NCOLS, nout=NOUT, cap=70, T=8, E=64, lbda=0.5, **ptr):
        a = dict(Xq=p, qn=p, P=p, pn=p, cols=p, logits=p, tdev=p)
        a.update(ptr)
        return glib.cfgr_otam_grouped(a["Xq"], a["qn"], a["P"], a["pn"], a["cols"], a["logits"], table, a["tdev"], G, nq, ncols, nout, cap,
                                      T, E, lbda, 0, None)

    for name in ("Xq", "qn", "P", "pn", "cols", "logits", "tdev"):
        assert otam(**{name: None}) != 0 and b"null" in err(), name
    assert otam(table=None) != 0 and b"null" in err()
    for kw in ({"T": 0}, {"T": 33}, {"E": 66}, {"E": 0}, {"E": 8196}, {"cap": 0}, {"nq": 0}, {"ncols": 0}, {"nout": 0}):
        assert otam(**kw) != 0 and b"bad shape" in err(), kw
    assert otam(cap=1 << 27, T=32) != 0 and b"32-bit" in err()
    assert otam(lbda=0.0) != 0 and b"lambda" in err()
    assert otam(Xq=ctypes.c_void_p(4100)) != 0 and b"16-byte aligned" in err()
    assert otam(P=ctypes.c_void_p(4104)) != 0 and b"16-byte aligned" in err()
    for G in (0, -1, (1 << 16) + 1):
        assert otam(G=G) != 0 and b"groups" in err(), G
    # each prefix column, once per row it can be wrong in
    for col in (0, 2, 4, 5):
        for row in (0, 1, 3):
            assert otam(table=_edit(row, col, GOOD[row][col] + 1)) != 0 and b"prefix sums" in err(), (row, col)
    assert otam(table=_edit(2, 4, 2)) != 0 and b"prefix sums" in err()         # TILE0 of the group without queries
    assert otam(table=_edit(1, 1, 8)) != 0 and b"prefix sums" in err()         # a count its successor's offsets contradict
    assert otam(T=16) != 0 and b"prefix sums" in err()                         # TILE0 was made for QB = 8, T = 16 has QB = 4
    assert otam(table=_edit(2, 3, 0)) != 0 and b"at least 1" in err()          # NC = 0
    assert otam(table=_edit(0, 3, -2)) != 0 and b"at least 1" in err()
    assert otam(table=_edit(1, 1, -1)) != 0 and b"negative" in err()
    # totals
    assert otam(nq=NQ + 1) != 0 and b"not to NQ" in err()
    assert otam(G=3, nout=73) != 0 and b"not to NQ" in err()
    assert otam(ncols=NCOLS - 1) != 0 and b"not to NCOLS" in err()
    assert otam(nout=NOUT + 1) != 0 and b"not to NOUT" in err()
    # 32-bit: a group of 65536 x 65536 logits
    big = _tbl([[0, 65536, 0, 65536, 0, 0], [65536, 1, 65536, 1, 0, 0]])
    assert otam(table=big, G=2, nq=65537, ncols=65537, nout=1, cap=1 << 20) != 0 and b"32-bit" in err()

    # topk_grouped(logits, table_host, table_dev, G, NQ, NOUT, k, values, index, stream)
    def topk(table=good, G=4, nq=NQ, nout=NOUT, k=1, logits=p, tdev=p, values=p, index=p):
        return glib.cfgr_topk_grouped(logits, table, tdev, G, nq, nout, k, values, index, None)

    for kw in ({"logits": None}, {"table": None}, {"tdev": None}, {"values": None}, {"index": None}):
        assert topk(**kw) != 0 and b"null" in err(), kw
    for kw in ({"nq": 0}, {"nout": 0}):
        assert topk(**kw) != 0 and b"bad shape" in err(), kw
    for k in (0, -1, 2, 17):                                                   # group 0 has queries and one slot
        assert topk(k=k) != 0 and b"smallest NC" in err(), k
    wide = [[0, 2, 0, 20, 0, 0], [2, 0, 20, 3, 1, 40], [2, 1, 23, 18, 1, 40]]    # the narrow group has no queries
    assert topk(table=_tbl(wide), G=3, nq=3, nout=58, k=17) != 0 and b"smallest NC" in err()
    assert topk(table=_tbl(wide), G=3, nq=3, nout=58, k=19) != 0 and b"smallest NC" in err()
    for col in (0, 2, 5):
        assert topk(table=_edit(3, col, GOOD[3][col] - 1)) != 0 and b"prefix sums" in err(), col
    assert topk(table=_edit(3, 3, 0)) != 0 and b"at least 1" in err()
    assert topk(nq=NQ - 1) != 0 and b"not to NQ" in err()
    assert topk(nout=NOUT - 1) != 0 and b"not to NOUT" in err()
    assert topk(table=_tbl([[0, 1, 0, 65536, 0, 0]]), G=1, nq=1, nout=65536) != 0 and b"65535" in err()


def test_python_wrappers_reject_cpu_tensors_and_bad_shapes(glib):
    import torch
    from clip_fsar_amd import groups_hip as gh
    from clip_fsar_amd import pool_hip as ph
    host = torch.tensor(GOOD, dtype=torch.int32)
    table = ph.Table(host, host, 4)               # a device copy that is no device tensor
    Xq, qn, P, pn = torch.zeros(NQ, 8, 64), torch.zeros(NQ * 8), torch.zeros(70, 8, 64), torch.zeros(70 * 8)
    cols, out = torch.zeros(NCOLS, dtype=torch.int32), torch.zeros(NOUT)
    with pytest.raises(RuntimeError, match="HIP device tensor"):
        gh.otam_grouped(Xq, qn, P, pn, cols, out, table, NOUT)
    with pytest.raises(RuntimeError, match="logits has shape"):
        gh.otam_grouped(Xq, qn, P, pn, cols, out[:-1], table, NOUT)
    with pytest.raises(RuntimeError, match="shape"):
        gh.otam_grouped(Xq, qn[:-1], P, pn, cols, out, table, NOUT)
    with pytest.raises(RuntimeError, match="Table"):
        gh.otam_grouped(Xq, qn, P, pn, cols, out, ph.Table(host[:, :4], host, 4), NOUT)
    with pytest.raises(RuntimeError, match="HIP device tensor"):
        gh.topk_grouped(out, table, NQ, NOUT, 1, torch.zeros(NQ, 1), torch.zeros(NQ, 1, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="shape"):
        gh.topk_grouped(out, table, NQ, NOUT, 1, torch.zeros(NQ, 2), torch.zeros(NQ, 1, dtype=torch.int32))
    assert gh.table_uploader("cpu", 4).cols == gh.TABLE_COLS


# ------------------------------------------------------------------ plan_groups against a list model
def _model(slot_of, order, counts, classes, qb):
    """the plainest statement of the table: walk the groups, keep four running sums"""
    rows, slots, q, c, t, o = [], [], 0, 0, 0, 0
    for n, ids in zip(counts, classes):
        ids = list(order) if ids is None else ids
        rows.append([q, n, c, len(ids), t, o])
        slots += [slot_of[i] for i in ids]
        q, c, o = q + n, c + len(ids), o + n * len(ids)
        t += ((n + qb - 1) // qb) * ((len(ids) + qb - 1) // qb)
    return rows, slots, o


@pytest.mark.parametrize("seed", range(6))
def test_plan_groups_against_a_model_on_random_books(seed):
    from clip_fsar_amd import groups_hip as gh
    from clip_fsar_amd import live_gallery as lg
    rng = random.Random(seed)
    book, next_id = lg.new_book(rng.choice([1, 3, 8])), 0
    for step in range(60):
        ids = list(range(next_id, next_id + rng.randint(1, 6)))
        next_id += len(ids)
        book = lg.plan_add(book, ids).book
        if len(book.order) > 3 and rng.random() < 0.5:
            book = lg.plan_remove(book, rng.sample(book.order, rng.randint(1, 2))).book
        T = rng.choice([1, 5, 8, 16, 32])
        G = rng.randint(1, 12)
        counts = [rng.choice([0, 1, 2, 7, 8, 9, 33]) for _ in range(G)]
        classes = [None if rng.random() < 0.2 else rng.sample(book.order, rng.randint(1, len(book.order))) for _ in range(G)]
        plan = lg.plan_groups(book, counts, classes, T)
        assert (plan.rows, plan.slots, plan.n_out) == _model(book.slot_of, book.order, counts, classes, gh.tile_videos(T))
        # a chunk of the queries is a table of its own over slices of the lists and of the logits
        N = sum(counts)
        if N:
            q0 = rng.randrange(N)
            q1 = rng.randint(q0 + 1, N)
            sub, (c_lo, c_hi), out_lo = lg.chunk_groups(plan.rows, q0, q1, T)
            flat = [(g, i) for g, n in enumerate(counts) for i in range(n)][q0:q1]      # (group, query in it) of the chunk's queries
            assert sum(r[gh.NQ] for r in sub) == q1 - q0 and c_hi - c_lo == sum(r[gh.NC] for r in sub)
            assert sub == gh.table_rows([r[gh.NQ] for r in sub], [r[gh.NC] for r in sub], T)[0]
            at = 0
            for r in sub:
                for i in range(r[gh.NQ]):
                    g, qi = flat[at]
                    at += 1
                    assert plan.slots[c_lo + r[gh.C0]:c_lo + r[gh.C0] + r[gh.NC]] == \
                        plan.slots[plan.rows[g][gh.C0]:plan.rows[g][gh.C0] + plan.rows[g][gh.NC]]
                    assert out_lo + r[gh.OUT0] + i * r[gh.NC] == plan.rows[g][gh.OUT0] + qi * plan.rows[g][gh.NC]
        before = (book.cap, list(book.free), list(book.order), dict(book.slot_of))
        known = book.order[0]
        with pytest.raises(ValueError, match="group 1: class 'nobody' is not registered"):
            lg.plan_groups(book, [1, 1], [[known], [known, "nobody"]], T)
        with pytest.raises(ValueError, match="group 0: a class appears twice"):
            lg.plan_groups(book, [1], [[known, known]], T)
        with pytest.raises(ValueError, match="group 1: classes= needs at least one class"):
            lg.plan_groups(book, [1, 1], [None, []], T)
        with pytest.raises(ValueError, match=">= 0"):
            lg.plan_groups(book, [1, -1], [None, None], T)
        with pytest.raises(ValueError, match=">= 0"):
            lg.plan_groups(book, [1.5], [None], T)
        with pytest.raises(ValueError, match="one count for each"):
            lg.plan_groups(book, [1, 2], [None], T)
        with pytest.raises(ValueError, match="one count for each"):
            lg.plan_groups(book, [], [], T)
        assert (book.cap, book.free, book.order, book.slot_of) == before
    with pytest.raises(ValueError, match="group 0: classes= needs at least one class"):
        lg.plan_groups(lg.new_book(2), [1], [None], 8)          # None on a book without classes


# ------------------------------------------------------------------ LiveGallery and StreamPool on a stub head: misuse, before any launch
def _stub_head(T=4, **train):
    engine = NS(arch={"embed": 8})
    return NS(args=NS(TRAIN=NS(**train), DATA=NS(NUM_INPUT_FRAMES=T)), _get_engine=lambda dev: engine, _engine_key=("stub",),
              arch_name="stub", precision="fp32", depth=1)


def _stub_gallery(ids=("a", "b", "c")):
    from clip_fsar_amd import live_gallery as lg
    g = lg.LiveGallery(_stub_head(), "cpu", capacity=4)
    if ids:
        g._install(lg.plan_add(g._book, list(ids)).book)       # registered on the host alone: nothing below reaches the device
    return g


def test_live_gallery_rejects_grouped_misuse_before_any_launch():
    import torch
    clips, feats = torch.zeros(3, 4, 3, 8, 8), torch.zeros(3, 4, 8)
    empty = _stub_gallery(ids=())
    with pytest.raises(RuntimeError, match="no classes registered"):
        empty.classify_grouped(clips, [3], [None])
    g = _stub_gallery()
    for call, src in ((g.classify_grouped, clips), (g.classify_features_grouped, feats)):
        with pytest.raises(ValueError, match="group 1: class 'z' is not registered"):
            call(src, [1, 2], [["a"], ["z"]])
        with pytest.raises(ValueError, match="appears twice"):
            call(src, [3], [["a", "a"]])
        with pytest.raises(ValueError, match="at least one class"):
            call(src, [3], [[]])
        with pytest.raises(ValueError, match=">= 0"):
            call(src, [4, -1], [None, None])
        with pytest.raises(ValueError, match="one count for each"):
            call(src, [3], [None, None])
        with pytest.raises(RuntimeError, match="no CPU path"):
            call(src, [1, 2], [["b", "a"], None])
    for k in (0, 3, 17, True, 1.0):                            # the shortest list of a group with clips has 2 classes
        with pytest.raises(ValueError, match="shortest class list"):
            g.topk_grouped(clips, [2, 0, 1], [["a", "b"], ["c"], None], k=k)
    with pytest.raises(RuntimeError, match="no CPU path"):
        g.topk_grouped(clips, [2, 0, 1], [["a", "b"], ["c"], None], k=2)
    assert g._store is None and g._group_tables is None and g._group_cols == (None, None)


def test_live_gallery_counts_must_add_up_to_the_clips():
    import torch
    from clip_fsar_amd import live_gallery as lg
    g = _stub_gallery()
    ok = torch.zeros(3, 4, 8)
    g._check_feats = lambda feats: feats                       # the device check aside: what follows it, still before any launch
    with pytest.raises(ValueError, match="add up to 2, the call holds 3"):
        g.classify_features_grouped(ok, [1, 1], [None, ["a"]])
    with pytest.raises(ValueError, match="at least 1 is needed"):
        g.classify_features_grouped(ok[:0], [0, 0], [None, ["a"]])
    r = lg.GroupedLogits(torch.arange(11.), [0, 6, 6, 11], [3, 2, 5], [2, 0, 1])
    assert len(r) == 3 and r.group(0).tolist() == [[0, 1, 2], [3, 4, 5]] and tuple(r.group(1).shape) == (0, 2)
    assert r.group(2).tolist() == [[6, 7, 8, 9, 10]]


def test_stream_pool_rejects_class_list_misuse_before_any_launch():
    import torch
    from clip_fsar_amd.gallery import SupportGallery
    from clip_fsar_amd.pool import GroupedPackedOutput, PackedOutput, StreamPool
    g = _stub_gallery()
    with pytest.raises(ValueError, match="needs a gallery that scores groups"):
        StreamPool(SupportGallery(_stub_head(), "cpu"), max_streams=2).open(classes=[1])
    with pytest.raises(ValueError, match="smooth > 0 is not supported"):
        StreamPool(g, max_streams=2, smooth=0.5).open(classes=["a"])
    p = StreamPool(g, max_streams=2)
    with pytest.raises(ValueError, match="session 0: class 'z' is not registered"):
        p.open(classes=["a", "z"])
    with pytest.raises(ValueError, match="session 0: a class appears twice"):
        p.open(classes=["a", "a"])
    with pytest.raises(ValueError, match="session 0: classes= needs at least one class"):
        p.open(classes=[])
    assert p.sessions == [] and p.stats()["open"] == 0          # a refused open() takes no slot and no handle
    a, b = p.open(classes=("c", "a")), p.open()
    assert (a, b) == (0, 1) and p._sessions[a].classes == ["c", "a"] and p._sessions[b].classes is None
    p.reset(a)
    assert p._sessions[a].classes == ["c", "a"]                  # reset() keeps the list
    p._check_state([a, b], [p._sessions[a], p._sessions[b]])
    g.remove_classes(["c"])                                      # the class leaves while the session is open
    with pytest.raises(ValueError, match="session 0: class 'c' is not registered"):
        p._check_state([b, a], [p._sessions[b], p._sessions[a]])
    p.close(a)
    assert p.open(classes=["b"]) == 2 and p._sessions[2].slot == 0 and p._sessions[2].classes == ["b"]      # the reused slot, another list
    assert PackedOutput._fields == ("sessions", "first_window", "offsets", "logits", "smoothed")            # unchanged
    # top-k of a grouped output: k against the shortest list of a session with windows, before any launch
    po = GroupedPackedOutput([b, 2], [0, 0], [0, 0, 2], torch.zeros(2), [0, 0, 2], [2, 1])
    for k in (0, 2, 17):
        with pytest.raises(ValueError, match="shortest class list"):
            p.topk(po, k=k)
    with pytest.raises(ValueError, match="no smoothed scores"):
        p.topk(po, k=1, smoothed=True)
    none = GroupedPackedOutput([b], [0], [0, 0], torch.zeros(0), [0, 0], [2])
    values, index = p.topk(none, k=2)
    assert tuple(values.shape) == (0, 2) and index.dtype == torch.int32
    out = StreamPool._split(GroupedPackedOutput([b, 2], [3, 0], [0, 2, 3], torch.arange(5.), [0, 4, 5], [2, 1]))
    assert out[b].first_window == 3 and out[b].logits.tolist() == [[0, 1], [2, 3]] and out[2].logits.tolist() == [[4]]
    assert out[b].smoothed is None
