"""CPU: the live-gallery library (libclipfsar_live.so, include/clipfsar_live.h) validates arguments and descriptor tables without a GPU;
LiveGallery's slot and column bookkeeping (the plan_* functions) against a model on random schedules.  Its exports, kernels and place in the
build are checked with every library's in tests/test_build_recipe.py."""
import ctypes
import os
import random
import re
from types import SimpleNamespace as NS

import pytest

from _abi import check_abi_at_load, check_exports, lib_row

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "clipfsar_live.h")


@pytest.fixture(scope="module")
def llib():
    import __graft_entry__ as ge
    ge.build()                                    # builds every library (no-op when up to date)
    from clip_fsar_amd import live_hip
    return live_hip.lib()


def test_header_exported_exactly_and_arity_matches(llib):
    check_exports(lib_row("live"))                 # the checks every library gets; below, what is particular to this one
    from clip_fsar_amd import live_hip as lh
    text = open(HEADER).read()
    assert int(re.search(r"#define CFSL_MAX_T (\d+)", text).group(1)) == lh.MAX_T == 32
    assert int(re.search(r"#define CFSL_MAX_ROWS (\d+)", text).group(1)) == lh.MAX_ROWS
    assert int(re.search(r"#define CFSL_TABLE_COLS (\d+)", text).group(1)) == lh.TABLE_COLS == 4
    for i, col in enumerate(("SLOT", "OFF", "N", "PRIOR")):          # the binding's column order is the header's
        assert int(re.search(r"#define CFSL_%s (\d+)" % col, text).group(1)) == getattr(lh, col) == i


def test_abi_version_is_checked_at_load(llib, monkeypatch):
    check_abi_at_load(lib_row("live"), monkeypatch)


# ------------------------------------------------------------------ validation, without a GPU
def _tbl(rows):
    flat = [v for r in rows for v in r]
    return (ctypes.c_int32 * len(flat))(*flat)


#        slot off n prior
GOOD = [[5,   0,  3, 0],
        [0,   3,  1, 2],
        [6,   4,  5, 0],
        [2,   9,  2, 7]]          # Nv = 11, cap = 8


def _edit(row, col, value):
    rows = [list(r) for r in GOOD]
    rows[row][col] = value
    return _tbl(rows)


def test_argument_validation_without_gpu(llib):
    p = ctypes.c_void_p(4096)                     # never dereferenced: every call below fails validation before any device work
    err, good = llib.cfsl_last_error, _tbl(GOOD)

    # otam_indexed(Xq, qn, P_store, pn_store, cols, logits, NQ, C, cap, T, E, lambda, single_direct, stream)
    def otam(NQ=4, C=3, cap=8, T=8, E=64, lbda=0.5, **ptr):
        a = dict(Xq=p, qn=p, P=p, pn=p, cols=p, logits=p)
        a.update(ptr)
        return llib.cfsl_otam_indexed(a["Xq"], a["qn"], a["P"], a["pn"], a["cols"], a["logits"], NQ, C, cap, T, E, lbda, 0, None)

    for name in ("Xq", "qn", "P", "pn", "cols", "logits"):
        assert otam(**{name: None}) != 0 and b"null" in err(), name
    for kw in ({"T": 0}, {"T": 33}, {"E": 66}, {"E": 0}, {"E": 8196}, {"C": 0}, {"cap": 0}, {"NQ": 0}, {"C": -1}):
        assert otam(**kw) != 0 and b"bad shape" in err(), kw
    assert otam(cap=1 << 27, T=32) != 0 and b"32-bit" in err()
    assert otam(NQ=1 << 28, T=16) != 0 and b"32-bit" in err()
    assert otam(lbda=0.0) != 0 and b"lambda" in err()
    assert otam(NQ=65536 * 8, T=8) != 0 and b"too large for one launch" in err()

    # accumulate(X, sums, means, table_host, table_dev, S, Nv, L, E, cap, rows_kept, means_by_slot, stream)
    def acc(table=good, S=4, Nv=11, L=9, E=64, cap=8, rows_kept=8, X=p, sums=p, means=p, tdev=p):
        return llib.cfsl_accumulate(X, sums, means, table, tdev, S, Nv, L, E, cap, rows_kept, 1, None)

    for kw in ({"X": None}, {"sums": None}, {"means": None}, {"table": None}, {"tdev": None}):
        assert acc(**kw) != 0 and b"null" in err(), kw
    for kw in ({"Nv": 0}, {"L": 0}, {"E": 0}, {"cap": 0}, {"rows_kept": 0}, {"rows_kept": 10}):
        assert acc(**kw) != 0 and b"bad shape" in err(), kw
    for S in (0, -1, 9, 1 << 17):
        assert acc(S=S, cap=8 if S < 100 else 1 << 20) != 0 and b"rows" in err(), S
    assert acc(table=_edit(1, 0, 8)) != 0 and b"outside [0, 8)" in err()
    assert acc(table=_edit(1, 0, -1)) != 0 and b"outside" in err()
    assert acc(cap=6) != 0 and b"outside [0, 6)" in err()
    assert acc(table=_edit(3, 0, 5)) != 0 and b"appears twice" in err()
    assert acc(table=_edit(2, 2, 0)) != 0 and b"at least 1" in err()
    assert acc(table=_edit(2, 2, -4)) != 0 and b"at least 1" in err()
    assert acc(table=_edit(1, 3, -1)) != 0 and b"prior" in err()
    for row, v in ((0, 1), (1, 2), (3, 10)):                                                     # an offset that is not the running sum
        assert acc(table=_edit(row, 1, v)) != 0 and b"prefix sum" in err(), (row, v)
    assert acc(table=_edit(1, 2, 2)) != 0 and b"prefix sum" in err()                             # a count its successor's offset contradicts
    assert acc(Nv=12) != 0 and b"not to Nv" in err()
    assert acc(S=3) != 0 and b"not to Nv" in err()
    assert acc(table=_edit(3, 3, 0x7fffffff)) != 0 and b"32-bit" in err()

    # slot_norms(P_store, pn_store, table_host, table_dev, S, cap, T, E, stream)
    def norms(table=good, S=4, cap=8, T=8, E=64, P=p, pn=p, tdev=p):
        return llib.cfsl_slot_norms(P, pn, table, tdev, S, cap, T, E, None)

    for kw in ({"P": None}, {"pn": None}, {"table": None}, {"tdev": None}):
        assert norms(**kw) != 0 and b"null" in err(), kw
    for kw in ({"cap": 0}, {"T": 0}, {"E": 0}):
        assert norms(**kw) != 0 and b"bad shape" in err(), kw
    assert norms(table=_edit(0, 0, 9)) != 0 and b"outside" in err()
    assert norms(table=_edit(0, 0, 2)) != 0 and b"appears twice" in err()
    assert norms(cap=1 << 27, T=32) != 0 and b"32-bit" in err()


def test_python_wrappers_reject_cpu_tensors_and_bad_tables(llib):
    import torch
    from clip_fsar_amd import live_hip as lh
    from clip_fsar_amd import pool_hip as ph
    host = torch.tensor(GOOD, dtype=torch.int32)
    table = ph.Table(host, host, 4)               # a device copy that is no device tensor
    X, sums, P = torch.zeros(11, 9, 64), torch.zeros(8, 9, 64), torch.zeros(8, 8, 64)
    with pytest.raises(RuntimeError, match="HIP device tensor"):
        lh.accumulate(X, sums, P, table, by_slot=True)
    with pytest.raises(RuntimeError, match="shape"):
        lh.accumulate(X, torch.zeros(8, 8, 64), P, table, by_slot=True)
    with pytest.raises(RuntimeError, match="means must be"):
        lh.accumulate(X, sums, P, table, by_slot=False)          # packed means have one entry per table row
    with pytest.raises(RuntimeError, match="Table"):
        lh.accumulate(X, sums, P, ph.Table(host[:, :3], host, 4), by_slot=True)
    with pytest.raises(RuntimeError, match="HIP device tensor"):
        lh.slot_norms(P, torch.zeros(64), table)
    with pytest.raises(RuntimeError, match="shape"):
        lh.slot_norms(P, torch.zeros(63), table)
    with pytest.raises(RuntimeError, match="HIP device tensor"):
        lh.otam_indexed(torch.zeros(2, 8, 64), torch.zeros(16), P, torch.zeros(64), torch.zeros(3, dtype=torch.int32), torch.zeros(2, 3))
    with pytest.raises(RuntimeError, match="shape"):
        lh.otam_indexed(torch.zeros(2, 8, 64), torch.zeros(16), P, torch.zeros(64), torch.zeros(3, dtype=torch.int32), torch.zeros(2, 4))
    up = lh.table_uploader("cpu", 4)
    assert up.cols == lh.TABLE_COLS
    with pytest.raises(RuntimeError, match="1 .. 4 rows of 4"):
        up.upload([[0] * 8])


# ------------------------------------------------------------------ the bookkeeping against a model
class _Model:
    """the plainest statement of the rules: a list of slots (None = free), the columns as a list of ids"""

    def __init__(self, cap):
        self.slots, self.order, self.shots, self.version = [None] * cap, [], {}, 0

    def add(self, ids, counts):
        out = []
        for c, k in zip(ids, counts):
            if None not in self.slots:
                cap = len(self.slots)
                self.slots += [None] * (max(cap + 1, cap * 3 // 2) - cap)
            s = self.slots.index(None)             # the lowest free slot
            self.slots[s] = c
            self.order.append(c)
            self.shots[c] = k
            out.append(s)
        return out

    def remove(self, ids):
        for c in ids:
            self.slots[self.slots.index(c)] = None
            self.order.remove(c)
            del self.shots[c]
        self.version += 1


def _same(book, m):
    assert book.cap == len(m.slots) and sorted(book.free) == [i for i, c in enumerate(m.slots) if c is None]
    assert book.order == m.order and book.shots == m.shots and book.version == m.version
    assert book.slot_of == {c: i for i, c in enumerate(m.slots) if c is not None}


@pytest.mark.parametrize("seed", range(6))
def test_bookkeeping_against_a_model_on_random_schedules(seed):
    from clip_fsar_amd import live_gallery as lg
    rng = random.Random(seed)
    cap0 = rng.choice([1, 2, 3, 8])
    book, m, next_id = lg.new_book(cap0), _Model(cap0), 0
    for step in range(300):
        op = rng.choice(["add", "add", "remove", "shots", "columns", "bad"])
        before = (book.cap, list(book.free), list(book.order), dict(book.slot_of), dict(book.shots), book.version)
        if op == "add":
            ids = list(range(next_id, next_id + rng.randint(1, 5)))
            next_id += len(ids)
            counts = [rng.randint(1, 4) for _ in ids]
            plan = lg.plan_add(book, ids, counts)
            # growth in one step: the model grows slot by slot as it runs full, the plan all at once -- to the same capacity only
            # when growing is deferred until the store is full, which is what both do
            assert plan.slots == m.add(ids, counts)
            book = plan.book
        elif op == "remove" and m.order:
            ids = rng.sample(m.order, rng.randint(1, min(3, len(m.order))))
            plan = lg.plan_remove(book, ids)
            assert plan.slots == [m.slots.index(c) for c in ids]
            m.remove(ids)
            book = plan.book
        elif op == "shots" and m.order:
            vids = [rng.choice(m.order) for _ in range(rng.randint(1, 6))]
            plan = lg.plan_shots(book, vids)
            assert plan.classes == list(dict.fromkeys(vids))
            off = 0
            for c, row in zip(plan.classes, plan.rows):
                assert row == (m.slots.index(c), off, vids.count(c), m.shots[c])
                off += vids.count(c)
                m.shots[c] += vids.count(c)
            assert off == len(vids)
            book = plan.book
        elif op == "columns" and m.order:
            assert lg.plan_columns(book) == [m.slots.index(c) for c in m.order]
            sub = rng.sample(m.order, rng.randint(1, len(m.order)))
            assert lg.plan_columns(book, sub) == [m.slots.index(c) for c in sub]
        elif op == "bad":                          # a failed call changes nothing
            known = m.order[0] if m.order else None
            with pytest.raises(ValueError, match="not registered"):
                lg.plan_remove(book, [known, "nobody"] if known is not None else ["nobody"])
            with pytest.raises(ValueError, match="not registered"):
                lg.plan_shots(book, ["nobody"])
            with pytest.raises(ValueError, match="not registered"):
                lg.plan_columns(book, ["nobody"])
            if known is not None:
                with pytest.raises(ValueError, match="already registered"):
                    lg.plan_add(book, [next_id + 1000, known])
                with pytest.raises(ValueError, match="twice"):
                    lg.plan_remove(book, [known, known])
                with pytest.raises(ValueError, match="twice"):
                    lg.plan_columns(book, [known, known])
            with pytest.raises(ValueError, match="twice"):
                lg.plan_add(book, [next_id + 1000, next_id + 1000])
            assert (book.cap, book.free, book.order, book.slot_of, book.shots, book.version) == before
        _same(book, m)


def test_growth_is_one_and_a_half_times_and_loaded_classes_take_no_shots():
    from clip_fsar_amd import live_gallery as lg
    assert [lg.grown(c, 1) for c in (1, 2, 3, 8, 64, 100)] == [2, 3, 4, 12, 96, 150]
    assert lg.grown(8, 30) == 40                   # 8 -> 12 -> 18 -> 27 -> 40
    book = lg.plan_add(lg.new_book(4), ["a", "b"]).book
    book = book._replace(shots={"a": 0, "b": 2})   # "a": loaded from a SupportGallery state
    with pytest.raises(ValueError, match="loaded without its sum"):
        lg.plan_shots(book, ["b", "a"])
    assert lg.plan_shots(book, ["b", "b"]).book.shots == {"a": 0, "b": 4}


# ------------------------------------------------------------------ LiveGallery on a stub head: misuse, before any device work
def _stub_head(T=4, **train):
    engine = NS(arch={"embed": 8})
    return NS(args=NS(TRAIN=NS(**train), DATA=NS(NUM_INPUT_FRAMES=T)), _get_engine=lambda dev: engine, _engine_key=("stub",),
              arch_name="stub", precision="fp32", depth=1)


def test_live_gallery_rejects_misuse_before_any_launch():
    import torch
    from clip_fsar_amd.gallery import SupportGallery
    from clip_fsar_amd.live_gallery import LiveGallery
    from clip_fsar_amd.pool import StreamPool
    from clip_fsar_amd.stream import WindowStream
    for flag in ("EVAL_TEXT", "COMBINE"):
        with pytest.raises(NotImplementedError, match="TextGallery"):
            LiveGallery(_stub_head(**{flag: True}), "cpu")
    for cap in (0, -1, 2.5, True):
        with pytest.raises(ValueError, match="capacity"):
            LiveGallery(_stub_head(), "cpu", capacity=cap)
    with pytest.raises(ValueError, match="at most 32"):
        LiveGallery(_stub_head(T=33), "cpu")
    g = LiveGallery(_stub_head(), "cpu", capacity=3)
    assert len(g) == 0 and g.class_ids == [] and g.layout_version == 0 and g.capacity == 3 and g._store is None
    assert g.fingerprint() == SupportGallery(_stub_head(), "cpu").fingerprint()
    with pytest.raises(ValueError, match="not registered"):
        g.remove_classes([1])
    with pytest.raises(ValueError, match="not registered"):
        g.shots(1)
    with pytest.raises(RuntimeError, match="no classes registered"):
        g.classify(torch.zeros(1, 4, 3, 8, 8))
    with pytest.raises(RuntimeError, match="no CPU path"):
        g.add_classes(torch.zeros(1, 4, 3, 8, 8), [0])
    with pytest.raises(RuntimeError, match="no CPU path"):
        g.add_shots(torch.zeros(1, 4, 3, 8, 8), [0])
    assert g._store is None and g._tables is None and len(g) == 0 and g.layout_version == 0
    sd = g.state_dict()
    assert sd["class_ids"] == [] and sd["counts"] == [] and tuple(sd["sums"].shape) == (0, 5, 8)
    SupportGallery(_stub_head(), "cpu").load_state_dict(sd)          # SupportGallery's keys are all there
    with pytest.raises(ValueError, match="fingerprint"):
        g.load_state_dict(dict(sd, fingerprint=dict(sd["fingerprint"], T=16)))
    with pytest.raises(ValueError, match="inconsistent shapes"):
        g.load_state_dict(dict(sd, class_ids=[1]))
    # accepted wherever a SupportGallery is
    assert StreamPool(g, max_streams=2).gallery is g and WindowStream(g, n_streams=1).gallery is g
