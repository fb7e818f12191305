"""CPU: the grouped text library (libclipfsar_live_text.so, include/clipfsar_live_text.h) validates its descriptor table without a GPU;
plan_text_groups against a list model; misuse of LiveTextGallery on a stub head; the state dicts.  Its exports, kernels and place in the
build are checked with every library's in tests/test_build_recipe.py."""
import ctypes
import os
import random
import re
from types import SimpleNamespace as NS

import pytest

from _abi import _prototypes, check_abi_at_load, check_exports, lib_row

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "clipfsar_live_text.h")


@pytest.fixture(scope="module")
def tlib():
    import __graft_entry__ as ge
    ge.build()                                    # builds every library (no-op when up to date)
    from clip_fsar_amd import live_text_hip
    return live_text_hip.lib()


# ------------------------------------------------------------------ what is particular to this library's header and source
def test_header_exported_exactly_and_arity_matches(tlib):
    check_exports(lib_row("live_text"))                 # the checks every library gets; below, what is particular to this one
    from clip_fsar_amd import live_text_hip as lt
    protos = _prototypes(HEADER, "cflt_")
    assert protos["cflt_text_logits_grouped"] == 18
    text = open(HEADER).read()
    assert int(re.search(r"#define CFLT_TABLE_COLS (\d+)", text).group(1)) == lt.TABLE_COLS == 8
    assert int(re.search(r"#define CFLT_MAX_GROUPS (\d+)", text).group(1)) == lt.MAX_GROUPS
    for i, col in enumerate(("Q0", "NQ", "C0", "NC", "TILE0", "OUT0", "PART0", "PAD")):       # the binding's column order is the header's
        assert int(re.search(r"#define CFLT_%s (\d+)" % col, text).group(1)) == getattr(lt, col) == i
    assert lt.table_uploader("cpu", 4).cols == lt.TABLE_COLS


def test_abi_version_is_checked_at_load(tlib, monkeypatch):
    check_abi_at_load(lib_row("live_text"), monkeypatch)


def test_the_source_allocates_nothing_and_holds_no_matrix_code_of_its_own():
    from clip_fsar_amd import build as b
    src = open(os.path.join(b.CSRC, b.SIDE_LIBS["live_text"].source)).read()
    for body in ("asm", "__builtin_amdgcn_mfma", "thread_local", "hipMalloc", "hipStreamCreate"):
        assert body not in src, body


# ------------------------------------------------------------------ table validation, without a GPU
def _tbl(rows):
    flat = [v for r in rows for v in r]
    return (ctypes.c_int32 * len(flat))(*flat)


#        Q0  NQ  C0   NC TILE0 OUT0  PART0 0
GOOD = [[0,   1,  0,   1,  0,    0,    0,  0],      # 1 x 1 tiles, 1 partial
        [1,  65,  1,  64,  1,    1,    1,  0],      # 2 x 1, 65 partials
        [66,  0, 65,   3,  3, 4161,   66,  0],      # no queries: no tiles, no output, no partials
        [66, 17, 68, 130,  3, 4161,   66,  0]]      # 1 x 3, 51 partials
NQ, NCOLS, NOUT, NPART, TILES = 83, 198, 4161 + 17 * 130, 66 + 51, 6


def _edit(row, col, value):
    rows = [list(r) for r in GOOD]
    rows[row][col] = value
    return _tbl(rows)


def test_good_table_is_what_the_binding_plans(tlib):
    from clip_fsar_amd import live_text_hip as lt
    rows, totals = lt.table_rows([1, 65, 0, 17], [1, 64, 3, 130])
    assert rows == GOOD and totals == (NQ, NCOLS, TILES, NOUT, NPART) and lt.n_partials(rows) == NPART
    assert tlib.cflt_workspace_floats(_tbl(GOOD), 4) == 2 * NPART
    assert tlib.cflt_workspace_floats(_tbl(GOOD), 1) == 2 and tlib.cflt_workspace_floats(_tbl(GOOD), 3) == 2 * 66
    assert tlib.cflt_workspace_floats(None, 4) == -1 and tlib.cflt_workspace_floats(_tbl(GOOD), 0) == -1
    assert tlib.cflt_workspace_floats(_tbl(GOOD), (1 << 16) + 1) == -1
    assert tlib.cflt_workspace_floats(_edit(1, 1, -1), 4) == -1 and tlib.cflt_workspace_floats(_edit(3, 3, 0), 4) == -1
    assert tlib.cflt_workspace_floats(_tbl([[0, 1 << 30, 0, 65, 0, 0, 0, 0]]), 1) == -1


def test_table_validation_without_gpu(tlib):
    p = ctypes.c_void_p(4096)                     # never dereferenced: every call below fails validation before any device work
    err, good = tlib.cflt_last_error, _tbl(GOOD)
    PTRS = ("emb", "en", "text", "tn", "cols", "scale", "logits", "partials", "tdev")

    def logits(table=good, G=4, nq=NQ, ncols=NCOLS, nout=NOUT, npart=NPART, cap=160, E=64, **ptr):
        a = dict.fromkeys(PTRS, p)
        a.update(ptr)
        return tlib.cflt_text_logits_grouped(a["emb"], a["en"], a["text"], a["tn"], a["cols"], a["scale"], a["logits"], a["partials"],
                                             table, a["tdev"], G, nq, ncols, nout, npart, cap, E, None)

    def softmax(table=good, G=4, nq=NQ, nout=NOUT, npart=NPART, **ptr):
        a = dict.fromkeys(("logits", "partials", "probs", "tdev"), p)
        a.update(ptr)
        return tlib.cflt_text_softmax_grouped(a["logits"], a["partials"], a["probs"], table, a["tdev"], G, nq, nout, npart, None)

    def combine(table=good, G=4, nq=NQ, nout=NOUT, npart=NPART, coff=0.9, **ptr):
        a = dict.fromkeys(("logits", "partials", "visual", "out", "tdev"), p)
        a.update(ptr)
        return tlib.cflt_text_combine_grouped(a["logits"], a["partials"], a["visual"], a["out"], table, a["tdev"], G, nq, nout, npart,
                                              coff, None)

    for name in PTRS:
        assert logits(**{name: None}) != 0 and b"null" in err(), name
    for name in ("logits", "partials", "probs", "tdev"):
        assert softmax(**{name: None}) != 0 and b"null" in err(), name
    for name in ("logits", "partials", "visual", "out", "tdev"):
        assert combine(**{name: None}) != 0 and b"null" in err(), name
    for call in (logits, softmax, combine):
        assert call(table=None) != 0 and b"null" in err()
    for kw in ({"E": 66}, {"E": 0}, {"E": 8196}, {"cap": 0}, {"nq": 0}, {"ncols": 0}, {"nout": 0}, {"npart": 0}):
        assert logits(**kw) != 0 and b"bad shape" in err(), kw
    for call in (softmax, combine):
        for kw in ({"nq": 0}, {"nout": 0}, {"npart": 0}):
            assert call(**kw) != 0 and b"bad shape" in err(), kw
    assert logits(emb=ctypes.c_void_p(4100)) != 0 and b"16-byte aligned" in err()
    assert logits(text=ctypes.c_void_p(4104)) != 0 and b"16-byte aligned" in err()
    for coff in (float("nan"), float("inf"), -float("inf")):
        assert combine(coff=coff) != 0 and b"finite" in err(), coff
    for call in (logits, softmax, combine):
        for G in (0, -1, (1 << 16) + 1):
            assert call(G=G) != 0 and b"groups" in err(), G
        # each prefix column with its own message, in a first, a middle and the last row
        for col, msg in ((0, b"Q0="), (2, b"C0="), (4, b"TILE0="), (5, b"OUT0="), (6, b"PART0="), (7, b"last column")):
            for row in (0, 1, 3):
                assert call(table=_edit(row, col, GOOD[row][col] + 1)) != 0 and msg in err() and (b"group %d " % row) in err(), (row, col)
        assert call(table=_edit(2, 4, 2)) != 0 and b"TILE0=" in err() and b"group 2 " in err()      # of the group without queries
        assert call(table=_edit(1, 1, 64)) != 0 and b"group 2 has Q0=66" in err()                  # a count its successor contradicts
        for row in (0, 1, 3):
            assert call(table=_edit(row, 1, -1)) != 0 and b"cannot be negative" in err() and (b"group %d " % row) in err()
            assert call(table=_edit(row, 3, 0)) != 0 and b"at least 1" in err() and (b"group %d " % row) in err()
        # the totals
        assert call(nq=NQ + 1) != 0 and b"not to NQ" in err()
        assert call(nout=NOUT - 1) != 0 and b"not to NOUT" in err()
        assert call(npart=NPART + 1) != 0 and b"not NPART" in err()
        # 32-bit sizes
        big = [[0, 1 << 16, 0, 1 << 16, 0, 0, 0, 0]]
        assert call(table=_tbl(big), G=1, nq=1 << 16, nout=1) != 0 and b"32-bit" in err()
    assert logits(ncols=NCOLS + 1) != 0 and b"not to NCOLS" in err()
    assert softmax(G=3, nq=66, nout=4161, npart=66, tdev=None) != 0 and b"null" in err()            # validation order: pointers first


def test_python_wrapper_rejects_cpu_tensors_and_bad_shapes(tlib):
    import torch
    from clip_fsar_amd import live_text_hip as lt
    from clip_fsar_amd import pool_hip as ph
    host = torch.tensor(GOOD, dtype=torch.int32)
    table = ph.Table(host, host, 4)               # a device copy that is no device tensor
    emb, en, text, tn = torch.zeros(NQ, 64), torch.zeros(NQ), torch.zeros(160, 64), torch.zeros(160)
    cols, scale = torch.zeros(NCOLS, dtype=torch.int32), torch.zeros(1)
    out, part = torch.zeros(NOUT), torch.zeros(2 * NPART)
    with pytest.raises(RuntimeError, match="HIP device tensor"):
        lt.text_logits_grouped(emb, en, text, tn, cols, scale, out, part, table, NOUT, NPART)
    with pytest.raises(RuntimeError, match="tn_store has shape"):
        lt.text_logits_grouped(emb, en, text, tn[:5], cols, scale, out, part, table, NOUT, NPART)
    with pytest.raises(RuntimeError, match=r"logits has shape .* expected \[>= %d\]" % NOUT):
        lt.text_logits_grouped(emb, en, text, tn, cols, scale, out[:-1], part, table, NOUT, NPART)
    with pytest.raises(RuntimeError, match=r"partials has shape"):
        lt.text_softmax_grouped(out, part[:-1], out, table, NQ, NOUT, NPART)
    with pytest.raises(RuntimeError, match=r"visual has shape"):
        lt.text_combine_grouped(out, part, out[:3], out, table, NQ, NOUT, NPART, 0.9)
    with pytest.raises(RuntimeError, match="Table"):
        lt.text_softmax_grouped(out, part, out, ph.Table(host[:, :6], host, 4), NQ, NOUT, NPART)
    with pytest.raises(RuntimeError, match="HIP device tensor"):
        lt.text_softmax_grouped(out, part, out, table, NQ, NOUT, NPART)


# ------------------------------------------------------------------ plan_text_groups against a list model
def test_plan_text_groups_against_a_list_model():
    from clip_fsar_amd import live_gallery as lg
    from clip_fsar_amd import live_text_gallery as ltg
    from clip_fsar_amd import live_text_hip as lt
    rng = random.Random(7)
    for trial in range(40):
        book = lg.new_book(rng.randint(1, 8))
        ids = list(range(rng.randint(1, 150)))
        book = lg.plan_add(book, ids).book
        gone = rng.sample(ids, rng.randint(0, len(ids) - 1))
        if gone:
            book = lg.plan_remove(book, gone).book
        T = rng.choice([1, 4, 8, 16])
        G = rng.randint(1, 12)
        counts = [rng.choice([0, 0, 1, 3, 64, 65, 129]) for _ in range(G)]
        classes = [None if rng.random() < 0.3 else rng.sample(book.order, rng.randint(1, len(book.order))) for _ in range(G)]
        plan = ltg.plan_text_groups(book, counts, classes, T)
        base = lg.plan_groups(book, counts, classes, T)
        assert (plan.rows, plan.slots, plan.n_out) == (base.rows, base.slots, base.n_out)
        # the model: every (group, query, class tile) in launch order owns the next partial, every (group, query, class) the next output
        q = c = tiles = out = part = 0
        for g, (n, cl) in enumerate(zip(counts, classes)):
            names = book.order if cl is None else cl
            row = plan.text_rows[g]
            assert row == [q, n, c, len(names), tiles, out, part, 0], (trial, g)
            assert plan.slots[c:c + len(names)] == [book.slot_of[x] for x in names]
            ct = len(range(0, len(names), 64))
            tiles += len(range(0, n, 64)) * ct
            part += sum(1 for _ in range(n) for _ in range(ct))
            q, c, out = q + n, c + len(names), out + n * len(names)
        assert plan.n_out == out and plan.n_part == part == lt.n_partials(plan.text_rows)
        assert ltg.text_rows_of(plan.rows) == (plan.text_rows, part)
    with pytest.raises(ValueError, match="LiveTextGallery: group 1: class 'x' is not registered"):
        ltg.plan_text_groups(book, [1, 1], [None, ["x"]], 8)
    with pytest.raises(ValueError, match="grouped scoring needs groups"):
        ltg.plan_text_groups(book, [], [], 8)


# ------------------------------------------------------------------ LiveTextGallery on a stub head: misuse, before any launch
def _stub_head(T=4, n_test=3, **train):
    import torch
    engine = NS(arch={"embed": 8}, text_test=torch.zeros(n_test, 8))
    return NS(args=NS(TRAIN=NS(**train), DATA=NS(NUM_INPUT_FRAMES=T)), _get_engine=lambda dev: engine, _engine_key=("stub",),
              arch_name="stub", precision="fp32", depth=1)


def _stub_gallery(mode, ids=("a", "b", 1), **train):
    from clip_fsar_amd import live_gallery as lg
    from clip_fsar_amd.live_text_gallery import LiveTextGallery
    g = LiveTextGallery(_stub_head(**train), "cpu", mode=mode, capacity=4)
    if ids:
        book = lg.plan_add(g._book, list(ids)).book                # registered on the host alone: nothing below reaches the device
        g._install(book if mode == "combine" else book._replace(shots=dict.fromkeys(ids, 0)))
    return g


def _snapshot(g):
    b = g._book
    return (b.cap, list(b.free), list(b.order), dict(b.slot_of), dict(b.shots), b.version, g._store, g.class_ids)


def test_construction_mode_and_fingerprint():
    from clip_fsar_amd.live_gallery import LiveGallery
    from clip_fsar_amd.live_text_gallery import LiveTextGallery
    from clip_fsar_amd.text_gallery import TextGallery
    with pytest.raises(ValueError, match="neither"):
        LiveTextGallery(_stub_head(), "cpu")
    with pytest.raises(ValueError, match="contradicts"):
        LiveTextGallery(_stub_head(EVAL_TEXT=True), "cpu", mode="combine")
    with pytest.raises(ValueError, match="mode must be"):
        LiveTextGallery(_stub_head(), "cpu", mode="otam")
    for bad in (0, -1, True, 2.0):
        with pytest.raises(ValueError, match="capacity must be an integer >= 1"):
            LiveTextGallery(_stub_head(COMBINE=True), "cpu", capacity=bad)
    assert LiveTextGallery(_stub_head(EVAL_TEXT=True, COMBINE=True), "cpu").mode == "eval_text"
    for train, mode in ((dict(COMBINE=True, TEXT_COFF=0.5), None), (dict(EVAL_TEXT=True), None), (dict(MERGE_BEFORE=True), "combine")):
        g, t = LiveTextGallery(_stub_head(**train), "cpu", mode=mode), TextGallery(_stub_head(**train), "cpu", mode=mode)
        assert isinstance(g, LiveGallery) and g.fingerprint() == t.fingerprint() and g.mode == t.mode and g.text_coff == t.text_coff
        assert len(g) == 0 and g.capacity == 64 and g.layout_version == 0
    for flag in ("EVAL_TEXT", "COMBINE"):                              # LiveGallery itself still points at TextGallery
        with pytest.raises(NotImplementedError, match="TextGallery"):
            LiveGallery(_stub_head(**{flag: True}), "cpu")


@pytest.mark.parametrize("mode", ["eval_text", "combine"])
def test_misuse_is_rejected_before_any_launch(mode):
    import torch
    g = _stub_gallery(mode)
    before = _snapshot(g)
    feats, vids = torch.zeros(2, 4, 8), torch.zeros(2, 4, 3, 8, 8)
    # the device checks
    for call in (lambda: g.classify(vids), lambda: g.classify_grouped(vids, [2], [None]), lambda: g.topk(vids, 1),
                 lambda: g.topk_grouped(vids, [2], [None], 1)):
        with pytest.raises(RuntimeError, match="queries must be a HIP device tensor"):
            call()
    for call in (lambda: g.classify_features(feats), lambda: g.classify_features_grouped(feats, [2], [None])):
        with pytest.raises(RuntimeError, match="feats must be a HIP device tensor"):
            call()
    # classes=: LiveGallery's rules and texts
    for call in (lambda c: g.classify_features(feats, classes=c), lambda c: g.classify(vids, classes=c), lambda c: g.topk(vids, 1, classes=c)):
        with pytest.raises(ValueError, match=r"LiveTextGallery: class 'z' is not registered \(classes=\)"):
            call(["a", "z"])
        with pytest.raises(ValueError, match="classes= needs at least one class"):
            call([])
        with pytest.raises(ValueError, match="a class appears twice in classes="):
            call(["a", 1, "a"])
    for call in (lambda n, c: g.classify_features_grouped(feats, n, c), lambda n, c: g.classify_grouped(vids, n, c),
                 lambda n, c: g.topk_grouped(vids, n, c, 1)):
        with pytest.raises(ValueError, match="LiveTextGallery: group 1: class 'z' is not registered"):
            call([1, 1], [None, ["z"]])
        with pytest.raises(ValueError, match="got 2 counts and 1 class lists"):
            call([1, 1], [None])
        with pytest.raises(ValueError, match="a group's count must be an integer >= 0"):
            call([1, -1], [None, None])
    for k in (0, 4, 17, True, 1.0):
        with pytest.raises(ValueError, match=r"topk: k must be in \[1, min\(16, number of classes\)\]"):
            g.topk(vids, k)
    for k in (0, 3, True):
        with pytest.raises(ValueError, match="topk_grouped: k must be in"):
            g.topk_grouped(vids, [1, 1], [None, ["a", "b"]], k)
    g._check_feats = lambda f: _shape_check(g, f)                  # the device check aside: what follows it, still before any launch
    with pytest.raises(ValueError, match="the groups' counts add up to 3, the call holds 2 clips"):
        g.classify_features_grouped(feats, [1, 2], [None, None])
    with pytest.raises(ValueError, match=r"feats must be \[N, T=4, E=8\]"):
        g.classify_features(torch.zeros(2, 3, 8))
    assert tuple(g.classify_features(feats[:0], classes=["b", "a"]).shape) == (0, 2)        # no clips: no launch
    # registration
    with pytest.raises(ValueError, match="class 'a' is already registered"):
        g.add_classes_features(feats, ["x", "a"], text={"x": [0.0] * 8})
    with pytest.raises(ValueError, match="2 videos but 3 class ids"):
        g.add_classes_features(feats, ["x", "y", "z"])
    with pytest.raises(ValueError, match="class 'x' is not an index into TEST.CLASS_NAME"):
        g.add_classes_features(feats, ["x", "x"])
    with pytest.raises(ValueError, match="text row of class 'x' has 7 values, expected 8"):
        g.add_classes_features(feats, ["x", "x"], text={"x": [0.0] * 7})
    with pytest.raises(RuntimeError, match="videos must be a HIP device tensor"):
        g.add_classes(vids, ["x", "y"])
    if mode == "combine":
        with pytest.raises(ValueError, match="add_text_classes: a COMBINE gallery needs support videos"):
            g.add_text_classes([0, 2])
        with pytest.raises(ValueError, match=r"class 'z' is not registered \(add_shots"):
            g.add_shots_features(feats, ["a", "z"])
        with pytest.raises(RuntimeError, match="videos must be a HIP device tensor"):
            g.add_shots(vids, ["a", "b"])
        g._book = g._book._replace(shots=dict(g._book.shots, b=0))
        before = _snapshot(g)
        with pytest.raises(ValueError, match="class 'b' was loaded without its sum"):
            g.add_shots_features(feats, ["a", "b"])
    else:
        for call in (lambda: g.add_shots(vids, ["a", "b"]), lambda: g.add_shots_features(feats, ["a", "b"]),
                     lambda: g.add_shots("no tensor", ["a"])):
            with pytest.raises(ValueError, match="an EVAL_TEXT class is its text row and takes no shots"):
                call()
        with pytest.raises(ValueError, match="class 'a' is already registered"):
            g.add_text_classes([0, "a"])
        with pytest.raises(ValueError, match=r"add_text_classes: class ids repeat in \[0, 0\]"):
            g.add_text_classes([0, 0])
        with pytest.raises(ValueError, match="class 5 is not an index into TEST.CLASS_NAME"):
            g.add_text_classes([0, 5])
        with pytest.raises(TypeError, match="`text` must map"):
            g.add_text_classes([0], text=[0])
    with pytest.raises(ValueError, match=r"class 'z' is not registered \(remove_classes\)"):
        g.remove_classes(["a", "z"])
    # a stale engine
    g.head._engine_key = ("other",)
    for call in (lambda: g.classify_features(feats), lambda: g.add_text_classes([0]) if mode == "eval_text" else g.add_classes(vids, [0, 0]),
                 lambda: g.classify_features_grouped(feats, [2], [None])):
        with pytest.raises(RuntimeError, match="changed since these prototypes"):
            call()
    g.head._engine_key = ("stub",)
    assert _snapshot(g) == before and g._store is None and g._tables is None and g._text_tables is None and g._group_tables is None


def _shape_check(g, feats):
    if feats.dim() != 3 or feats.shape[1] != g.T or feats.shape[2] != g.E:
        raise ValueError("%s: feats must be [N, T=%d, E=%d], got %s" % (g._name, g.T, g.E, tuple(feats.shape)))
    return feats


def test_stream_pool_accepts_it_and_surfaces_the_shot_error_before_any_launch():
    from clip_fsar_amd.pool import StreamPool
    from clip_fsar_amd.stream import WindowStream
    for mode in ("eval_text", "combine"):
        g = _stub_gallery(mode)
        assert WindowStream(g, n_streams=1, max_push=2).gallery is g
        p = StreamPool(g, max_streams=3, stride=2, max_push=3)
        a = p.open(classes=["b", 1])                                  # a gallery that scores groups
        with pytest.raises(ValueError, match="session %d: class 'z' is not registered" % (a + 1)):
            p.open(classes=["z"])
        p._sessions[a].t = 11
        assert p.enrolable(a) == range(3, 4)
        before = _snapshot(g)
        if mode == "eval_text":
            with pytest.raises(ValueError, match="an EVAL_TEXT class is its text row and takes no shots"):
                p.enroll(a, "a")
            with pytest.raises(ValueError, match="takes no shots"):
                p.enroll_windows([(a, None, 2), (a, 3, "b")])         # a new class beside a further shot: nothing is registered
        else:
            with pytest.raises(ValueError, match="class 7 is not an index into TEST.CLASS_NAME"):
                p.enroll(a, 7)
        assert _snapshot(g) == before and g._store is None and p._enroll_tables is None and p._sessions[a].classes == ["b", 1]


# ------------------------------------------------------------------ state dicts: the key sets, both directions (host tensors alone)
@pytest.mark.parametrize("mode", ["eval_text", "combine"])
def test_state_dict_keys_both_directions(mode):
    import torch
    from clip_fsar_amd.live_text_gallery import LiveTextGallery
    from clip_fsar_amd.text_gallery import TextGallery
    T, E, C = 4, 8, 3
    Cp = C if mode == "combine" else 0
    t = TextGallery(_stub_head(), "cpu", mode=mode)
    gen = torch.Generator().manual_seed(3)
    t._ids, t._text, t._tn = ["a", "b", 1], torch.randn(C, E, generator=gen), torch.rand(C, generator=gen) + 1
    t._P, t._pn = torch.randn(Cp, T, E, generator=gen), torch.rand(Cp * T, generator=gen) + 1
    sd_t = t.state_dict()
    assert set(sd_t) == {"fingerprint", "class_ids", "text", "text_norms", "prototypes", "norms"}
    g = LiveTextGallery(_stub_head(), "cpu", mode=mode, capacity=2)
    assert set(g.state_dict()) == set(sd_t) | {"sums", "counts"} and g.state_dict()["class_ids"] == []
    TextGallery(_stub_head(), "cpu", mode=mode).load_state_dict(g.state_dict())          # an empty one loads too
    g.load_state_dict(sd_t)                                           # TextGallery -> LiveTextGallery
    assert g.class_ids == ["a", "b", 1] and [g.shots(c) for c in g.class_ids] == [0, 0, 0] and g.capacity == 3 and g.layout_version == 1
    assert set(g._store) == ({"P", "pn", "text", "sums", "tn"} if mode == "combine" else {"text", "tn"})
    with pytest.raises(ValueError, match="takes no shots" if mode == "eval_text" else "class 'a' was loaded without its sum"):
        g._check_feats = lambda f: f                                  # the device check aside
        g.add_shots_features(torch.zeros(1, T, E), ["a"])
    g.remove_classes(["b"])
    sd_g = g.state_dict()
    assert set(sd_g) == set(sd_t) | {"sums", "counts"} and sd_g["class_ids"] == ["a", 1] and sd_g["counts"] == [0, 0]
    keep = torch.tensor([0, 2])
    assert torch.equal(sd_g["text"], sd_t["text"][keep]) and torch.equal(sd_g["text_norms"], sd_t["text_norms"][keep])
    assert tuple(sd_g["prototypes"].shape) == (2 if Cp else 0, T, E) and tuple(sd_g["sums"].shape) == (2 if Cp else 0, T + 1, E)
    if Cp:
        assert torch.equal(sd_g["prototypes"], sd_t["prototypes"][keep])
        assert torch.equal(sd_g["norms"], sd_t["norms"].view(C, T)[keep].reshape(-1))
    t2 = TextGallery(_stub_head(), "cpu", mode=mode)
    t2.load_state_dict(sd_g)                                          # LiveTextGallery -> TextGallery
    assert t2.class_ids == ["a", 1] and torch.equal(t2._text, sd_g["text"]) and torch.equal(t2._P, sd_g["prototypes"])
    g2 = LiveTextGallery(_stub_head(), "cpu", mode=mode)
    g2.load_state_dict(sd_g)                                          # and its own
    assert g2.class_ids == ["a", 1] and torch.equal(g2.state_dict()["text"], sd_g["text"])
    other = "combine" if mode == "eval_text" else "eval_text"
    with pytest.raises(ValueError, match="fingerprint"):
        LiveTextGallery(_stub_head(), "cpu", mode=other).load_state_dict(sd_g)
    with pytest.raises(ValueError, match="inconsistent shapes"):
        g2.load_state_dict(dict(sd_g, text_norms=sd_g["text_norms"][:1]))
    with pytest.raises(ValueError, match="come together"):
        g2.load_state_dict({k: v for k, v in sd_g.items() if k != "counts"})
    assert g2.class_ids == ["a", 1]
