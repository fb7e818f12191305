"""CPU: the stream-pool library (libclipfsar_pool.so, include/clipfsar_pool.h) validates arguments and descriptor tables without a GPU; the
host plan of a push (plan_push, slot assignment) against a brute-force model of the ring over random schedules; StreamPool's constructor and
session errors on a stub head.  Its exports, kernels and place in the build are checked with every library's in tests/test_build_recipe.py."""
import ctypes
import os
import random
import re
from types import SimpleNamespace as NS

import pytest

from _abi import check_exports, lib_row

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "clipfsar_pool.h")


@pytest.fixture(scope="module")
def plib():
    import __graft_entry__ as ge
    ge.build()                                    # builds every library (no-op when up to date)
    from clip_fsar_amd import pool_hip
    return pool_hip.lib()


def test_header_exported_exactly_and_arity_matches(plib):
    check_exports(lib_row("pool"))                 # the checks every library gets; below, what is particular to this one
    from clip_fsar_amd import pool_hip as ph
    text = open(HEADER).read()
    assert int(re.search(r"#define CFSP_MAX_T (\d+)", text).group(1)) == ph.MAX_T == 32
    assert int(re.search(r"#define CFSP_MAX_STREAMS (\d+)", text).group(1)) == ph.MAX_STREAMS
    assert int(re.search(r"#define CFSP_TABLE_COLS (\d+)", text).group(1)) == ph.TABLE_COLS == 8
    cols = ("SLOT", "PUT_POS", "N", "FEAT_OFF", "WIN_POS", "NW", "WIN_OFF", "HAS_STATE")
    for i, col in enumerate(cols):                # the binding's column order is the header's
        assert int(re.search(r"#define CFSP_%s (\d+)" % col, text).group(1)) == getattr(ph, col) == i


# ------------------------------------------------------------------ validation, without a GPU
def _tbl(rows):
    flat = [v for r in rows for v in r]
    return (ctypes.c_int32 * len(flat))(*flat)


#        slot put_pos n feat_off win_pos nW win_off has_state
GOOD = [[2, 5, 3, 0, 1, 1, 0, 0],
        [0, 0, 4, 3, 0, 0, 1, 0],
        [1, 9, 2, 7, 6, 2, 1, 1]]               # N = 9, NW = 3; cap 16, max_streams 4


def _edit(row, col, value):
    rows = [list(r) for r in GOOD]
    rows[row][col] = value
    return _tbl(rows)


def test_argument_validation_without_gpu(plib):
    p = ctypes.c_void_p(4096)                     # never dereferenced: every call below fails validation before any device work
    L, err, good = plib, plib.cfsp_last_error, _tbl(GOOD)
    # ring_put(feats, ring, table_host, table_dev, S, N, E, max_streams, cap, stream)
    put = L.cfsp_ring_put
    for args in ((None, p, good, p), (p, None, good, p), (p, p, None, p), (p, p, good, None)):
        assert put(*args, 3, 9, 64, 4, 16, None) != 0 and b"null" in err()
    for N, E, cap in ((0, 64, 16), (9, 0, 16), (9, 64, 0), (-1, 64, 16)):
        assert put(p, p, good, p, 3, N, E, 4, cap, None) != 0 and b"bad shape" in err(), (N, E, cap)
    assert put(p, p, good, p, 3, 9, 64, 0, 16, None) != 0 and b"max_streams" in err()
    assert put(p, p, good, p, 3, 9, 64, 1 << 20, 16, None) != 0 and b"max_streams" in err()
    assert put(p, p, good, p, 0, 9, 64, 4, 16, None) != 0 and b"rows" in err()
    assert put(p, p, good, p, 3, 9, 64, 2, 16, None) != 0 and b"rows" in err()                     # more rows than slots
    assert put(p, p, good, p, 3, 10, 64, 4, 16, None) != 0 and b"not to N" in err()                # counts do not sum to N
    assert put(p, p, good, p, 3, 9, 64, 4, 1 << 26, None) != 0 and b"too large" in err()
    assert put(p, p, _tbl([[0, 0, 16, 0, 0, 0, 0, 0]]), p, 1, 16, 1 << 20, 64, 2047, None) != 0 and b"too large" in err()

    # the table, through every entry point that reads the column
    ws, sm = L.cfsp_window_sequences, L.cfsp_smooth_logits

    calls = (lambda t: put(p, p, t, p, 3, 9, 64, 4, 16, None), lambda t: ws(p, p, t, p, 3, 3, 0, 3, 4, 64, 4, 16, 2, 1, None),
             lambda t: sm(p, p, p, t, p, 3, 3, 5, 4, 0.5, None))

    def rejected(table, *words, by=(0, 1, 2)):
        for i in by:
            assert calls[i](table) != 0 and all(w in err() for w in words), (i, words, err())

    for slot in (-1, 4):
        rejected(_edit(1, 0, slot), b"slot", b"outside")
    rejected(_edit(2, 0, 2), b"appears twice")
    for col in (2, 5):
        rejected(_edit(0, col, -1), b"negative count")
    for col in (3, 6):                             # offsets that are not the prefix sums of the counts
        rejected(_edit(2, col, 5), b"prefix sums")
    rejected(_edit(0, 3, 1), b"prefix sums")
    rejected(_edit(1, 7, 2), b"has_state")
    for col in (1, 4):                             # ring positions: below 0 everywhere, at cap where there is a ring
        rejected(_edit(1, col, -1), b"ring position")
        rejected(_edit(1, col, 16), b"ring position", by=(0, 1))
    assert put(p, p, _tbl([[0, 0, 17, 0, 0, 0, 0, 0]]), p, 1, 17, 64, 4, 16, None) != 0 and b"do not fit" in err()

    # window_sequences(ring, X, table_host, table_dev, S, NW, w0, w1, T, E, max_streams, cap, stride, rate, stream)
    for args in ((None, p, good, p), (p, None, good, p), (p, p, None, p), (p, p, good, None)):
        assert ws(*args, 3, 3, 0, 3, 4, 64, 4, 16, 2, 1, None) != 0 and b"null" in err()
    for NW, E, cap in ((0, 64, 16), (3, 0, 16), (3, 64, 0)):
        assert ws(p, p, good, p, 3, NW, 0, 3, 4, E, 4, cap, 2, 1, None) != 0 and b"bad shape" in err()
    for T in (0, 33, -1):
        assert ws(p, p, good, p, 3, 3, 0, 3, T, 64, 4, 16, 2, 1, None) != 0 and b"T=" in err(), T
    for stride in (0, -3):
        assert ws(p, p, good, p, 3, 3, 0, 3, 4, 64, 4, 16, stride, 1, None) != 0 and b"stride" in err()
    for rate in (0, -1):
        assert ws(p, p, good, p, 3, 3, 0, 3, 4, 64, 4, 16, 2, rate, None) != 0 and b"rate" in err()
    for w0, w1 in ((-1, 2), (2, 2), (3, 2), (0, 4)):
        assert ws(p, p, good, p, 3, 3, w0, w1, 4, 64, 4, 16, 2, 1, None) != 0 and b"window range" in err(), (w0, w1)
    assert ws(p, p, good, p, 3, 4, 0, 3, 4, 64, 4, 16, 2, 1, None) != 0 and b"not to NW" in err()
    # two windows at stride 2 of T = 4 frames at rate 5 span 2 + 15 + 1 = 18 ring positions: more than cap = 16
    assert ws(p, p, good, p, 3, 3, 0, 3, 4, 64, 4, 16, 2, 5, None) != 0 and b"do not fit" in err()
    assert ws(p, p, good, p, 3, 3, 0, 3, 4, 64, 4, 16, 1 << 30, 1, None) != 0 and b"do not fit" in err()
    assert ws(p, p, good, p, 3, 3, 0, 3, 4, 1 << 22, 4, 2047, 2, 1, None) != 0 and b"too large" in err()

    # smooth_logits(logits, state, out, table_host, table_dev, S, NW, C, max_streams, alpha, stream)
    for args in ((None, p, p, good, p), (p, None, p, good, p), (p, p, None, good, p), (p, p, p, None, p), (p, p, p, good, None)):
        assert sm(*args, 3, 3, 5, 4, 0.5, None) != 0 and b"null" in err()
    for NW, C in ((0, 5), (3, 0)):
        assert sm(p, p, p, good, p, 3, NW, C, 4, 0.5, None) != 0 and b"bad shape" in err()
    for alpha in (1.0, 1.5, -0.1, float("nan"), float("inf")):
        assert sm(p, p, p, good, p, 3, 3, 5, 4, alpha, None) != 0 and b"alpha" in err(), alpha
    assert sm(p, p, p, good, p, 3, 2, 5, 4, 0.5, None) != 0 and b"not to NW" in err()
    assert sm(p, p, p, good, p, 3, 3, 1 << 30, 4, 0.5, None) != 0 and b"too large" in err()


def test_python_wrappers_reject_cpu_tensors_and_bad_tables(plib):
    import torch
    from clip_fsar_amd import pool_hip as ph
    host = torch.tensor(GOOD, dtype=torch.int32)
    table = ph.Table(host, host, 3)               # a device copy that is no device tensor
    with pytest.raises(RuntimeError, match="HIP device tensor"):
        ph.ring_put(torch.zeros(9, 8), torch.zeros(4, 16, 8), table)
    with pytest.raises(RuntimeError, match="shape"):
        ph.ring_put(torch.zeros(9, 8), torch.zeros(4, 16, 4), table)
    with pytest.raises(RuntimeError, match="shape"):
        ph.window_sequences(torch.zeros(4, 16, 8), torch.zeros(2, 4, 8), table, 3, 0, 3, 4, 2, 1)
    with pytest.raises(RuntimeError, match="shape"):
        ph.smooth_logits(torch.zeros(3, 5), torch.zeros(4, 6), torch.zeros(3, 5), table, 0.5)
    with pytest.raises(RuntimeError, match="Table"):
        ph.ring_put(torch.zeros(9, 8), torch.zeros(4, 16, 8), ph.Table(host[:, :7], host, 3))
    with pytest.raises(RuntimeError, match="1 .. 4 rows"):
        ph.TableUploader("cpu", 4).upload([[0] * 8] * 5)
    with pytest.raises(RuntimeError, match="1 .. 4 rows"):
        ph.TableUploader("cpu", 4).upload([])


# ------------------------------------------------------------------ the host plan against a model of the ring
def _stub_head(T=4, **train):
    engine = NS(arch={"embed": 8})
    return NS(args=NS(TRAIN=NS(**train), DATA=NS(NUM_INPUT_FRAMES=T)), _get_engine=lambda dev: engine, _engine_key=("stub",),
              arch_name="stub", precision="fp32", depth=1)


class _Model:
    """What the device does with a round's descriptor table, on frame LABELS instead of features: the ring holds (handle, frame number)."""

    def __init__(self, max_streams, cap):
        self.cap = cap
        self.ring = [[None] * cap for _ in range(max_streams)]

    def put(self, rows, labels):                  # labels: the round's packed frames
        for slot, put_pos, n, feat_off, _, _, _, _ in rows:
            for i in range(n):
                self.ring[slot][(put_pos + i) % self.cap] = labels[feat_off + i]

    def gather(self, rows, T, stride, rate):      # -> the packed window list, each window its T labels
        out = []
        for slot, _, _, _, win_pos, nW, win_off, _ in rows:
            assert win_off == len(out)
            out += [[self.ring[slot][(win_pos + w * stride + j * rate) % self.cap] for j in range(T)] for w in range(nW)]
        return out


@pytest.mark.parametrize("T,stride,rate,max_push", [(4, 1, 1, 3), (8, 2, 1, 8), (8, 3, 2, 5), (5, 9, 3, 4), (1, 1, 1, 1), (16, 16, 1, 6)])
def test_host_plan_against_a_brute_force_model(T, stride, rate, max_push):
    """random schedules of open / close / reset / uneven pushes (some beyond max_push): every window of every session once and in order,
    made of that session's own frames; slots reused; descriptor rows consistent; rounds of at most max_push frames per session"""
    from clip_fsar_amd.gallery import SupportGallery
    from clip_fsar_amd.pool import StreamPool, plan_push
    rng = random.Random(1000 * T + 10 * stride + rate)
    max_streams = 5
    pool = StreamPool(SupportGallery(_stub_head(T=T), "cpu"), max_streams=max_streams, stride=stride, rate=rate, max_push=max_push, smooth=0.5)
    cap = (T - 1) * rate + max_push
    assert pool.cap == cap and tuple(pool._ring.shape) == (max_streams, cap, 8)
    model = _Model(max_streams, cap)
    t, emitted, slots_seen, reused, multi_round = {}, {}, {}, 0, 0
    for step in range(400):
        op = rng.random()
        if (op < 0.12 or not t) and len(t) < max_streams:
            h = pool.open()
            slot = pool._session(h).slot
            assert slot == min(set(range(max_streams)) - {pool._session(o).slot for o in t})       # the lowest free slot
            reused += slot in slots_seen.values()
            slots_seen[h] = slot
            t[h], emitted[h] = 0, 0
            continue
        if op < 0.18 and t:
            h = rng.choice(sorted(t))
            pool.close(h)
            del t[h], emitted[h]
            with pytest.raises(ValueError, match="not open"):
                pool.close(h)
            continue
        if op < 0.22 and t:
            h = rng.choice(sorted(t))
            pool.reset(h)
            t[h], emitted[h] = 0, 0
            continue
        if not t:
            continue
        members = rng.sample(sorted(t), rng.randint(1, len(t)))                                  # any subset, in any order
        counts = [rng.choice((1, 1, 2, 3, max_push, max_push + 1, 2 * max_push + 2)) for _ in members]
        plan = plan_push([(pool._session(h).slot, t[h]) for h in members], counts, T, stride, rate, max_push, smoothing=True)
        labels = [(h, t[h] + i) for h, n in zip(members, counts) for i in range(n)]              # the push's packed frames
        assert len(plan.rounds) == -(-max(counts) // max_push)
        multi_round += len(plan.rounds) > 1
        windows, taken = [], {h: 0 for h in members}
        for rnd in plan.rounds:
            assert 1 <= len(rnd.rows) <= len(members) and len({r[0] for r in rnd.rows}) == len(rnd.rows)
            piece = []
            feat_off = win_off = 0
            for row, m, (f0, n) in zip(rnd.rows, rnd.members, rnd.src):
                h = members[m]
                slot, put_pos, rn, roff, win_pos, nW, woff, has_state = row
                assert slot == pool._session(h).slot and 1 <= rn == n <= max_push
                assert rn == min(max_push, counts[m] - taken[h])                                # round r: up to max_push of what is left
                assert put_pos == (t[h] + taken[h]) % cap and (roff, woff) == (feat_off, win_off)
                first = emitted[h] + sum(1 for w in windows if w[0] == h)
                assert win_pos == (first * stride) % cap and has_state == int(first > 0)
                assert labels[f0:f0 + n] == [(h, t[h] + taken[h] + i) for i in range(n)]
                piece += labels[f0:f0 + n]
                taken[h] += n
                feat_off, win_off = feat_off + n, win_off + nW
            model.put(rnd.rows, piece)
            got = model.gather(rnd.rows, T, stride, rate)
            for row, m in zip(rnd.rows, rnd.members):
                for w in got[row[6]:row[6] + row[5]]:
                    windows.append((members[m], w))
        # every window the push completes, per session: once, in order, made of the session's own frames
        order = plan.order if plan.order is not None else list(range(len(windows)))
        assert sorted(order) == list(range(len(windows)))
        result = [windows[g] for g in order]      # session-major
        pos = 0
        for m, h in enumerate(members):
            last = lambda k: k * stride + (T - 1) * rate
            want = [k for k in range(emitted[h], emitted[h] + counts[m] + 1) if t[h] <= last(k) < t[h] + counts[m]]
            assert plan.first_window[m] == emitted[h] and plan.n_windows[m] == len(want), (members, counts)
            for k in want:
                owner, frames = result[pos]
                assert owner == h and frames == [(h, k * stride + j * rate) for j in range(T)], (h, k, frames)
                pos += 1
            emitted[h] += len(want)
            t[h] += counts[m]
        assert pos == len(result)
    assert reused >= 3 and multi_round >= 10, (reused, multi_round)
    assert pool.stats()["open"] == len(t) and pool.sessions == sorted(t)


# ------------------------------------------------------------------ constructor and session errors (no GPU: a stub head)
def test_constructor_and_session_errors_on_a_stub_head():
    import torch
    from clip_fsar_amd.gallery import SupportGallery
    from clip_fsar_amd.pool import StreamPool
    from clip_fsar_amd.text_gallery import TextGallery
    g = SupportGallery(_stub_head(), "cpu")
    with pytest.raises(TypeError, match="SupportGallery or a TextGallery"):
        StreamPool(_stub_head())
    for kw in ({"max_streams": 0}, {"stride": 0}, {"rate": -1}, {"max_push": 0}, {"stride": 1.5}, {"max_streams": True}, {"max_streams": 1 << 17}):
        with pytest.raises(ValueError, match=list(kw)[0]):
            StreamPool(g, **kw)
    for smooth in (1.0, -0.1, 2.0, float("nan")):
        with pytest.raises(ValueError, match="smooth"):
            StreamPool(g, smooth=smooth)
    with pytest.raises(ValueError, match="at most 32"):
        StreamPool(SupportGallery(_stub_head(T=33), "cpu"))
    p = StreamPool(TextGallery(_stub_head(COMBINE=True), "cpu"), max_streams=3, stride=2, rate=3, max_push=5, smooth=0.25)
    assert (p.max_streams, p.T, p.E, p.cap) == (3, 4, 8, 3 * 3 + 5) and tuple(p._ring.shape) == (3, 14, 8)
    a, b, c = p.open(), p.open(), p.open()
    assert (a, b, c) == (0, 1, 2) and p.sessions == [0, 1, 2]
    with pytest.raises(RuntimeError, match="all 3 slots are in use"):
        p.open()
    assert p.stats(a) == {"frames": 0, "tower_frames": 0, "windows": 0}
    assert p.stats() == {"frames": 0, "tower_frames": 0, "windows": 0, "open": 3}
    p.close(b)
    d = p.open()
    assert d == 3 and p._session(d).slot == 1     # handles are never reused, slots are
    for bad in (b, 17, -1, "a", None, True):
        for call in (p.close, p.reset, p.stats) if bad is not None else (p.close, p.reset):
            with pytest.raises(ValueError, match="not open"):
                call(bad)
    frames = torch.zeros(2, 3, 4, 4)
    with pytest.raises(RuntimeError, match="no classes registered"):
        p.push({a: frames})
    p.gallery._ids.append(0)                      # a registered class: the push gets as far as its own checks
    with pytest.raises(ValueError, match="not open"):
        p.push({b: frames})
    with pytest.raises(ValueError, match="not open"):
        p.push_packed(frames, [a, b], [1, 1])
    with pytest.raises(ValueError, match="appears twice"):
        p.push_packed(frames, [a, a], [1, 1])
    with pytest.raises(ValueError, match="appears twice"):
        p.push_features_packed(torch.zeros(2, 8), [c, a, c], [1, 1, 1])
    with pytest.raises(RuntimeError, match="HIP device tensor"):
        p.push({a: frames})
    with pytest.raises(RuntimeError, match="HIP device tensor"):
        p.push_packed(frames, [a, c], [1, 1])
    with pytest.raises(RuntimeError, match="HIP device tensor"):
        p.push_features({a: torch.zeros(2, 8)})
    with pytest.raises(RuntimeError, match="HIP device tensor"):
        p.push_features_packed(torch.zeros(2, 8), [a], [2])
    with pytest.raises(ValueError, match="counts sum to 3"):
        p.push_packed(frames, [a, c], [1, 2])
    with pytest.raises(ValueError, match="counts sum to 1"):
        p.push_features_packed(torch.zeros(2, 8), [a], [1])
    with pytest.raises(ValueError, match="count >= 1"):
        p.push_packed(frames, [a, c], [2, 0])
    with pytest.raises(ValueError, match="count >= 1"):
        p.push_packed(frames, [a, c], [2])
    with pytest.raises(ValueError, match="non-empty dict"):
        p.push({})
    with pytest.raises(ValueError, match="non-empty dict"):
        p.push(frames)
    assert p.stats(a)["frames"] == 0              # nothing advanced
    p.gallery.head._engine_key = ("rebuilt",)
    with pytest.raises(RuntimeError, match="changed"):
        p.push({a: frames})
    with pytest.raises(RuntimeError, match="changed"):
        p.push_features_packed(torch.zeros(2, 8), [a], [2])
