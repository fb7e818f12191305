"""GPU: grouped scoring (libclipfsar_groups.so) -- the grouped cosine + OTAM kernel bit for bit against cfsl_otam_indexed group by group at
every tile edge, T form and search position, the grouped top-k against cfsg_topk; LiveGallery.classify_grouped against classify(classes=)
group by group; a StreamPool whose sessions have class lists of their own against gallery.classify on every session's materialised
windows, and a pool without lists bit for bit against the pool as it was before lists existed."""
import collections
import random

import pytest
import torch

from _cases import maxdiff
from test_gpu_gallery import BOUND, DEV, _features
from test_gpu_live import IDS, _pair, _videos
from test_gpu_pool import _ticks
from test_gpu_stream import _frames, _materialised, _n_windows

pytestmark = pytest.mark.gpu
SENTINEL = -12345.0


# ------------------------------------------------------------------ 1: the grouped kernel against the indexed kernel, group by group
def _problem(counts, widths, cap, T, E, seed):
    """Queries of all groups packed, a store of cap slots whose slots outside the lists are NaN (prototypes and norms), and per group a
    random list of distinct slots -> (xq, qn, Ps, pns, lists)"""
    from clip_fsar_amd import gallery_hip as gh
    rng = random.Random(seed)
    lists = [rng.sample(range(cap), w) for w in widths]
    used = sorted({s for l in lists for s in l})
    Xq, P = _features(max(1, sum(counts)), len(used), T, E, seed=seed)
    xq, p = Xq.to(DEV), P.to(DEV)
    qn, pn = torch.empty(xq.shape[0] * T, device=DEV), torch.empty(len(used) * T, device=DEV)
    gh.row_norms(xq, qn)
    gh.row_norms(p, pn)
    Ps = torch.full((cap, T, E), float("nan"), device=DEV)
    pns = torch.full((cap, T), float("nan"), device=DEV)
    idx = torch.tensor(used, device=DEV)
    Ps[idx], pns[idx] = p, pn.view(-1, T)
    return xq, qn, Ps, pns.reshape(-1).contiguous(), lists


def _grouped(xq, qn, Ps, pns, counts, lists, T, sd, pad=37):
    """one grouped launch -> (flat logits allocated `pad` beyond NOUT and pre-filled with the sentinel, rows, NOUT)"""
    from clip_fsar_amd import groups_hip as grh
    rows, (nq, ncols, _, n_out) = grh.table_rows(counts, [len(l) for l in lists], T)
    assert nq == xq.shape[0]
    cols = torch.tensor([s for l in lists for s in l], device=DEV, dtype=torch.int32)
    out = torch.full((n_out + pad,), SENTINEL, device=DEV)
    grh.otam_grouped(xq, qn, Ps, pns, cols, out, grh.table_uploader(DEV, len(rows)).upload(rows), n_out, 0.5, sd)
    return out, rows, n_out


def _indexed(xq, qn, Ps, pns, counts, lists, T, sd):
    """the reference: one cfsl_otam_indexed launch per group with queries -> the groups' blocks, flat, in order"""
    from clip_fsar_amd import live_hip as lh
    blocks, q = [], 0
    for n, l in zip(counts, lists):
        if n:
            lg = torch.empty(n, len(l), device=DEV)
            lh.otam_indexed(xq[q:q + n], qn[q * T:(q + n) * T], Ps, pns, torch.tensor(l, device=DEV, dtype=torch.int32), lg, 0.5, sd)
            blocks.append(lg.reshape(-1))
        q += n
    return torch.cat(blocks)


def _check(counts, widths, cap, T, E, seed):
    xq, qn, Ps, pns, lists = _problem(counts, widths, cap, T, E, seed)
    for sd in (False, True):
        out, rows, n_out = _grouped(xq, qn, Ps, pns, counts, lists, T, sd)
        want = _indexed(xq, qn, Ps, pns, counts, lists, T, sd)
        torch.cuda.synchronize()
        assert want.shape[0] == n_out
        assert bool(torch.isfinite(out[:n_out]).all()), "a slot outside the lists was read, or a logit was not written"
        assert bool((out[n_out:] == SENTINEL).all()) and not bool((out[:n_out] == SENTINEL).any())
        assert torch.equal(out[:n_out], want), (T, E, sd, maxdiff(out[:n_out].cpu(), want.cpu()))


def _edges(T):
    """the issue's pattern scaled to QB = the videos along a tile's side: one pair, one full tile, one past it, a group without queries,
    and several tiles both ways; 10 QB + 6 columns from a store of 8 QB + 6 slots, so the lists overlap"""
    qb = min(64 // T, 16)
    return [1, qb, qb + 1, 0, 2 * qb + 1], [1, qb, qb + 1, 3, 8 * qb + 1], 8 * qb + 6


#             T   E
EDGE_CASES = [(8, 64), (8, 36),            # QB 8; E = 36: a partial K chunk
              (16, 64),                    # QB 4
              (5, 36),                     # QB 12, run-time T, 60 of 64 tile rows
              (32, 64),                    # QB 2
              (1, 64),                     # QB 16
              (8, 512)]


@pytest.mark.parametrize("T,E", EDGE_CASES)
def test_grouped_kernel_equals_indexed_kernel_group_by_group(T, E):
    counts, widths, cap = _edges(T)
    if T == 8:
        assert (counts, widths, cap) == ([1, 8, 9, 0, 17], [1, 8, 9, 3, 65], 70) and sum(widths) == 86
    _check(counts, widths, cap, T, E, seed=T * 1000 + E)


def test_groups_without_queries_first_in_the_middle_and_last():
    _check([0, 3, 0, 9, 0], [2, 5, 8, 3, 4], 12, 8, 64, seed=1)
    _check([0, 0, 1], [70, 1, 9], 70, 16, 64, seed=2)


def test_three_hundred_random_groups():
    """the search over TILE0: 300 groups of 0 .. 12 queries and 1 .. 20 slots, about a seventh of them without queries"""
    rng = random.Random(300)
    counts = [rng.choice([0, 1, 2, 3, 5, 8, 12]) for _ in range(300)]
    widths = [rng.randint(1, 20) for _ in range(300)]
    assert counts.count(0) >= 20
    _check(counts, widths, 50, 8, 32, seed=300)


@pytest.mark.parametrize("bad", [70, -1, 1 << 30])
def test_a_slot_out_of_range_poisons_its_column_in_its_group_alone(bad):
    T, E = 8, 64
    counts, widths, cap = _edges(T)
    xq, qn, Ps, pns, lists = _problem(counts, widths, cap, T, E, seed=9)
    good, rows, n_out = _grouped(xq, qn, Ps, pns, counts, lists, T, False)
    for g, j in ((0, 0), (2, 8), (4, 31), (3, 1)):            # the last one: a group without queries, nothing to poison
        broken = [list(l) for l in lists]
        broken[g][j] = bad
        out, _, _ = _grouped(xq, qn, Ps, pns, counts, broken, T, False)
        torch.cuda.synchronize()
        lo, w = rows[g][5], widths[g]
        hit = torch.zeros(n_out, dtype=torch.bool, device=DEV)
        hit[lo:lo + counts[g] * w].view(counts[g], w)[:, j] = True
        assert int(hit.sum()) == counts[g]
        assert bool(torch.isnan(out[:n_out][hit]).all()) and torch.equal(out[:n_out][~hit], good[:n_out][~hit]), (bad, g, j)
        assert bool((out[n_out:] == SENTINEL).all())


# ------------------------------------------------------------------ 2: the grouped top-k against cfsg_topk on every group's dense block
@pytest.mark.parametrize("k", [1, 5, 16])
def test_grouped_topk_equals_topk_of_every_block(k):
    from clip_fsar_amd import gallery_hip as gh
    from clip_fsar_amd import groups_hip as grh
    counts, widths = [3, 1, 5, 0, 2, 0], [20, 70, 16, 3, 130, 40]          # the narrow group has no queries: k = 16 is allowed
    rows, (nq, _, _, n_out) = grh.table_rows(counts, widths, 8)
    g = torch.Generator().manual_seed(k)
    logits = (torch.randint(-40, 0, (n_out + 5,), generator=g).float() / 4).to(DEV)       # 40 values: ties in every row of 70 and 130
    logits[rows[4][5] + 3] = float("nan")                                                  # never selected
    logits[rows[4][5] + 7] = float("-inf")
    values = torch.full((nq, k), SENTINEL, device=DEV)
    index = torch.full((nq, k), -7, device=DEV, dtype=torch.int32)
    grh.topk_grouped(logits, grh.table_uploader(DEV, 8).upload(rows), nq, n_out, k, values, index)
    for r in rows:
        q0, n, w, lo = r[0], r[1], r[3], r[5]
        if n:
            v, i = torch.empty(n, k, device=DEV), torch.empty(n, k, device=DEV, dtype=torch.int32)
            gh.topk(logits[lo:lo + n * w].view(n, w).contiguous(), k, v, i)
            assert torch.equal(values[q0:q0 + n], v) and torch.equal(index[q0:q0 + n], i), r
            sv, si = torch.sort(torch.nan_to_num(logits[lo:lo + n * w].view(n, w), nan=float("-inf")), dim=1, descending=True, stable=True)
            assert torch.equal(v, sv[:, :k]) and torch.equal(i.long(), si[:, :k])          # and that is the stable descending sort


# ------------------------------------------------------------------ 3: the gallery
T = 8
GALLERY_CONFIGS = [("fp32", False), ("bf16", False), ("fp32", True)]


def _against_classify(live, Q, counts, classes, what):
    """classify_grouped against classify(q_i, classes=c_i) group by group: 2e-5 ("same clip, another batch") and equal argmax"""
    res = live.classify_grouped(Q, counts, classes)
    assert len(res) == len(counts) and res.counts == counts and res.offsets[0] == 0 and res.offsets[-1] == res.logits.shape[0]
    worst, q = 0.0, 0
    for i, (n, c) in enumerate(zip(counts, classes)):
        blk = res.group(i)
        assert tuple(blk.shape) == (n, len(live) if c is None else len(c)) and res.widths[i] == blk.shape[1]
        if n:
            ref = live.classify(Q[q:q + n], classes=c)
            worst = max(worst, maxdiff(blk.cpu(), ref.cpu()))
            assert torch.equal(blk.argmax(1), ref.argmax(1)), (what, i)
        q += n
    print("%s: |classify_grouped - classify(classes=)| = %.2e over %d groups, %d clips" % (what, worst, len(counts), q))
    assert bool(torch.isfinite(res.logits).all()) and worst <= BOUND, (what, worst)
    return res


@pytest.mark.parametrize("precision,merge_before", GALLERY_CONFIGS)
def test_classify_grouped_equals_classify_group_by_group(precision, merge_before, monkeypatch):
    V, Q, W = _videos(12, 61), _videos(11, 62), _videos(2, 63)
    counts = [3, 1, 0, 5, 2]
    with torch.no_grad():
        head, live, _ = _pair(precision, merge_before, capacity=4)
        live.add_classes(V, IDS)                                    # classes 0 1 2 5 7 9
        classes = [[9, 0, 5], None, [1], [7], [2, 9, 1, 0, 7, 5]]
        tag = "%s merge_before=%d" % (precision, merge_before)
        res = _against_classify(live, Q, counts, classes, tag)
        feats = torch.empty(11, T, live.E, device=DEV)
        live._features(live._fresh_engine(), Q, feats)
        assert torch.equal(live.classify_features_grouped(feats, counts, classes).logits, res.logits)
        # a class removed and a class added between two calls: class 0's slot goes to class 11, the lists follow the ids
        live.remove_classes([0, 5])
        live.add_classes(W, [11, 11])
        with pytest.raises(ValueError, match="group 0: class 0 is not registered"):
            live.classify_grouped(Q, counts, classes)
        classes = [[9, 11], None, [1], [11, 7], [2, 9, 1, 11, 7]]
        again = _against_classify(live, Q, counts, classes, tag + ", after remove + add")
        assert again.widths == [2, 5, 1, 2, 5] and live.class_ids == [1, 2, 7, 9, 11]
        # top-k per query within its own list: the stable descending sort of its row
        vals, idx = live.topk_grouped(Q, counts, classes, k=2)
        with pytest.raises(ValueError, match="shortest class list"):
            live.topk_grouped(Q, counts, classes, k=3)
        q = 0
        for i, n in enumerate(counts):
            if n:
                sv, si = torch.sort(again.group(i), dim=1, descending=True, stable=True)
                assert torch.equal(vals[q:q + n], sv[:, :2]) and torch.equal(idx[q:q + n].long(), si[:, :2]), i
            q += n
        assert q == vals.shape[0] == idx.shape[0]
        # chunks of 3 clips: they start and end inside groups, and one lies inside the group of 5
        monkeypatch.setattr(live._fresh_engine(), "max_frames", 3 * T)
        _against_classify(live, Q, counts, classes, tag + ", chunks of 3 clips")


# ------------------------------------------------------------------ 4: the pool
ARCH, STRIDE, RATE, MAX_PUSH = "ViT-test/16", 2, 2, 6
SIZES = {"a": (80, 112), "b": (64, 64), "c": (97, 131), "d": (72, 96)}       # push_u8: every session its own source resolution
SCALE, CROP, MEAN, STD = [72, 96], 64, (0.45, 0.45, 0.45), (0.225, 0.225, 0.225)
#        two sessions with lists, one with None, and the reused slot's new owner (d takes b's slot) with another list
LISTS = {"a": [9, 0, 5], "b": [7, 2], "c": None, "d": [1, 9, 7, 0]}


def _schedule(pool, ticks, content, call, lists):
    """test_gpu_pool._run_schedule with open(classes=lists[name]) and the push left to `call(pool, {handle: rows})`
    -> ({(name, epoch): (frames pushed, first frame, [StreamOutput])}, handles)"""
    h, used, epoch, start, outs = {}, collections.defaultdict(int), collections.defaultdict(int), {}, {}
    for name in ("a", "b"):
        h[name] = pool.open(classes=lists[name])
    for op, tick in ticks:
        if op == "open c":
            h["c"] = pool.open(classes=lists["c"])
        elif op == "close b, open d":
            slot = pool._session(h["b"]).slot
            pool.close(h.pop("b"))
            h["d"] = pool.open(classes=lists["d"])
            assert pool._session(h["d"]).slot == slot                         # the freed slot, with the previous owner's frames in it
        elif op == "reset a":
            pool.reset(h["a"])
            epoch["a"] += 1
        got = call(pool, {h[name]: content[name][used[name]:used[name] + n] for name, n in tick.items()})
        assert list(got) == [h[name] for name in tick]
        for name, n in tick.items():
            rec = outs.setdefault((name, epoch[name]), [0, used[name], []])
            rec[0] += n
            rec[2].append(got[h[name]])
            used[name] += n
    return outs, h


class _PoolBeforeLists:
    """StreamPool._run as it was before sessions could have class lists, kept here as the reference of the pool without lists"""

    @staticmethod
    def run(self, eng, feats, handles, recs, counts):
        from clip_fsar_amd import pool_hip as php
        from clip_fsar_amd.pool import PackedOutput, plan_push
        g, T, C = self.gallery, self.T, len(self.gallery)
        plan = plan_push([(s.slot, s.t) for s in recs], counts, T, self.stride, self.rate, self.max_push, smoothing=bool(self.alpha))
        NW = sum(plan.n_windows)
        logits = torch.empty(NW, C, device=self.dev, dtype=torch.float32)
        per = max(1, eng.max_frames // T)
        g0 = 0
        for rnd in plan.rounds:
            piece = feats if len(plan.rounds) == 1 else torch.cat([feats[f0:f0 + n] for f0, n in rnd.src], 0)
            table = self._tables.upload(rnd.rows)
            php.ring_put(piece, self._ring, table)
            nW = sum(r[php.NW] for r in rnd.rows)
            if nW == 0:
                continue
            if self._X is None or self._X.shape[0] < min(nW, per):
                self._X = torch.empty(min(nW, per), T, self.E, device=self.dev, dtype=torch.float32)
            out = logits[g0:g0 + nW]
            for w0 in range(0, nW, per):
                w1 = min(nW, w0 + per)
                X = self._X[:w1 - w0]
                php.window_sequences(self._ring, X, table, nW, w0, w1, T, self.stride, self.rate)
                out[w0:w1].copy_(g.classify_features(X))
            g0 += nW
        if plan.order is not None and NW:
            logits = logits.index_select(0, torch.tensor(plan.order, device=self.dev))
        offsets = [0]
        for s, n, nW in zip(recs, counts, plan.n_windows):
            s.t += n
            offsets.append(offsets[-1] + nW)
        self._totals["frames"] += sum(counts)
        self._totals["windows"] += NW
        return PackedOutput(handles, plan.first_window, offsets, logits, None)


def _pool_setup(precision, merge_before):
    head, live, _ = _pair(precision, merge_before, capacity=8)
    live.add_classes(_videos(12, 71), IDS)
    span = (T - 1) * RATE + 1
    ticks = _ticks(span, STRIDE)
    assert max(n for _, t in ticks for n in t.values()) == 17 and min(n for _, t in ticks for n in t.values()) == 1
    need = collections.defaultdict(int)
    for _, tick in ticks:
        for name, n in tick.items():
            need[name] += n
    return head, live, ticks, need


@pytest.mark.parametrize("precision,merge_before", GALLERY_CONFIGS)
def test_pool_with_class_lists_equals_classify_on_materialised_windows(precision, merge_before):
    """The four-session schedule of the pool's contract test (joins, a close with slot reuse, a reset, skipped ticks, pushes of 1 to 17
    frames at max_push = 6) through push, push_features and push_u8: every session's logits against gallery.classify of its
    materialised windows with its list, 2e-5 and equal argmax; first windows, window counts and stats are the pool's without lists."""
    from clip_fsar_amd.pool import StreamPool
    from clip_fsar_amd.preprocess import preprocess_video
    with torch.no_grad():
        head, live, ticks, need = _pool_setup(precision, merge_before)
        data = head.args.DATA
        data.TEST_SCALE, data.TEST_CROP_SIZE, data.MEAN, data.STD = SCALE, CROP, list(MEAN), list(STD)
        u8 = {name: torch.randint(0, 256, (n, *SIZES[name], 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(ord(name)))
              for name, n in need.items()}
        frames = {name: preprocess_video(c.to(DEV), SCALE, CROP, MEAN, STD) for name, c in u8.items()}
        eng = live._fresh_engine()
        feats = {name: torch.empty(fr.shape[0], live.E, device=DEV) for name, fr in frames.items()}
        for name, fr in frames.items():
            eng.vit.forward(fr.contiguous(), feats[name])
        legs = {"push": (frames, lambda pool, arg: pool.push(arg)), "push_features": (feats, lambda pool, arg: pool.push_features(arg)),
                "push_u8": (u8, lambda pool, arg: pool.push_u8(arg))}
        plain = StreamPool(live, max_streams=3, stride=STRIDE, rate=RATE, max_push=MAX_PUSH)
        base, hb = _schedule(plain, ticks, frames, legs["push"][1], dict.fromkeys(LISTS))
        refs = {}                                                               # classify of a session's windows, once for all legs
        for leg, (content, call) in legs.items():
            pool = StreamPool(live, max_streams=3, stride=STRIDE, rate=RATE, max_push=MAX_PUSH)
            outs, h = _schedule(pool, ticks, content, call, LISTS)
            worst, windows = 0.0, 0
            assert sorted(outs) == sorted(base)
            for key, (n, f0, pieces) in sorted(outs.items()):
                name = key[0]
                width = len(live) if LISTS[name] is None else len(LISTS[name])
                assert [o.first_window for o in pieces] == [o.first_window for o in base[key][2]], key
                assert [o.logits.shape[0] for o in pieces] == [o.logits.shape[0] for o in base[key][2]], key
                assert all(o.logits.shape[1] == width and o.smoothed is None for o in pieces), key
                nW = _n_windows(n, T, STRIDE, RATE)
                assert sum(o.logits.shape[0] for o in pieces) == nW
                if nW == 0:
                    continue
                if key not in refs:
                    refs[key] = live.classify(_materialised(frames[name][None, f0:f0 + n], T, STRIDE, RATE, nW), classes=LISTS[name])
                got = torch.cat([o.logits for o in pieces])
                worst = max(worst, maxdiff(got.cpu(), refs[key].cpu()))
                assert torch.equal(got.argmax(1), refs[key].argmax(1)), (leg, key)
                windows += nW
            print("%s merge_before=%d %s: |pool with lists - classify(classes=)| = %.2e over %d windows" % (
                precision, merge_before, leg, worst, windows))
            assert worst <= BOUND and windows > 20, (leg, worst, windows)
            tower = leg != "push_features"
            for name in h:
                want = dict(plain.stats(hb[name]), tower_frames=plain.stats(hb[name])["tower_frames"] if tower else 0)
                assert pool.stats(h[name]) == want, (leg, name)
            assert pool.stats() == dict(plain.stats(), tower_frames=plain.stats()["tower_frames"] if tower else 0)


def test_packed_output_of_a_push_with_lists_order_topk_and_late_errors():
    """pushes beyond max_push (several rounds, the round order differing from the session order) stay session-major with windows
    ascending; the packed tuple, top-k within each session's list; a list naming a removed class raises at the push, before any launch"""
    from clip_fsar_amd.pool import GroupedPackedOutput, PackedOutput, StreamPool
    with torch.no_grad():
        head, live, _, _ = _pool_setup("fp32", False)
        fr = _frames(ARCH, 3, 40, seed=81)
        pool = StreamPool(live, max_streams=3, stride=STRIDE, rate=RATE, max_push=MAX_PUSH)
        a, b, c = pool.open(classes=[5, 9]), pool.open(), pool.open(classes=[2, 0, 1, 7])
        counts = [3, 33, 17]                                        # a: no window; b: 6 rounds; c: its first window arrives in round 3
        po = pool.push_packed(torch.cat([fr[0, :3], fr[1, :33], fr[2, :17]]), [a, b, c], counts)
        nW = [_n_windows(n, T, STRIDE, RATE) for n in counts]
        assert isinstance(po, GroupedPackedOutput) and nW == [0, 10, 2]
        assert po.sessions == [a, b, c] and po.first_window == [0, 0, 0] and po.offsets == [0, 0, 10, 12]
        assert po.widths == [2, 6, 4] and po.logit_offsets == [0, 0, 60, 68] and tuple(po.logits.shape) == (68,)
        ref_b = live.classify(_materialised(fr[1:2, :33], T, STRIDE, RATE, 10))
        ref_c = live.classify(_materialised(fr[2:3, :17], T, STRIDE, RATE, 2), classes=[2, 0, 1, 7])
        d = max(maxdiff(po.logits[:60].view(10, 6).cpu(), ref_b.cpu()), maxdiff(po.logits[60:].view(2, 4).cpu(), ref_c.cpu()))
        print("several rounds, session-major: |pool with lists - classify| = %.2e" % d)
        assert d <= BOUND
        vals, idx = pool.topk(po, k=3)
        sv, si = torch.sort(po.logits[:60].view(10, 6), dim=1, descending=True, stable=True)
        assert torch.equal(vals[:10], sv[:, :3]) and torch.equal(idx[:10].long(), si[:, :3])
        sv, si = torch.sort(po.logits[60:].view(2, 4), dim=1, descending=True, stable=True)
        assert torch.equal(vals[10:], sv[:, :3]) and torch.equal(idx[10:].long(), si[:, :3])
        with pytest.raises(ValueError, match="shortest class list"):
            pool.topk(po, k=5)
        # a session's windows spread over rounds again, then a push of sessions without lists: a PackedOutput as ever
        po2 = pool.push_packed(torch.cat([fr[0, 3:17], fr[2, 17:19]]), [a, c], [14, 2])
        assert po2.offsets == [0, 2, 3] and po2.widths == [2, 4] and po2.first_window == [0, 2] and tuple(po2.logits.shape) == (8,)
        ref_a = live.classify(_materialised(fr[0:1, :17], T, STRIDE, RATE, 2), classes=[5, 9])
        assert maxdiff(po2.logits[:4].view(2, 2).cpu(), ref_a.cpu()) <= BOUND
        assert isinstance(pool.push_packed(fr[1, 33:35], [b], [2]), PackedOutput)
        # a class of c's list leaves: the push raises, names the session, and nothing has advanced
        live.remove_classes([1])
        before = (pool.stats(), pool.stats(c), pool.stats(b))
        with pytest.raises(ValueError, match="session %d: class 1 is not registered" % c):
            pool.push({b: fr[1, 35:36], c: fr[2, 19:20]})
        assert (pool.stats(), pool.stats(c), pool.stats(b)) == before
        out = pool.push({b: fr[1, 35:37], a: fr[0, 17:19]})          # the others go on, with one column fewer where there is no list
        assert tuple(out[b].logits.shape) == (1, 5) and tuple(out[a].logits.shape) == (1, 2)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_pool_without_lists_is_the_pool_as_it_was(precision, monkeypatch):
    """no session has a list: the push takes the dense path (the grouped one is never entered, the result is a PackedOutput) and its
    logits are, bit for bit, those of StreamPool._run as it was before class lists -- the same launches in the same order"""
    from clip_fsar_amd.pool import PackedOutput, StreamPool
    with torch.no_grad():
        head, live, ticks, need = _pool_setup(precision, False)
        content = {name: _frames(ARCH, 1, n, seed=90 + i)[0] for i, (name, n) in enumerate(sorted(need.items()))}
        results = {}
        for which in ("now", "before"):
            pool = StreamPool(live, max_streams=3, stride=STRIDE, rate=RATE, max_push=MAX_PUSH)
            monkeypatch.setattr(pool, "_run_grouped", None)                   # entering it would raise
            if which == "before":
                monkeypatch.setattr(pool, "_run", _PoolBeforeLists.run.__get__(pool))
            packed = []

            def call(pool, arg):
                po = pool.push_packed(torch.cat(list(arg.values())), list(arg), [v.shape[0] for v in arg.values()])
                packed.append(po)
                return StreamPool._split(po)

            _schedule(pool, ticks, content, call, dict.fromkeys(LISTS))
            results[which] = (packed, pool.stats())
        assert results["now"][1] == results["before"][1]
        rows = 0
        for x, y in zip(*(results[w][0] for w in ("now", "before"))):
            assert isinstance(x, PackedOutput) and x.smoothed is None
            assert x.sessions == y.sessions and x.first_window == y.first_window and x.offsets == y.offsets
            assert torch.equal(x.logits, y.logits)
            rows += x.logits.shape[0]
        assert rows > 20
