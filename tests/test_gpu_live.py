"""GPU: the live gallery (clip_fsar_amd.live_gallery.LiveGallery on libclipfsar_live.so) -- the indexed cosine + OTAM kernel against the
dense kernel on the gathered store (bit for bit) and against the float64 restatement, the running class sums against cfsg_segment_mean,
LiveGallery against SupportGallery on the same calls, removal, subsets, further shots, state dicts, and a StreamPool over it."""
import pytest
import torch

import clip_fsar_amd.synth as synth
from _cases import maxdiff
from test_gpu_gallery import BOUND, DEV, _features, _head, _restated

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ 1: the indexed kernel
def _store(P, cap, cols, T, E):
    """(P_store [cap, T, E], pn_store [cap * T]) holding P[j] at slot cols[j]; every other slot is NaN, prototypes and norms"""
    from clip_fsar_amd import gallery_hip as gh
    pn = torch.empty(P.shape[0] * T, device=DEV)
    gh.row_norms(P, pn)
    Ps = torch.full((cap, T, E), float("nan"), device=DEV)
    pns = torch.full((cap, T), float("nan"), device=DEV)
    idx = torch.tensor(cols, device=DEV)
    Ps[idx] = P
    pns[idx] = pn.view(-1, T)
    return Ps, pns.reshape(-1).contiguous(), pn


#                 NQ  C   cap  T   E
INDEXED_SHAPES = [(9, 11, 40, 8, 64),        # ragged tile in both directions
                  (5, 3, 7, 16, 96),         # C below a tile's 4 classes
                  (13, 25, 64, 5, 36),       # run-time T; 60 of 64 tile rows; E not a multiple of the 32-float chunk
                  (3, 5, 9, 32, 64),         # two videos per tile
                  (70, 130, 300, 8, 128)]    # several tiles each way


@pytest.mark.parametrize("NQ,C,cap,T,E", INDEXED_SHAPES)
def test_indexed_kernel_equals_dense_kernel_on_the_gathered_store(NQ, C, cap, T, E):
    from clip_fsar_amd import gallery_hip as gh
    from clip_fsar_amd import live_hip as lh
    Xq, P = _features(NQ, C, T, E, seed=NQ * 7 + C)
    xq, p = Xq.to(DEV), P.to(DEV)
    qn = torch.empty(NQ * T, device=DEV)
    gh.row_norms(xq, qn)
    g = torch.Generator().manual_seed(cap)
    subset = torch.randperm(cap, generator=g)[:C].tolist()          # a random permutation of a random subset of the slots
    for cols, n_slots in ((subset, cap), (list(range(C)), C)):       # ... and the identity with cap == C
        Ps, pns, pn = _store(p, n_slots, cols, T, E)
        cd = torch.tensor(cols, device=DEV, dtype=torch.int32)
        for sd in (False, True):
            dense = torch.empty(NQ, C, device=DEV)
            gh.otam_gallery(xq, qn, Ps[cd.long()].contiguous(), pns.view(-1, T)[cd.long()].reshape(-1).contiguous(), dense, 0.5, sd)
            lg = torch.full((NQ, C), 7.0, device=DEV)
            lh.otam_indexed(xq, qn, Ps, pns, cd, lg, 0.5, sd)
            torch.cuda.synchronize()
            assert bool(torch.isfinite(lg).all()), "a slot outside cols was read"
            assert torch.equal(lg, dense), (n_slots, sd, maxdiff(lg.cpu(), dense.cpu()))


def test_indexed_kernel_against_the_float64_restatement():
    from clip_fsar_amd import gallery_hip as gh
    from clip_fsar_amd import live_hip as lh
    NQ, C, cap, T, E = INDEXED_SHAPES[0]
    Xq, P = _features(NQ, C, T, E, seed=5)
    xq = Xq.to(DEV)
    qn = torch.empty(NQ * T, device=DEV)
    gh.row_norms(xq, qn)
    cols = torch.randperm(cap, generator=torch.Generator().manual_seed(1))[:C].tolist()
    Ps, pns, _ = _store(P.to(DEV), cap, cols, T, E)
    for sd in (False, True):
        ref, _ = _restated(Xq, P, sd)
        lg = torch.empty(NQ, C, device=DEV)
        lh.otam_indexed(xq, qn, Ps, pns, torch.tensor(cols, device=DEV, dtype=torch.int32), lg, 0.5, sd)
        torch.cuda.synchronize()
        e = float((lg.cpu().double() - ref).abs().max())
        print("indexed kernel NQ %d C %d cap %d T %d E %d single_direct %d: |dlogits| vs float64 %.2e" % (NQ, C, cap, T, E, sd, e))
        assert e <= BOUND, e


@pytest.mark.parametrize("bad", [40, -1, 1 << 30])
def test_a_slot_out_of_range_poisons_its_column_alone(bad):
    from clip_fsar_amd import gallery_hip as gh
    from clip_fsar_amd import live_hip as lh
    NQ, C, cap, T, E = INDEXED_SHAPES[0]
    Xq, P = _features(NQ, C, T, E, seed=9)
    xq = Xq.to(DEV)
    qn = torch.empty(NQ * T, device=DEV)
    gh.row_norms(xq, qn)
    cols = torch.randperm(cap, generator=torch.Generator().manual_seed(2))[:C].tolist()
    Ps, pns, _ = _store(P.to(DEV), cap, cols, T, E)
    good = torch.empty(NQ, C, device=DEV)
    lh.otam_indexed(xq, qn, Ps, pns, torch.tensor(cols, device=DEV, dtype=torch.int32), good)
    for j in (0, 6, C - 1):
        broken = list(cols)
        broken[j] = bad
        lg = torch.empty(NQ, C, device=DEV)
        lh.otam_indexed(xq, qn, Ps, pns, torch.tensor(broken, device=DEV, dtype=torch.int32), lg)
        torch.cuda.synchronize()
        keep = [c for c in range(C) if c != j]
        assert bool(torch.isnan(lg[:, j]).all()) and torch.equal(lg[:, keep], good[:, keep]), (bad, j)


# ------------------------------------------------------------------ 2: running sums, means, norms
@pytest.mark.parametrize("E", [64, 36])
@pytest.mark.parametrize("rows_kept", [8, 9])
def test_accumulate_continues_segment_mean_bit_for_bit(E, rows_kept):
    """11 videos over 4 classes in slots 5, 0, 6, 2 of 8, delivered at once and in three uneven calls: sums and means are those of one
    cfsg_segment_mean over each class's videos in order, untouched slots stay untouched, norms are cfsg_row_norms'"""
    from clip_fsar_amd import gallery_hip as gh
    from clip_fsar_amd import live_hip as lh
    Nv, L, cap, slots, counts = 11, 9, 8, [5, 0, 6, 2], [3, 1, 5, 2]
    g = torch.Generator().manual_seed(E + rows_kept)
    X = (torch.randn(Nv, L, E, generator=g) * 3).to(DEV)
    starts = [0, 3, 4, 9]
    vids = [list(range(s, s + n)) for s, n in zip(starts, counts)]
    ref_mean = torch.empty(4, rows_kept, E, device=DEV)
    gh.segment_mean(X, torch.tensor(starts + [Nv], device=DEV, dtype=torch.int32), ref_mean)
    ref_norm = torch.empty(4 * rows_kept, device=DEV)
    gh.row_norms(ref_mean, ref_norm)
    up = lh.table_uploader(DEV, 8)
    # every call: per class how many of its next videos it brings.  One call; three uneven calls, the second with a single video,
    # the second and third skipping a class
    for calls in ([counts], [[1, 1, 2, 0], [0, 0, 1, 0], [2, 0, 2, 2]]):
        sums = torch.full((cap, L, E), 123.0, device=DEV)
        means = torch.full((cap, rows_kept, E), 321.0, device=DEV)
        norms = torch.full((cap * rows_kept,), 5.0, device=DEV)
        packed = None
        done = [0, 0, 0, 0]
        for call in calls:
            rows, pick, off = [], [], 0
            for c in range(4):
                if call[c]:
                    rows.append([slots[c], off, call[c], done[c]])
                    pick += vids[c][done[c]:done[c] + call[c]]
                    off += call[c]
                    done[c] += call[c]
            table = up.upload(rows)
            x = X[torch.tensor(pick, device=DEV)].contiguous()
            lh.accumulate(x, sums, means, table, by_slot=True)
            lh.slot_norms(means, norms, table)
            if len(calls) == 1:                   # the packed form of the means, as MERGE_BEFORE uses it
                packed = torch.empty(4, rows_kept, E, device=DEV)
                lh.accumulate(x, sums.clone(), packed, table, by_slot=False)
        torch.cuda.synchronize()
        assert done == counts
        for c, s in enumerate(slots):
            total = X[vids[c][0]]
            for v in vids[c][1:]:
                total = total + X[v]               # fp32 adds in video order: cfsg_segment_mean's sum
            assert torch.equal(sums[s, :rows_kept], total[:rows_kept]), (len(calls), c)
            assert torch.equal(means[s], ref_mean[c]), (len(calls), c)
            assert torch.equal(norms[s * rows_kept:(s + 1) * rows_kept], ref_norm[c * rows_kept:(c + 1) * rows_kept]), (len(calls), c)
            assert bool((sums[s, rows_kept:] == 123.0).all())
        if packed is not None:
            assert torch.equal(packed, ref_mean)
        for s in (1, 3, 4, 7):                     # untouched slots stay untouched
            assert bool((sums[s] == 123.0).all()) and bool((means[s] == 321.0).all())
            assert bool((norms[s * rows_kept:(s + 1) * rows_kept] == 5.0).all())


# ------------------------------------------------------------------ 3: the gallery
ARCH, T = "ViT-test/16", 8
IDS = [0, 0, 1, 2, 2, 2, 5, 5, 7, 9, 9, 9]
CONFIGS = [("fp32", False, False), ("bf16", False, False), ("fp32", True, False), ("fp32", False, True)]


def _pair(precision="fp32", merge_before=False, single_direct=False, capacity=4):
    from clip_fsar_amd.gallery import SupportGallery
    from clip_fsar_amd.live_gallery import LiveGallery
    head = _head(ARCH, precision, T)
    head.args.TRAIN.MERGE_BEFORE = merge_before
    head.args.TRAIN.SINGLE_DIRECT = single_direct
    return head, LiveGallery(head, DEV, capacity=capacity), SupportGallery(head, DEV)


def _videos(n, seed):
    a = synth.ARCHS[ARCH]
    return (torch.randn(n, T, 3, a["res"], a["res"], generator=torch.Generator().manual_seed(seed)) * 0.5).to(DEV)


def _dense(live):
    """(prototypes, norms) of a LiveGallery in column order"""
    idx = torch.tensor([live.slot_of(c) for c in live.class_ids], device=DEV)
    return live._store["P"][idx], live._store["pn"].view(-1, T)[idx].reshape(-1)


@pytest.mark.parametrize("precision,merge_before,single_direct", CONFIGS)
def test_live_gallery_equals_support_gallery_through_adds_and_removals(precision, merge_before, single_direct):
    V, Q = _videos(12, 11), _videos(10, 12)
    with torch.no_grad():
        head, live, sup = _pair(precision, merge_before, single_direct, capacity=4)       # grows 4 -> 6 on the way
        assert live.add_classes(V[:6], IDS[:6]) == sup.add_classes(V[:6], IDS[:6]) == [0, 1, 2]
        base = live._store["P"].data_ptr()
        assert live.add_classes(V[6:8], IDS[6:8]) == sup.add_classes(V[6:8], IDS[6:8]) == [3]
        assert live._store["P"].data_ptr() == base and live.capacity == 4                  # no growth: the store did not move
        assert live.add_classes(V[8:], IDS[8:]) == sup.add_classes(V[8:], IDS[8:]) == [4, 5]
        assert live.class_ids == sup.class_ids == [0, 1, 2, 5, 7, 9] and len(live) == 6 and live.capacity == 6
        P, pn = _dense(live)
        assert torch.equal(P, sup._P) and torch.equal(pn, sup._pn)
        assert [live.shots(c) for c in live.class_ids] == [2, 1, 3, 2, 1, 3]
        lg = live.classify(Q)
        assert torch.equal(lg, sup.classify(Q)) and bool(torch.isfinite(lg).all())
        with pytest.raises(ValueError, match="already registered"):
            live.add_classes(V[:1], [0])
        # remove the first, a middle and the last class
        with pytest.raises(ValueError, match="not registered"):
            live.remove_classes([0, 4])
        assert live.class_ids == [0, 1, 2, 5, 7, 9] and live.layout_version == 0
        ptr = live._store["P"].data_ptr()
        live.remove_classes([0, 5, 9])
        assert live.class_ids == [1, 2, 7] and live.layout_version == 1 and live._store["P"].data_ptr() == ptr
        keep = [i for i, c in enumerate(IDS) if c in (1, 2, 7)]
        rest = _pair(precision, merge_before, single_direct)[2]
        rest.add_classes(V[keep], [IDS[i] for i in keep])
        assert torch.equal(live.classify(Q), rest.classify(Q))
        # a class added afterwards takes the lowest freed slot and the last column; nothing of the slot's previous owner is visible
        old_slot = 0                                                                        # class 0 took slot 0
        W = _videos(2, 13)
        assert live.add_classes(W, [11, 11]) == rest.add_classes(W, [11, 11]) == [3]
        assert live.slot_of(11) == old_slot and live.class_ids == [1, 2, 7, 11] and live.shots(11) == 2
        assert torch.equal(live.classify(Q), rest.classify(Q))
        P, pn = _dense(live)
        assert torch.equal(P, rest._P) and torch.equal(pn, rest._pn)


def test_subsets_and_topk_are_columns_of_the_full_result():
    V, Q = _videos(12, 21), _videos(7, 22)
    with torch.no_grad():
        head, live, sup = _pair()
        live.add_classes(V, IDS)
        full = live.classify(Q)
        order = live.class_ids
        for sub in ([9, 0, 5], [7], [2, 9, 1, 0, 7, 5]):
            cols = [order.index(c) for c in sub]
            lg = live.classify(Q, classes=sub)
            assert tuple(lg.shape) == (7, len(sub)) and torch.equal(lg, full[:, cols])
            k = min(2, len(sub))
            vals, idx = live.topk(Q, k=k, classes=sub)
            sv, si = torch.sort(full[:, cols], dim=1, descending=True, stable=True)
            assert torch.equal(vals, sv[:, :k]) and torch.equal(idx.long(), si[:, :k])
        feats = torch.empty(7, T, live.E, device=DEV)
        live._features(live._fresh_engine(), Q, feats)
        assert torch.equal(live.classify_features(feats, classes=[5, 1]), full[:, [order.index(5), order.index(1)]])
        vals, idx = live.topk(Q, k=3)
        sv, si = torch.sort(full, dim=1, descending=True, stable=True)
        assert torch.equal(vals, sv[:, :3]) and torch.equal(idx.long(), si[:, :3])
        for bad, msg in (([0, 4], "not registered"), ([0, 0], "twice"), ([], "at least one")):
            with pytest.raises(ValueError, match=msg):
                live.classify(Q, classes=bad)
        with pytest.raises(ValueError, match="k must be"):
            live.topk(Q, k=3, classes=[0, 1])


@pytest.mark.parametrize("precision,merge_before", [("fp32", False), ("bf16", False), ("fp32", True)])
def test_add_shots_in_pieces_against_one_registration(precision, merge_before):
    """class 3: 1 + 2 + 2 shots against one add_classes of 5 (class 4 goes along with 2 + 1).  'Same clip, another batch': the bound is
    the project's 2e-5 (the fp32 tail picks its GEMM by row count), the argmax is equal on every row, the shot counts are exact.
    The measured difference is printed."""
    V, Q = _videos(8, 31), _videos(12, 32)
    ids = [3, 3, 3, 3, 3, 4, 4, 4]
    with torch.no_grad():
        head, live, _ = _pair(precision, merge_before)
        one = _pair(precision, merge_before)[1]
        one.add_classes(V, ids)
        live.add_classes(V[[0, 5, 6]], [3, 4, 4])
        assert live.add_shots(V[[1, 2]], [3, 3]) == [3]
        assert live.add_shots(V[[7, 3, 4]], [4, 3, 3]) == [3, 5]
        assert live.shots(3) == one.shots(3) == 5 and live.shots(4) == one.shots(4) == 3
        with pytest.raises(ValueError, match="not registered"):
            live.add_shots(V[:1], [17])
        assert live.shots(3) == 5
        a, b = live.classify(Q), one.classify(Q)
    d = maxdiff(a.cpu(), b.cpu())
    print("add_shots 1 + 2 + 2 vs one add_classes of 5, %s merge_before=%d: |dlogits| = %.2e" % (precision, merge_before, d))
    assert d <= BOUND, d
    assert torch.equal(a.argmax(1), b.argmax(1))


def test_state_dict_round_trips():
    V, Q = _videos(12, 41), _videos(5, 42)
    W = _videos(3, 43)
    with torch.no_grad():
        head, live, sup = _pair()
        live.add_classes(V, IDS)
        live.remove_classes([1])
        lg = live.classify(Q)
        sd = live.state_dict()
        assert sd["class_ids"] == [0, 2, 5, 7, 9] and sd["counts"] == [2, 3, 2, 1, 3] and tuple(sd["sums"].shape) == (5, T + 1, live.E)
        other = _pair(capacity=2)[1]
        other.load_state_dict(sd)
        assert other.class_ids == live.class_ids and torch.equal(other.classify(Q), lg)
        assert live.add_shots(W, [7, 2, 7]) == other.add_shots(W, [7, 2, 7]) == [3, 4]       # the sums came along: the same bits go on
        lg2 = live.classify(Q)
        assert torch.equal(other.classify(Q), lg2) and not torch.equal(lg2, lg)
        sup.load_state_dict(sd)                                                            # a SupportGallery takes the dict as it is
        assert sup.class_ids == sd["class_ids"] and torch.equal(sup.classify(Q), lg)
        third = _pair()[1]
        third.load_state_dict(sup.state_dict())                                            # ... and a LiveGallery a SupportGallery's
        assert torch.equal(third.classify(Q), lg) and third.shots(7) == 0
        with pytest.raises(ValueError, match="loaded without its sum"):
            third.add_shots(W[:1], [7])
        assert torch.equal(third.classify(Q), lg)


def test_stream_pool_and_window_stream_over_a_live_gallery():
    from clip_fsar_amd.pool import StreamPool
    from clip_fsar_amd.stream import WindowStream
    V, W = _videos(12, 51), _videos(1, 52)
    with torch.no_grad():
        head, live, sup = _pair()
        live.add_classes(V, IDS)
        sup.add_classes(V, IDS)
        g = torch.Generator().manual_seed(53)
        feats = torch.randn(T + 3, live.E, generator=g).to(DEV)
        pl, ps = StreamPool(live, max_streams=3, max_push=16), StreamPool(sup, max_streams=3, max_push=16)
        a, b = pl.open(), ps.open()
        out_l, out_s = pl.push_features({a: feats})[a], ps.push_features({b: feats})[b]
        assert tuple(out_l.logits.shape) == (4, 6) and torch.equal(out_l.logits, out_s.logits)
        # smoothing on: "remove one, add one" keeps the class count and changes what a column means
        pool = StreamPool(live, max_streams=3, max_push=16, smooth=0.5)
        ws = WindowStream(live, n_streams=1, max_push=16, smooth=0.5)
        h = pool.open()
        pool.push_features({h: feats})
        ws.push_features(feats[None])
        live.remove_classes([2])
        live.add_classes(W, [3])
        assert len(live) == 6
        with pytest.raises(RuntimeError, match=r"reset\(\) the session"):
            pool.push_features({h: feats[:2]})
        with pytest.raises(RuntimeError, match=r"reset\(\) the stream"):
            ws.push_features(feats[None, :2])
        later = pool.open()                                    # a session opened afterwards carries no state: it goes on
        assert pool.push_features({later: feats})[later].smoothed.shape == (4, 6)
        with pytest.raises(RuntimeError, match=r"reset\(\) the session"):
            pool.push_features({h: feats[:2]})                 # ... and the stale one raises until it is reset
        pool.reset(h)
        ws.reset()
        out = pool.push_features({h: feats})[h]
        assert torch.equal(out.logits, live.classify_features(torch.stack([feats[i:i + T] for i in range(4)])))
        assert ws.push_features(feats[None]).smoothed.shape == (1, 4, 6)
        assert pool.push_features({h: feats[:2], later: feats[:1]})[h].smoothed.shape == (2, 6)
