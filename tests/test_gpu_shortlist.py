"""GPU: the shortlist (libclipfsar_shortlist.so, clip_fsar_amd.shortlist.Shortlist) -- the selection kernel bit for bit against
reference_select at every chunk edge, keep, group size and special value; the coarse rows and scores against the float64 references under
the bound tests/test_shortlist_abi.py derives; Shortlist end to end on a small LiveGallery (columns, logits, keep >= C, topk, topk against
the gallery's own), the refresh of coarse rows after further shots, a reused slot and a growth, and chunk independence.

Every output lives inside a larger buffer of sentinels that must be intact afterwards, and every input is compared with its copy.

Measured on an MI355X (run with -s for every figure): see DESIGN.md, section "Shortlist"."""
import itertools

import pytest
import torch

import clip_fsar_amd.synth as synth
from test_gpu_gallery import BOUND, DEV, _head, _restated
from test_shortlist_abi import NONE, bound, rho, row_bound, sequences

pytestmark = pytest.mark.gpu
NAN, INF = float("nan"), float("inf")
PAD = 64                                          # sentinels on each side of an output


def _guarded(shape, dtype, fill):
    """(a contiguous view of `shape` inside a larger buffer of `fill`, check(): the surroundings are intact)"""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * PAD,), fill, device=DEV, dtype=dtype)

    def check():
        assert bool((buf[:PAD] == fill).all()) and bool((buf[PAD + n:] == fill).all()), "a write outside the output"
    return buf[PAD:PAD + n].view(*shape), check


def _bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------ 1: the selection
def _scores(NQ, NC, counts, seed):
    """scores quantised to four values, so that ties at the threshold abound; NaN, +inf, -inf and both zeros sprinkled in; column NC // 2
    NaN and column 0 -inf in every query (two columns no group can select); every fourth group with clips all-equal"""
    g = torch.Generator().manual_seed(seed)
    S = torch.randint(0, 4, (NQ, NC), generator=g).float() * 0.5 - 0.5           # -0.5, 0.0, 0.5, 1.0
    special = torch.tensor([NAN, INF, -INF, -0.0, 0.0])
    where = torch.rand(NQ, NC, generator=g) < 0.06
    S[where] = special[torch.randint(0, 5, (int(where.sum()),), generator=g)]
    q = 0
    for i, n in enumerate(counts):
        if n and i % 4 == 3:
            S[q:q + n] = 0.5
        q += n
    S[:, 0] = -INF
    S[:, NC // 2] = NAN
    return S


def _group_scores(S, counts):
    """[G, NC] float64 group scores, NaN where a column is not selectable -- the rule restated with torch, for the preconditions alone"""
    out, q = [], 0
    for n in counts:
        blk = S[q:q + n].double()
        best = torch.where(blk.isnan(), torch.full_like(blk, -INF), blk).max(0).values if n else torch.full((S.shape[1],), -INF).double()
        out.append(torch.where(best == -INF, torch.full_like(best, NAN), best))
        q += n
    return torch.stack(out)


def _conditions(S, counts, K):
    """(some group has more columns at its threshold than it takes, some group has fewer selectable columns than K)"""
    ties = padding = False
    for row in _group_scores(S, counts):
        ok = row[~row.isnan()]
        if ok.numel() < K:
            padding = True
        elif ok.numel() > K:
            thr = ok.sort(descending=True).values[K - 1]
            ties = ties or int((ok >= thr).sum()) > K
    return ties, padding


def _run_select(S, cols, counts, keep, work_fill):
    from clip_fsar_amd import shortlist_hip as sh
    G, (NQ, NC) = len(counts), S.shape
    K = min(keep, NC)
    sel_cols, check_c = _guarded((G, K), torch.int32, 12345)
    sel_slots, check_s = _guarded((G, K), torch.int32, 54321)
    work, check_w = _guarded((sh.workspace_floats(G, NC),), torch.float32, work_fill)
    s, c = S.to(DEV), cols.to(DEV)
    rows, total = sh.table_rows(counts)
    assert total == NQ
    sh.select(s, c, sh.table_uploader(DEV, max(G, 1)).upload(rows), keep, sel_cols, sel_slots, work)
    torch.cuda.synchronize()
    for check in (check_c, check_s, check_w):
        check()
    assert torch.equal(_bits(s.cpu()), _bits(S)) and torch.equal(c.cpu(), cols), "an input changed"
    return sel_cols.cpu(), sel_slots.cpu()


def _check_select(S, cols, counts, keep, want_ties, want_padding):
    """want_ties, want_padding: what the case claims to be -- asserted first, on the scores alone, before the device is called"""
    from clip_fsar_amd.shortlist import reference_select
    NC = S.shape[1]
    K = min(keep, NC)
    assert _conditions(S, counts, K) == (want_ties, want_padding), (NC, keep, counts[:8])
    ref = torch.tensor(reference_select(S, counts, keep), dtype=torch.int32).view(len(counts), K)
    sel_cols, sel_slots = _run_select(S, cols, counts, keep, 3.0)
    assert torch.equal(sel_cols, ref), (NC, keep, counts[:8])
    slots = torch.where(ref == NONE, torch.full_like(ref, -1), cols[ref.clamp(max=NC - 1).long()])
    assert torch.equal(sel_slots, slots), (NC, keep, counts[:8])
    again = _run_select(S, cols, counts, keep, -1.5)           # another run, other garbage in the workspace: identical bytes
    assert torch.equal(again[0], sel_cols) and torch.equal(again[1], sel_slots)


def _claims(NC, K, counts):
    """(ties, padding) a case of _scores is meant to show.  Columns 0 and NC // 2 have no selectable score in any group, so K >= NC - 1
    pads every group and leaves no tie at a threshold; a group without clips pads at every K.  K <= 2 of at least 61 scored columns pads
    no group with clips, and is meant to cut through equal scores (four values, or several +inf): _case takes the first scores that do."""
    return NC >= 63 and K <= 2, 0 in counts or K > NC - 2


def _case(NC, counts, keeps):
    """the first scores of the seed sequence whose reference conditions are the claimed ones at every keep"""
    for seed in range(NC * 31 + len(counts) + counts[0], NC * 31 + len(counts) + counts[0] + 2000, 100):
        S = _scores(sum(counts), NC, counts, seed)
        if all(_conditions(S, counts, min(k, NC)) == _claims(NC, min(k, NC), counts) for k in keeps):
            return S
    raise AssertionError("no scores with the claimed conditions: NC %d, counts %r" % (NC, counts[:8]))


@pytest.mark.parametrize("NC", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_select_equals_reference_select_bit_for_bit(NC):
    keeps = sorted({k for k in (1, 2, NC - 1, NC, NC + 5) if k >= 1})
    cols = torch.randperm(NC + 7, generator=torch.Generator().manual_seed(NC))[:NC].to(torch.int32)
    many = [(0, 1, 3, 17)[i % 4] for i in range(300)]
    for counts in ([1], [3], [17], [0, 1], many):             # G = 1 at every size (a lone group of 0 clips has no S: it rides with one clip)
        S = _case(NC, counts, keeps)
        for keep in keeps:
            ties, padding = _claims(NC, min(keep, NC), counts)
            assert ties or padding                             # every case shows one of the two
            _check_select(S, cols, counts, keep, ties, padding)


def _stated(groups, K):
    """(ties, padding) of hand-made groups, each stated as the multiplicities of its selectable scores from the largest value down: a
    group pads when it has fewer than K of them, and has a tie at its threshold when it has more and no run of equal scores ends at K"""
    ties = padding = False
    for runs in groups:
        ends = list(itertools.accumulate(runs))
        padding = padding or sum(runs) < K
        ties = ties or (sum(runs) > K and K not in ends)
    return ties, padding


def test_select_special_rows():
    """hand-made rows at a chunk edge (NC = 257): all equal; both zeros alone; NaN everywhere but one column; +inf and -inf; the largest
    and smallest floats; denormals on both sides of zero"""
    NC = 257
    cols = torch.arange(NC, dtype=torch.int32)
    rows = {
        "all equal": torch.full((NC,), 2.5),
        "zeros": torch.tensor([0.0, -0.0] * 128 + [0.0]),
        "one score": torch.full((NC,), NAN).index_fill(0, torch.tensor([256]), -7.0),
        "infinities": torch.tensor([INF, -INF, 1.0] * 85 + [INF, -INF]),
        "extremes": torch.tensor([3.4028234e38, -3.4028234e38, 1e-45, -1e-45, 0.0, -0.0, NAN] * 36 + [1.0] * 5),
        "minus inf": torch.full((NC,), -INF),
    }
    runs = {                                                   # each row's selectable scores, the largest value first: how many are equal
        "all equal": [257],
        "zeros": [257],                                        # -0.0 == +0.0: one run
        "one score": [1],
        "infinities": [86, 85],                                # +inf, 1.0; the 86 -inf are not selectable
        "extremes": [36, 5, 36, 72, 36, 36],                   # max, 1.0, the denormal, both zeros, minus the denormal, -max; 36 NaN
        "minus inf": [],
    }
    for name, row in rows.items():
        S = row.view(1, NC).contiguous()
        for keep in (1, 2, 128, 256, 257):
            _check_select(S, cols, [1], keep, *_stated([runs[name]], keep))
    assert _stated([runs["all equal"]], 100) == (True, False) and _stated([runs["all equal"]], 257) == (False, False)
    assert _stated([runs["one score"]], 2) == _stated([runs["minus inf"]], 1) == (False, True)
    assert _stated([runs["infinities"]], 86) == (False, False) and _stated([runs["infinities"]], 128) == (True, False)
    S = torch.stack([rows["zeros"], rows["one score"], rows["infinities"]])       # a group of three: max over NaN, zeros and infinities
    whole = [[86, 85, 86]]                                     # +inf (c % 3 == 0, and 255), 1.0 (c % 3 == 2), 0.0 (the rest: over -inf, over -7)
    split = [[257], [], [86, 85, 1]]                           # the zeros; no clips; +inf, 1.0 and the -7 (c % 3 == 1 is NaN over -inf: none)
    for keep in (1, 85, 86, 200, 300):
        K = min(keep, NC)
        _check_select(S, cols, [3], keep, *_stated(whole, K))
        assert _stated(split, K)[1]
        _check_select(S, cols, [1, 0, 2], keep, *_stated(split, K))


# ------------------------------------------------------------------ 2: the coarse rows and scores
@pytest.mark.parametrize("T", [1, 8, 32])
@pytest.mark.parametrize("E", [4, 36, 512])
def test_mean_unit_rows_and_coarse_scores_against_float64(T, E):
    from clip_fsar_amd import shortlist_hip as sh
    from clip_fsar_amd.shortlist import reference_coarse, reference_mean_unit_rows
    worst = worst_row = 0.0
    for family, NQ, NC in itertools.product(("gauss", "near", "scale"), (1, 65), (1, 63, 65)):
        cap = NC + 3
        Xq, qn = sequences(family, NQ, T, E, seed=T * 1000 + E + NQ)
        P, pn = sequences(family, cap, T, E, seed=T * 1000 + E + NC + 7)
        assert max(rho(Xq, qn), rho(P, pn)) <= 1.0005
        perm = torch.randperm(cap, generator=torch.Generator().manual_seed(NC))
        used, spare = perm[:NC], perm[NC:]
        xq, qnd, p, pnd = Xq.to(DEV), qn.to(DEV), P.to(DEV), pn.to(DEV)
        # the store's rows: the used slots and two slots outside the store, which write nothing; the spare slots keep their sentinel
        store, check_store = _guarded((cap, E), torch.float32, 7.0)
        stale = torch.cat([used[:NC // 2], torch.tensor([-1, cap]), used[NC // 2:]]).to(torch.int32).to(DEV)
        sh.mean_unit_rows(p, pnd, stale, store)
        U, check_u = _guarded((NQ, E), torch.float32, 7.0)
        sh.mean_unit_rows(xq, qnd, None, U)
        # the scores: two more columns whose slots are outside the store
        cols = torch.cat([used[:NC // 2], torch.tensor([-1]), used[NC // 2:], torch.tensor([cap])]).to(torch.int32)
        S, check_S = _guarded((NQ, NC + 2), torch.float32, 7.0)
        sh.coarse_scores(U, store, cols.to(DEV), S)
        torch.cuda.synchronize()
        for check in (check_store, check_u, check_S):
            check()
        assert bool((store[spare.to(DEV)] == 7.0).all()), "a slot outside the list was written"
        for dev, host in ((xq, Xq), (qnd, qn), (p, P), (pnd, pn)):
            assert torch.equal(dev.cpu(), host), "an input changed"
        # the two kinds of mean rows on their own, element by element under the rounding of one row
        uq, up = reference_mean_unit_rows(Xq, qn), reference_mean_unit_rows(P, pn)
        over_u = (U.cpu().double() - uq).abs() / row_bound(Xq, qn)
        over_p = ((store.cpu().double() - up).abs() / row_bound(P, pn))[used]
        worst_row = max(worst_row, float(over_u.max()), float(over_p.max()))
        assert float(over_u.max()) <= 1.0 and float(over_p.max()) <= 1.0, (family, NQ, NC, float(over_u.max()), float(over_p.max()))
        s = S.cpu()
        bad = [NC // 2, NC + 1]
        good = [j for j in range(NC + 2) if j not in bad]
        assert bool(s[:, bad].isnan().all()) and bool(torch.isfinite(s[:, good]).all())
        ref = reference_coarse(uq, up[cols[good].long()])
        err = float((s[:, good].double() - ref).abs().max())
        worst = max(worst, err / bound(T, E))
        assert err <= bound(T, E), (family, NQ, NC, err, bound(T, E))
    print("coarse scores T %d E %d: worst err / bound %.2f (bound %.2e); a mean row's element: worst err / bound %.2f" % (
        T, E, worst, bound(T, E), worst_row))


# ------------------------------------------------------------------ 3: end to end, on a small LiveGallery
ARCH, T = "ViT-test/16", 8
C, N = 24, 20
COUNTS = [3, 1, 0, 5, 2, 4, 5]                    # 20 clips, 160 rows through context2: one GEMM form at every batch up to 24 clips


class _World:
    pass


@pytest.fixture(scope="module")
def world():
    """24 classes of one shot each in 8 families of 3 (a family shares a picture, a class adds its own to it, a frame adds a little
    noise: the frames of a video look alike, as a real video's do); the clips of a group are the windows of one stream, noisy copies of
    the shot of one class.  Built once, never changed."""
    from clip_fsar_amd.live_gallery import LiveGallery
    w = _World()
    a = synth.ARCHS[ARCH]
    g = torch.Generator().manual_seed(77)
    image = (3, a["res"], a["res"])
    with torch.no_grad():
        w.head = _head(ARCH, "fp32", T)
        w.head.args.TRAIN.MERGE_BEFORE = w.head.args.TRAIN.SINGLE_DIRECT = False
        w.live = LiveGallery(w.head, DEV, capacity=32)
        family = torch.randn(C // 3, 1, *image, generator=g).repeat_interleave(3, 0)
        w.V = (0.5 * (family + 0.5 * torch.randn(C, 1, *image, generator=g) + 0.2 * torch.randn(C, T, *image, generator=g))).to(DEV)
        w.live.add_classes(w.V, list(range(C)))
        w.truth = [(5 * i + 2) % C for i, n in enumerate(COUNTS) for _ in range(n)]
        w.Q = (w.V[torch.tensor(w.truth, device=DEV)] + 0.05 * torch.randn(N, T, *image, generator=g).to(DEV)).contiguous()
        w.feats = torch.empty(N, T, w.live.E, device=DEV)
        w.live._features(w.live._fresh_engine(), w.Q, w.feats)
        torch.cuda.synchronize()
    return w


def _groups(counts):
    q = 0
    for i, n in enumerate(counts):
        yield i, q, n
        q += n


@pytest.mark.parametrize("classes", [None, [7, 0, 15, 3, 10, 22, 5, 19, 1, 20]])
def test_columns_and_logits_of_a_call(world, classes):
    from clip_fsar_amd.shortlist import Shortlist, reference_select
    live = world.live
    ids = live.class_ids if classes is None else classes
    with torch.no_grad():
        sl = Shortlist(live, keep=6)
        before = world.feats.clone()
        r = sl.classify_features(world.feats, counts=COUNTS, classes=classes)
        S = sl.coarse_features(world.feats, classes=classes)
        torch.cuda.synchronize()
        assert r.keep == 6 and tuple(r.logits.shape) == (N, 6) and tuple(r.columns.shape) == (len(COUNTS), 6) and r.counts == COUNTS
        assert tuple(S.shape) == (N, len(ids)) and torch.equal(world.feats, before)
        want = reference_select(S.cpu(), COUNTS, 6)
        assert r.columns.cpu().tolist() == want
        assert r.class_ids() == [[ids[c] if c != NONE else None for c in row] for row in want]
        assert want[2] == [NONE] * 6                                                # the group without clips
        for i, q, n in _groups(COUNTS):
            if n:
                exact = live.classify_features(world.feats[q:q + n], classes=[ids[c] for c in want[i]])
                assert torch.equal(r.logits[q:q + n], exact), i                     # bit for bit
        rp = sl.classify(world.Q, counts=COUNTS, classes=classes)                   # from pixels: the same features, the same bits
        assert torch.equal(rp.logits, r.logits) and torch.equal(rp.columns, r.columns)


def test_keep_at_least_c_gives_the_bits_of_plain_classify_features(world):
    from clip_fsar_amd.shortlist import Shortlist
    with torch.no_grad():
        full = world.live.classify_features(world.feats)
        for keep in (C, 64):
            r = Shortlist(world.live, keep=keep).classify_features(world.feats)     # counts None: every clip its own group
            assert r.keep == C and torch.equal(r.logits, full)
            assert r.columns.cpu().tolist() == [list(range(C))] * N
        r = Shortlist(world.live, keep=C).classify_features(world.feats, counts=COUNTS)
        assert torch.equal(r.logits, full)


def _topk_of(logits, columns, counts, k):
    """top-k over a result's logits (the stable descending sort), mapped to class indices through the group's columns"""
    sv, si = torch.sort(logits, dim=1, descending=True, stable=True)
    group = torch.repeat_interleave(torch.arange(len(counts)), torch.tensor(counts)).to(logits.device)
    return sv[:, :k], columns[group].gather(1, si[:, :k]).to(torch.int32)


def test_topk_is_topk_over_the_logits_mapped_to_class_indices(world):
    from clip_fsar_amd.shortlist import Shortlist
    with torch.no_grad():
        for classes, counts in ((None, COUNTS), ([7, 0, 15, 3, 10, 22, 5, 19, 1, 20], COUNTS), (None, None)):
            sl = Shortlist(world.live, keep=6)
            r = sl.classify_features(world.feats, counts=counts, classes=classes)
            for k in (1, 3, 6):
                values, index = sl.topk_features(world.feats, k=k, counts=counts, classes=classes)
                wv, wi = _topk_of(r.logits, r.columns, r.counts, k)
                assert torch.equal(values, wv) and torch.equal(index, wi) and index.dtype == torch.int32, (classes, k)
            pv, pi = sl.topk(world.Q, k=3, counts=counts, classes=classes)
            wv, wi = _topk_of(r.logits, r.columns, r.counts, 3)
            assert torch.equal(pv, wv) and torch.equal(pi, wi)


def test_topk_equals_the_gallerys_own_where_the_reference_says_it_must(world):
    """Precondition, on the float64 references alone (the device's context2 rows and prototypes are their inputs): every clip's full-OTAM
    top-k lies inside its group's reference shortlist, and neither ranking has a gap at its cut that fp32 could close -- 2 x the bound of
    the coarse scores at the shortlist's threshold, 2 x the project's 2e-5 at the k-th logit.  Then the shortlist loses nothing."""
    from clip_fsar_amd.shortlist import Shortlist, reference_coarse, reference_mean_unit_rows, reference_select
    live, k, keep = world.live, 3, 8
    with torch.no_grad():
        sl = Shortlist(live, keep=keep)
        Xq, qn = sl._queries(live._fresh_engine(), world.feats, False)
        idx = torch.tensor([live.slot_of(c) for c in live.class_ids], device=DEV)
        P, pn = live._store["P"][idx].cpu(), live._store["pn"].view(-1, T)[idx].reshape(-1).cpu()
        xq, qn = Xq.cpu(), qn.cpu()
    full, _ = _restated(xq, P, False)
    coarse = reference_coarse(reference_mean_unit_rows(xq, qn), reference_mean_unit_rows(P, pn))
    lists = reference_select(coarse, COUNTS, keep)
    scores = _group_scores(coarse, COUNTS)
    worst_rank, coarse_gap, logit_gap = 0, INF, INF
    for i, q, n in _groups(COUNTS):
        if not n:
            continue
        ranked = scores[i].sort(descending=True).values
        coarse_gap = min(coarse_gap, float(ranked[keep - 1] - ranked[keep]))
        order = scores[i].argsort(descending=True).tolist()
        for clip in range(q, q + n):
            sv, si = full[clip].sort(descending=True)
            logit_gap = min(logit_gap, float(sv[k - 1] - sv[k]))
            worst_rank = max(worst_rank, max(order.index(c) for c in si[:k].tolist()))
    print("full-OTAM top-%d against the reference shortlist of %d of %d classes: worst coarse rank %d (0 = best), smallest gap at the "
          "shortlist's cut %.2e, at the k-th logit %.2e" % (k, keep, C, worst_rank, coarse_gap, logit_gap))
    assert worst_rank < keep and coarse_gap > 2 * bound(T, live.E) and logit_gap > 2 * BOUND
    for i, q, n in _groups(COUNTS):
        for clip in range(q, q + n):
            assert set(full[clip].sort(descending=True).indices[:k].tolist()) <= set(lists[i]), (clip, lists[i])
    with torch.no_grad():
        values, index = sl.topk(world.Q, k=k, counts=COUNTS)
        gv, gi = live.topk(world.Q, k=k)
        assert torch.equal(values, gv) and torch.equal(index, gi)
        assert sl.classify(world.Q, counts=COUNTS).columns.cpu().tolist() == lists


def test_nothing_crosses_between_host_and_device_once_a_call_launches(world, monkeypatch):
    """A tensor made on the host reaches the device by a copy that waits for the stream, and so does one brought back.  From its first
    launch (the first of _queries) to its return a call makes neither: no torch.tensor(.., device=), no .to / .cuda of a host tensor, no
    .cpu / .tolist / .item of a device tensor and no torch.cuda.synchronize -- with stale coarse rows to refresh, for classify as for
    topk.  (The group tables go up through the pinned uploaders, by copy_(.., non_blocking=True).)"""
    from clip_fsar_amd.live_gallery import LiveGallery
    from clip_fsar_amd.shortlist import Shortlist
    E = world.live.E
    g = torch.Generator().manual_seed(9)
    f = lambda n: torch.randn(n, T, E, generator=g).to(DEV)
    with torch.no_grad():
        live = LiveGallery(world.head, DEV, capacity=8)
        live.add_classes_features(f(7), list(range(7)))
        sl = Shortlist(live, keep=3)
        Q, more = f(6), f(1)
        quiet = sl.topk_features(Q, k=2, counts=[2, 0, 4])                        # the answer, from an unwatched Shortlist's call
        sl = Shortlist(live, keep=3)
        state, seen = {"launched": False}, []
        queries, tensor, to, cuda = sl._queries, torch.tensor, torch.Tensor.to, torch.Tensor.cuda

        def watched_queries(*a):
            state["launched"] = True
            return queries(*a)

        def watched_tensor(*a, **kw):
            if state["launched"] and torch.device(kw.get("device") or "cpu").type != "cpu":
                seen.append("torch.tensor(.., device=)")
            return tensor(*a, **kw)

        def up(name, orig):
            def watched(self, *a, **kw):
                out = orig(self, *a, **kw)
                if state["launched"] and not self.is_cuda and out.is_cuda:
                    seen.append(name)
                return out
            return watched

        def down(name):
            orig = getattr(torch.Tensor, name)

            def watched(self, *a, **kw):
                if state["launched"] and self.is_cuda:
                    seen.append(name)
                return orig(self, *a, **kw)
            return watched

        monkeypatch.setattr(sl, "_queries", watched_queries)
        monkeypatch.setattr(torch, "tensor", watched_tensor)
        monkeypatch.setattr(torch.Tensor, "to", up(".to", to))
        monkeypatch.setattr(torch.Tensor, "cuda", up(".cuda", cuda))
        for name in ("cpu", "tolist", "item"):
            monkeypatch.setattr(torch.Tensor, name, down(name))
        monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **kw: seen.append("torch.cuda.synchronize"))

        def call(fn, *a, **kw):
            out = fn(*a, **kw)
            state["launched"] = False
            return out

        values, index = call(sl.topk_features, Q, k=2, counts=[2, 0, 4])          # all 7 coarse rows are stale
        assert seen == [] and sl.stats == {"calls": 1, "refreshed": 7}
        live.add_shots_features(more, [4])
        assert seen == []                                                         # the gallery's call is not watched: nothing launched
        call(sl.topk_features, Q, k=2, counts=[2, 0, 4], classes=[6, 4, 0, 2])    # one stale row, another list
        r = call(sl.classify_features, Q, counts=[6])
        call(sl.coarse_features, Q)
        assert seen == [] and sl.stats == {"calls": 3, "refreshed": 8}
        state["launched"] = True                                                  # the watch itself: it sees each kind of crossing
        torch.tensor([1], device=DEV).tolist()
        torch.zeros(1).to(DEV).cpu()
        assert seen == ["torch.tensor(.., device=)", "tolist", ".to", "cpu"]
        monkeypatch.undo()
        assert r.class_ids()[0] == sorted(r.class_ids()[0]) and len(r.class_ids()[0]) == 3        # the one sync, after the call
        assert torch.equal(values, quiet[0]) and torch.equal(index, quiet[1])


def test_a_group_straddling_a_chunk_boundary_gives_the_same_bits(world, monkeypatch):
    from clip_fsar_amd.shortlist import Shortlist
    with torch.no_grad():
        sl = Shortlist(world.live, keep=6)
        r = sl.classify_features(world.feats, counts=COUNTS)
        eng = world.live._fresh_engine()
        for clips in (3, 7):                                                        # chunks of 3 and of 7 clips cut the groups of 5
            monkeypatch.setattr(eng, "max_frames", clips * T)
            rc = sl.classify_features(world.feats, counts=COUNTS)
            # from pixels the tower runs chunk by chunk too, and its features are its own business ("same clip, another batch"): the
            # call is held to what it gives, unchunked, on the features the tower computes in these chunks
            cv, ci = sl.topk(world.Q, k=2, counts=COUNTS)
            feats = torch.empty_like(world.feats)
            world.live._features(eng, world.Q, feats)
            monkeypatch.undo()
            assert torch.equal(rc.logits, r.logits) and torch.equal(rc.columns, r.columns), clips
            tv, ti = sl.topk_features(feats, k=2, counts=COUNTS)
            assert torch.equal(cv, tv) and torch.equal(ci, ti), clips


# ------------------------------------------------------------------ 4: the refresh of coarse rows
def test_coarse_rows_follow_the_gallery(world):
    """after further shots of a class, a class in a freed slot and a growth past capacity the coarse rows in use equal a from-scratch
    recomputation, and stats counts the touched slots alone"""
    from clip_fsar_amd import shortlist_hip as sh
    from clip_fsar_amd.live_gallery import LiveGallery
    from clip_fsar_amd.shortlist import Shortlist, reference_select
    E = world.live.E
    g = torch.Generator().manual_seed(5)
    f = lambda n: torch.randn(n, T, E, generator=g).to(DEV)
    with torch.no_grad():
        live = LiveGallery(world.head, DEV, capacity=8)
        live.add_classes_features(f(8), [0, 1, 2, 3, 4, 5, 5, 6])                   # 7 classes, slots 0 .. 6 of 8
        sl = Shortlist(live, keep=3)
        Q = f(6)

        def check(refreshed):
            r = sl.classify_features(Q, counts=[2, 4])
            S = sl.coarse_features(Q)
            assert sl.stats["refreshed"] == refreshed
            slots = torch.tensor([live.slot_of(c) for c in live.class_ids], device=DEV)
            scratch = torch.full((live.capacity, E), 7.0, device=DEV)
            sh.mean_unit_rows(live._store["P"], live._store["pn"], None, scratch)
            assert sl._coarse.shape == scratch.shape and torch.equal(sl._coarse[slots], scratch[slots])
            assert r.columns.cpu().tolist() == reference_select(S.cpu(), [2, 4], 3)
            for i, q, n in _groups([2, 4]):
                ids = [live.class_ids[c] for c in r.columns[i].tolist()]
                assert torch.equal(r.logits[q:q + n], live.classify_features(Q[q:q + n], classes=ids))

        check(7)
        check(7)                                                                    # nothing moved: nothing is recomputed
        assert live.add_shots_features(f(2), [2, 2]) == [3]
        check(8)
        slot = live.slot_of(3)
        live.remove_classes([3])
        live.add_classes_features(f(1), [11])
        assert live.slot_of(11) == slot
        check(9)
        live.add_classes_features(f(3), [12, 13, 14])                               # 10 classes: past the capacity of 8
        assert live.capacity > 8
        check(12)
        sub = Shortlist(live, keep=2)                                               # candidates alone are refreshed
        sub.classify_features(Q, classes=[13, 0, 5])
        assert sub.stats == {"calls": 1, "refreshed": 3}
