"""GPU: the live text gallery (clip_fsar_amd.live_text_gallery.LiveTextGallery on libclipfsar_live_text.so) -- the grouped text kernels
group by group against the dense kernels of libclipfsar_gallery_text.so on the gathered store (bit for bit) and against the float64
restatement; the gallery against a fresh TextGallery after adds, removals and further shots, against ClipFsarEngine.forward and the
reference's goldens on an episode among distractors, grouped against single calls, under a StreamPool with class lists and enrolment,
top-k and state dicts in both directions."""
import random

import pytest
import torch

import clip_fsar_amd.synth as synth
from _cases import load_golden, maxdiff
from test_gpu_gallery_text import BOUND, DEV, SCALE, _episode, _head, _restated
from test_gpu_groups import LISTS, MAX_PUSH, RATE, STRIDE, _schedule
from test_gpu_pool import _ticks
from test_gpu_stream import _frames, _materialised, _n_windows

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0
PAD = 37
NAN = float("nan")


# ------------------------------------------------------------------ 1: the kernels, through the binding
class _Problem:
    """counts[g] queries against lists[g] (slots of a store of cap rows; None: drawn, overlapping between groups).  Every slot that no
    list names is NaN in text_store and in tn_store: a stray read shows as a NaN somewhere."""

    def __init__(self, counts, widths, cap, E, seed, lists=None, antipodal=None):
        from clip_fsar_amd import gallery_hip as gh
        from clip_fsar_amd import live_text_hip as lt
        rng = random.Random(seed)
        g = torch.Generator().manual_seed(seed)
        self.counts, self.cap, self.E = counts, cap, E
        self.lists = lists if lists is not None else [rng.sample(range(cap), w) for w in widths]
        self.rows, (self.NQ, self.NCOLS, self.tiles, self.n_out, self.n_part) = lt.table_rows(counts, [len(l) for l in self.lists])
        base = torch.randn(E, generator=g)
        NQ = max(self.NQ, 1)
        self.emb = ((base + 1.5 * torch.randn(NQ, E, generator=g)) * (0.3 + 3 * torch.rand(NQ, 1, generator=g))).float().to(DEV)   # spread norms
        named = sorted({s for l in self.lists for s in l if 0 <= s < cap})
        rows = ((base + 1.5 * torch.randn(len(named), E, generator=g)) * (0.3 + 3 * torch.rand(len(named), 1, generator=g))).float().to(DEV)
        self.text = torch.full((cap, E), NAN, device=DEV)
        self.tn = torch.full((cap,), NAN, device=DEV)
        idx = torch.tensor(named, device=DEV)
        norms = torch.empty(len(named), device=DEV)
        self.en = torch.empty(NQ, device=DEV)
        if antipodal is not None:                           # (slot a, slot b, query): the query's own row and its negative, cos = +-1
            a, b, q = antipodal
            rows[named.index(a)], rows[named.index(b)] = self.emb[q], -self.emb[q]
        gh.row_norms(rows, norms)
        gh.row_norms(self.emb, self.en)
        self.text[idx], self.tn[idx] = rows, norms
        self.vis = -(4.0 + 8.0 * torch.rand(self.n_out, generator=g)).to(DEV)             # OTAM logits = -cum
        self.cols = torch.tensor([s for l in self.lists for s in l], device=DEV, dtype=torch.int32)
        self.table = lt.table_uploader(DEV, len(self.rows)).upload(self.rows)
        assert lt.workspace_floats(self.table) == 2 * self.n_part

    def grouped(self, scale, coff):
        """-> (logits, EVAL_TEXT probabilities, COMBINE output), flat [n_out]; the sentinels behind every buffer are checked"""
        from clip_fsar_amd import live_text_hip as lt
        buf = lambda n: torch.full((n + PAD,), SENTINEL, device=DEV)
        lg, probs, comb, part = buf(self.n_out), buf(self.n_out), buf(self.n_out), buf(2 * self.n_part)
        sc = torch.tensor([scale], device=DEV)
        lt.text_logits_grouped(self.emb, self.en, self.text, self.tn, self.cols, sc, lg, part, self.table, self.n_out, self.n_part)
        lt.text_softmax_grouped(lg, part, probs, self.table, self.NQ, self.n_out, self.n_part)
        lt.text_combine_grouped(lg, part, self.vis, comb, self.table, self.NQ, self.n_out, self.n_part, coff)
        inplace = lg.clone()
        lt.text_softmax_grouped(inplace, part, inplace, self.table, self.NQ, self.n_out, self.n_part)      # out may alias logits
        torch.cuda.synchronize()
        for b, n in ((lg, self.n_out), (probs, self.n_out), (comb, self.n_out), (part, 2 * self.n_part), (inplace, self.n_out)):
            assert bool((b[n:] == SENTINEL).all()), "a write behind the buffer"
        assert not bool((part[:2 * self.n_part] == SENTINEL).any())                        # every partial was written
        assert _same(inplace[:self.n_out], probs[:self.n_out])
        return lg[:self.n_out], probs[:self.n_out], comb[:self.n_out]

    def dense(self, g, scale, coff, nan_at=()):
        """group g through the dense kernels on text_store[its list] (rows nan_at of it NaN) -> (logits, probs, combine) [n, w], the
        float64 restatement's (probs, combine), or None for a group without queries"""
        from clip_fsar_amd import gallery_text_hip as gt
        q0, n, c0, w, _, out0 = self.rows[g][:6]
        if n == 0:
            return None
        cols = self.cols[c0:c0 + w].long().clamp(0, self.cap - 1)
        text, tn = self.text[cols].contiguous(), self.tn[cols].contiguous()
        for j in nan_at:
            text[j], tn[j] = NAN, NAN
        emb, en = self.emb[q0:q0 + n], self.en[q0:q0 + n]
        vis = self.vis[out0:out0 + n * w].view(n, w).clone()                               # a dense matrix of its own: rows at i * w
        part = torch.empty(gt.workspace_floats(n, w), device=DEV)
        lg, probs, comb = (torch.empty(n, w, device=DEV) for _ in range(3))
        gt.text_logits(emb, en, text, tn, torch.tensor([scale], device=DEV), lg, part)
        gt.text_softmax(lg, part, probs)
        gt.text_combine(lg, part, vis, comb, coff)
        _, ref_p = _restated(emb.cpu(), text.cpu(), scale)
        _, ref_c = _restated(emb.cpu(), text.cpu(), scale, vis.cpu(), coff)
        return lg, probs, comb, ref_p, ref_c

    def block(self, flat, g):
        q0, n, c0, w, _, out0 = self.rows[g][:6]
        return flat[out0:out0 + n * w].view(n, w)


def _same(a, b):
    """torch.equal with NaN equal to NaN"""
    return a.shape == b.shape and bool(((a == b) | (a.isnan() & b.isnan())).all())


def _check(p, scale=SCALE, coff=0.9, what=""):
    """every group: logits and EVAL_TEXT probabilities torch.equal to the dense kernels; COMBINE torch.equal when every NC is a multiple
    of 4 (row_pass4 splits the visual row alike), <= BOUND against float64 otherwise; probabilities <= BOUND against float64"""
    lg, probs, comb = p.grouped(scale, coff)
    assert bool(torch.isfinite(lg).all() and torch.isfinite(probs).all() and torch.isfinite(comb).all())
    aligned = all(len(l) % 4 == 0 for l in p.lists)
    e_p = e_c = e_sum = 0.0
    for g in range(len(p.rows)):
        ref = p.dense(g, scale, coff)
        if ref is None:
            continue
        d_lg, d_p, d_c, ref_p, ref_c = ref
        torch.cuda.synchronize()
        assert torch.equal(p.block(lg, g), d_lg), (what, g, "logits")
        assert torch.equal(p.block(probs, g), d_p), (what, g, "probs")
        if aligned:
            assert torch.equal(p.block(comb, g), d_c), (what, g, "combine")
        e_p = max(e_p, float((p.block(probs, g).cpu().double() - ref_p).abs().max()))
        e_c = max(e_c, float((p.block(comb, g).cpu().double() - ref_c).abs().max()))
        e_sum = max(e_sum, float((p.block(probs, g).cpu().double().sum(1) - 1).abs().max()))
    print("%s scale %g coff %.1f: %d groups, %d tiles: |dprobs| %.2e |dcombine| %.2e |row sum - 1| %.2e vs float64%s" % (
        what, scale, coff, len(p.rows), p.tiles, e_p, e_c, e_sum, " (combine bit-equal)" if aligned else ""))
    assert e_p <= BOUND and e_c <= BOUND and e_sum <= 1e-5, (e_p, e_c, e_sum)
    return probs


@pytest.mark.parametrize("E", [4, 36, 512])
def test_grouped_kernels_equal_the_dense_kernels_at_the_tile_edges(E):
    """groups of 1, 64, 65, 0 and 129 queries against overlapping lists of 1, 64, 65, 3 and 130 of 160 slots; groups without queries
    first, in the middle and last; E: a K loop of one partial chunk, a partial last chunk, the workload's"""
    _check(_Problem([0, 1, 64, 65, 0, 129, 0], [5, 1, 64, 65, 3, 130, 2], 160, E, seed=E), what="edges E=%d" % E)


def test_combine_is_bit_equal_where_every_list_is_a_multiple_of_four():
    _check(_Problem([3, 65, 2, 1], [4, 64, 68, 132], 160, 36, seed=5), coff=0.5, what="NC % 4 == 0")


def test_merge_of_more_partials_than_threads():
    """one query against 16 385 slots: 257 partials, past the 256-thread stride of merge_partials"""
    p = _Problem([1], [16385], 16400, 36, seed=9)
    assert p.n_part == 257 and p.tiles == 257
    _check(p, what="257 partials")


def test_three_hundred_random_groups():
    rng = random.Random(300)
    counts = [rng.randint(0, 9) for _ in range(300)]
    widths = [rng.randint(1, 70) for _ in range(300)]
    _check(_Problem(counts, widths, 200, 64, seed=300), what="300 random groups")


@pytest.mark.parametrize("scale", [1.0, 100.0])
@pytest.mark.parametrize("coff", [0.9, 0.5])
def test_scale_and_coff(scale, coff):
    rng = random.Random(17)
    lists = [rng.sample(range(160), 7), rng.sample(range(160), 9), list(range(131))]
    p = _Problem([5, 0, 70], None, 160, 64, seed=17, lists=lists, antipodal=(3, 100, 74))    # the last query's row and its negative
    probs = _check(p, scale=scale, coff=coff, what="scale / coff")
    if scale == 100.0:
        assert float(p.block(probs, 2)[69, 100]) == 0.0                                     # expf(-200): the probability underflows


@pytest.mark.parametrize("bad", [-1, 160])
def test_a_slot_out_of_range_poisons_its_column_in_its_group_alone(bad):
    cap = 160
    rng = random.Random(bad)
    widths = [9, 70, 3, 65]
    lists = [rng.sample(range(cap), w) for w in widths]
    at = 66                                                                                 # in the second class tile of group 1
    lists[1][at] = bad
    p = _Problem([4, 66, 0, 3], widths, cap, 36, seed=3, lists=lists)
    lg, probs, comb = p.grouped(SCALE, 0.9)
    for g in (0, 1, 3):
        d_lg, d_p, d_c, _, _ = p.dense(g, SCALE, 0.9, nan_at=(at,) if g == 1 else ())
        torch.cuda.synchronize()
        assert _same(p.block(lg, g), d_lg) and _same(p.block(probs, g), d_p), g
        if g == 1:
            assert bool(p.block(lg, g)[:, at].isnan().all()) and bool(torch.isfinite(p.block(lg, g)[:, :at]).all())
            assert float((p.block(comb, g).cpu().double().nan_to_num() - d_c.cpu().double().nan_to_num()).abs().max()) <= BOUND
            assert bool((p.block(comb, g).isnan() == d_c.isnan()).all())
        else:                                                                               # nothing outside the store was read
            assert torch.equal(p.block(lg, g), d_lg) and bool(torch.isfinite(p.block(probs, g)).all() and torch.isfinite(p.block(comb, g)).all())


# ------------------------------------------------------------------ 2: the gallery
ARCH, T = "ViT-test/16", 8
IDS = [0, 0, 1, 2, 2, 2, 5, 5, 7, 9, 9, 9]
#          precision  mode        merge_before single_direct coff
CONFIGS = [("fp32", "eval_text", False, False, None), ("bf16", "eval_text", False, False, None),
           ("fp32", "combine", False, False, None), ("bf16", "combine", True, False, 0.5),
           ("fp32", "combine", False, True, None), ("fp32", "combine", True, False, 0.5)]


def _galleries(precision, mode, merge_before=False, single_direct=False, coff=None, capacity=4, head=None):
    """(head, a LiveTextGallery, a maker of fresh TextGalleries)"""
    from clip_fsar_amd.live_text_gallery import LiveTextGallery
    from clip_fsar_amd.text_gallery import TextGallery
    head = head if head is not None else _head(ARCH, precision, T)
    head.args.TRAIN.MERGE_BEFORE, head.args.TRAIN.SINGLE_DIRECT, head.args.TRAIN.TEXT_COFF = merge_before, single_direct, coff
    return head, LiveTextGallery(head, DEV, mode=mode, capacity=capacity), lambda: TextGallery(head, DEV, mode=mode)


def _videos(n, seed):
    a = synth.ARCHS[ARCH]
    return (torch.randn(n, T, 3, a["res"], a["res"], generator=torch.Generator().manual_seed(seed)) * 0.5).to(DEV)


def _features(g, videos):
    feats = torch.empty(videos.shape[0], T, g.E, device=DEV)
    g._features(g._fresh_engine(), videos, feats)
    return feats


def _fresh_with(fresh, V, ids, order):
    """a fresh TextGallery holding the classes `order`, in that order, registered from their videos of (V, ids) in the videos' order"""
    pick = [i for c in order for i, v in enumerate(ids) if v == c]
    t = fresh()
    t.add_classes(V[pick], [ids[i] for i in pick])
    assert t.class_ids == list(order)
    return t


def _sub_state(sd, order):
    """the state dict of the classes `order` of sd, in that order"""
    at = [sd["class_ids"].index(c) for c in order]
    i = torch.tensor(at)
    has_p = sd["prototypes"].shape[0] > 0
    return {"fingerprint": sd["fingerprint"], "class_ids": list(order), "text": sd["text"][i], "text_norms": sd["text_norms"][i],
            "prototypes": sd["prototypes"][i] if has_p else sd["prototypes"],
            "norms": sd["norms"].view(-1, T)[i].reshape(-1) if has_p else sd["norms"]}


@pytest.mark.parametrize("precision,mode,merge_before,single_direct,coff", CONFIGS)
def test_live_text_gallery_equals_a_fresh_text_gallery(precision, mode, merge_before, single_direct, coff):
    """adds, removals, a reused slot, growth: classify is a fresh TextGallery's with the same classes registered from the same videos,
    bit for bit, and classify(classes=L) a fresh TextGallery's holding exactly L.  After further shots (COMBINE) the prototypes are
    LiveGallery's -- against one registration of all shots 'the same clip in another batch', the project's 2e-5 -- so there the fresh
    TextGallery holds the same classes through the state dict, and the single registration is held to 2e-5 with equal argmax."""
    V, W, Q = _videos(12, 11), _videos(4, 13), _videos(10, 12)
    with torch.no_grad():
        head, live, fresh = _galleries(precision, mode, merge_before, single_direct, coff)
        assert live.add_classes(V[:6], IDS[:6]) == [0, 1, 2]
        live.remove_classes([1])
        assert live.add_classes(V[6:], IDS[6:]) == [2, 3, 4] and live.class_ids == [0, 2, 5, 7, 9] and live.capacity == 6
        assert live.slot_of(5) == 1                                                         # the freed slot
        if mode == "eval_text":
            assert live.add_text_classes([3, "kite"], text={"kite": torch.randn(live.E, generator=torch.Generator().manual_seed(1))}) == [5, 6]
            live.remove_classes([3, "kite"])
            assert set(live._store) == {"text", "tn"} and [live.shots(c) for c in live.class_ids] == [0] * 5
        else:
            assert [live.shots(c) for c in live.class_ids] == [2, 3, 2, 1, 3]
        live.remove_classes([0, 9])
        assert live.add_classes(W[:2], [11, 11]) == [3] and live.class_ids == [2, 5, 7, 11] and live.layout_version >= 2
        allV, all_ids = torch.cat([V, W[:2]]), IDS + [11, 11]
        out = live.classify(Q)
        assert tuple(out.shape) == (10, 4) and bool(torch.isfinite(out).all())
        assert torch.equal(out, _fresh_with(fresh, allV, all_ids, live.class_ids).classify(Q))
        feats = _features(live, Q)
        assert torch.equal(live.classify_features(feats), out)
        for L in ([11, 2], [7], [5, 11, 7, 2]):
            sub = live.classify(Q, classes=L)
            assert tuple(sub.shape) == (10, len(L)) and torch.equal(sub, _fresh_with(fresh, allV, all_ids, L).classify(Q)), L
            if mode == "eval_text":
                assert float((sub.double().sum(1) - 1).abs().max().cpu()) <= 1e-5          # the softmax ran over the list
        if mode == "eval_text":
            with pytest.raises(ValueError, match="takes no shots"):
                live.add_shots(W[2:], [2, 7])
            return
        assert live.add_shots(W[2:], [7, 2]) == [2, 4]
        out2 = live.classify(Q)
        sd = live.state_dict()
        t = fresh()
        t.load_state_dict(sd)
        assert not torch.equal(out2, out) and torch.equal(out2, t.classify(Q))
        for L in ([7, 2], [11, 7, 5]):
            t.load_state_dict(_sub_state(sd, L))
            assert torch.equal(live.classify(Q, classes=L), t.classify(Q)), L
        moreV, more_ids = torch.cat([allV, W[2:]]), all_ids + [7, 2]
        one = _fresh_with(fresh, moreV, more_ids, live.class_ids).classify(Q)
        d = maxdiff(out2.cpu(), one.cpu())
        print("%s %s mb=%d sd=%d coff=%s: further shots vs one registration of all shots: %.2e" % (precision, mode, merge_before,
                                                                                                 single_direct, coff, d))
        assert d <= BOUND and torch.equal(out2.argmax(1), one.argmax(1))


@pytest.mark.parametrize("precision,mode,merge_before,single_direct,coff", CONFIGS)
def test_an_episode_among_distractors_equals_the_engine(precision, mode, merge_before, single_direct, coff):
    """12 classes registered, classify(classes=the episode's 5) against ClipFsarEngine.forward(mode=...) on the episode"""
    with torch.no_grad():
        head, live, _ = _galleries(precision, mode, merge_before, single_direct, coff)
        d, same = _episode_check(head, live, _episode(ARCH, 5, 2, T, episode=4, q=2), 5, mode, merge_before, single_direct, n_test=24)[:2]
    print("%s %s mb=%d sd=%d coff=%s: |classify(classes=episode) - engine| = %.2e" % (precision, mode, merge_before, single_direct, coff, d))
    assert d <= BOUND and same, d


def _episode_check(head, live, ep, way, mode, merge_before, single_direct, n_test):
    """distractors before, between and after the episode's classes, one of them removed again -> (|gallery - engine|, equal argmax,
    the gallery's output in the episode's column order)"""
    eng = head._get_engine(DEV)
    res = synth.ARCHS[ARCH]["res"]
    Tn = live.T
    S = ep["support_set"].shape[0] // Tn
    lg_ep, _ = eng.forward(ep["support_set"], ep["target_set"], ep["support_labels"], ep["real_support_labels"], way=way, T=Tn,
                           merge_before=merge_before, single_direct=single_direct, mode=mode, text_coff=live.text_coff)
    vids = ep["support_set"].reshape(S, Tn, *ep["support_set"].shape[1:])
    real = [int(v) for v in ep["real_support_labels"].cpu()]
    others = [c for c in range(n_test) if c not in real][:8]
    D = (torch.randn(8, Tn, 3, res, res, generator=torch.Generator().manual_seed(77)) * 0.5).to(DEV)
    live.add_classes(D[:3], others[:3])
    first = [s for s in range(S) if real[s] in sorted(set(real))[:2]]
    rest = [s for s in range(S) if s not in first]
    live.add_classes(vids[first], [real[s] for s in first])
    live.add_classes(D[3:6], others[3:6])
    live.add_classes(vids[rest], [real[s] for s in rest])
    live.add_classes(D[6:], others[6:])
    live.remove_classes([others[1]])
    assert len(live) == 12
    sl = [float(v) for v in ep["support_labels"].cpu()]
    ranks = {v: i for i, v in enumerate(sorted(set(sl)))}
    col_of = {real[s]: ranks[sl[s]] for s in range(S)}
    order = sorted(col_of, key=lambda c: col_of[c])                                        # the episode's classes in its column order
    Qn = ep["target_set"].shape[0] // Tn
    lg = live.classify(ep["target_set"].reshape(Qn, Tn, *ep["target_set"].shape[1:]), classes=order)
    torch.cuda.synchronize()
    a, b = lg.cpu(), lg_ep[0].cpu()
    return maxdiff(a, b), torch.equal(a.argmax(1), b.argmax(1)), a


@pytest.mark.parametrize("case", ["n4_evaltext_5w2s_T4", "n4_combine_5w1s_T8", "n4_combine_5w3s_T4_mb_c05"])
def test_an_episode_among_distractors_against_reference_goldens(case):
    from clip_fsar_amd.live_text_gallery import LiveTextGallery
    g = load_golden(case)
    m = g["meta"]
    assert m["arch"] == ARCH
    head = _head(m["arch"], "fp32", m["T"], scale=m["scale"], n_train=m["n_train"], n_test=m["n_test"], seed=m["seed"])
    ep = synth.make_episode(m["way"], m["shot"], m["q"], m["T"], synth.ARCHS[ARCH]["res"], m["n_test"], m["episode"], m["seed"])
    ep = {k: torch.from_numpy(v).to(DEV) for k, v in ep.items()}
    mb = m.get("merge_before", False)
    head.args.TRAIN.MERGE_BEFORE, head.args.TRAIN.SINGLE_DIRECT, head.args.TRAIN.TEXT_COFF = mb, False, m.get("text_coff")
    with torch.no_grad():
        live = LiveTextGallery(head, DEV, mode=m["mode"], capacity=4)
        d_ep, _, out = _episode_check(head, live, ep, m["way"], m["mode"], mb, False, m["n_test"])
    d_ref = maxdiff(out, torch.from_numpy(g["logits"]))
    print("%s: |classify(classes=episode) - reference| = %.2e, - engine = %.2e" % (case, d_ref, d_ep))
    assert d_ref < 1e-4, d_ref
    assert d_ep <= BOUND


GROUP_COUNTS = [3, 0, 4, 1, 2]
GROUP_LISTS = [[9, 0, 5], [7], None, [2, 9, 1, 0, 7, 5], [5, 1]]


@pytest.mark.parametrize("precision,mode,merge_before,single_direct,coff", CONFIGS[:4])
def test_grouped_equals_single_calls_group_by_group(precision, mode, merge_before, single_direct, coff, monkeypatch):
    V, Q = _videos(12, 21), _videos(sum(GROUP_COUNTS), 22)
    with torch.no_grad():
        head, live, _ = _galleries(precision, mode, merge_before, single_direct, coff)
        live.add_classes(V, IDS)
        feats = _features(live, Q)
        r = live.classify_features_grouped(feats, GROUP_COUNTS, GROUP_LISTS)
        rp = live.classify_grouped(Q, GROUP_COUNTS, GROUP_LISTS)
        eng = live._fresh_engine()
        monkeypatch.setattr(eng, "max_frames", 3 * T)                                       # chunks of 3 clips cut the groups
        rc = live.classify_features_grouped(feats, GROUP_COUNTS, GROUP_LISTS)
        monkeypatch.undo()
        assert len(r) == 5 and r.counts == GROUP_COUNTS and r.widths == [3, 1, 6, 6, 2] and r.logits.shape[0] == r.offsets[-1] == 43
        worst = worst_px = worst_chunk = 0.0
        q = 0
        for i, (n, L) in enumerate(zip(GROUP_COUNTS, GROUP_LISTS)):
            if n == 0:
                assert r.group(i).shape == (0, 1)
                continue
            ref = live.classify_features(feats[q:q + n], classes=L)
            ref_px = live.classify(Q[q:q + n], classes=L)
            if mode == "eval_text":
                assert torch.equal(r.group(i), ref) and torch.equal(rc.group(i), ref), i
            worst = max(worst, maxdiff(r.group(i).cpu(), ref.cpu()))
            worst_chunk = max(worst_chunk, maxdiff(rc.group(i).cpu(), ref.cpu()))
            worst_px = max(worst_px, maxdiff(rp.group(i).cpu(), ref_px.cpu()))
            assert torch.equal(r.group(i).argmax(1), ref.argmax(1)) and torch.equal(rp.group(i).argmax(1), ref_px.argmax(1)), i
            q += n
    print("%s %s mb=%d coff=%s: grouped vs single calls: features %.2e, in chunks of 3 %.2e, pixels %.2e" % (
        precision, mode, merge_before, coff, worst, worst_chunk, worst_px))
    assert worst <= BOUND and worst_chunk <= BOUND and worst_px <= 2e-5


def test_topk_and_topk_grouped_agree_with_torch():
    V, Q = _videos(12, 31), _videos(sum(GROUP_COUNTS), 32)
    with torch.no_grad():
        for mode in ("eval_text", "combine"):
            head, live, _ = _galleries("fp32", mode)
            live.add_classes(V, IDS)
            for classes, k in ((None, 4), ([9, 0, 5], 2), ([7], 1)):
                probs = live.classify(Q, classes=classes)
                vals, idx = live.topk(Q, k=k, classes=classes)
                sv, si = torch.sort(probs, dim=1, descending=True, stable=True)            # ties to the lower index
                assert torch.equal(vals, sv[:, :k]) and torch.equal(idx.long(), si[:, :k]), (mode, classes)
            counts, lists = [3, 0, 4, 3], [[9, 0, 5], [7], None, [5, 1]]
            r = live.classify_grouped(Q, counts, lists)
            vals, idx = live.topk_grouped(Q, counts, lists, k=2)
            q = 0
            for i, n in enumerate(counts):
                if n == 0:
                    continue
                sv, si = torch.sort(r.group(i), dim=1, descending=True, stable=True)
                assert torch.equal(vals[q:q + n], sv[:, :2]) and torch.equal(idx[q:q + n].long(), si[:, :2]), (mode, i)
                q += n
            with pytest.raises(ValueError, match="k must be"):
                live.topk_grouped(Q, counts, lists, k=3)


@pytest.mark.parametrize("mode", ["eval_text", "combine"])
def test_state_dict_round_trips_with_text_gallery(mode):
    V, Q = _videos(12, 41), _videos(5, 42)
    with torch.no_grad():
        head, live, fresh = _galleries("fp32", mode, coff=0.5)
        live.add_classes(V, IDS)
        live.remove_classes([1])
        out = live.classify(Q)
        sd = live.state_dict()
        assert sd["class_ids"] == [0, 2, 5, 7, 9] and sd["counts"] == ([2, 3, 2, 1, 3] if mode == "combine" else [0] * 5)
        t = fresh()
        t.load_state_dict(sd)                                                               # LiveTextGallery -> TextGallery
        assert t.class_ids == live.class_ids and torch.equal(t.classify(Q), out)
        other = _galleries("fp32", mode, coff=0.5, capacity=2)[1]
        other.load_state_dict(t.state_dict())                                               # TextGallery -> LiveTextGallery
        assert other.class_ids == live.class_ids and torch.equal(other.classify(Q), out) and other.shots(7) == 0
        assert torch.equal(other.classify(Q, classes=[9, 2]), live.classify(Q, classes=[9, 2]))
        third = _galleries("fp32", mode, coff=0.5)[1]
        third.load_state_dict(sd)                                                           # and its own
        assert torch.equal(third.classify(Q), out)
        if mode == "combine":
            W = _videos(2, 43)
            assert live.add_shots(W, [7, 2]) == third.add_shots(W, [7, 2]) == [2, 4]       # the sums came along: the same bits go on
            assert torch.equal(third.classify(Q), live.classify(Q))
            with pytest.raises(ValueError, match="loaded without its sum"):
                other.add_shots(W[:1], [7])


# ------------------------------------------------------------------ 3: under a stream pool
def test_pool_with_class_lists_over_a_combine_gallery():
    """The four-session schedule of the pool's contract test over a COMBINE gallery, two sessions with lists and one without (and the
    reused slot's new owner with another): every session's logits against classify_features of its materialised windows with its list"""
    from clip_fsar_amd.pool import StreamPool
    with torch.no_grad():
        head, live, _ = _galleries("fp32", "combine", capacity=8)
        live.add_classes(_videos(12, 71), IDS)
        span = (T - 1) * RATE + 1
        ticks = _ticks(span, STRIDE)
        need = {}
        for _, tick in ticks:
            for name, n in tick.items():
                need[name] = need.get(name, 0) + n
        eng = live._fresh_engine()
        feats = {}
        for i, (name, n) in enumerate(sorted(need.items())):
            fr = _frames(ARCH, 1, n, seed=300 + i)[0]
            feats[name] = torch.empty(n, live.E, device=DEV)
            eng.vit.forward(fr.contiguous(), feats[name])
        call = lambda pool, arg: pool.push_features(arg)
        plain = StreamPool(live, max_streams=3, stride=STRIDE, rate=RATE, max_push=MAX_PUSH)
        base, hb = _schedule(plain, ticks, feats, call, dict.fromkeys(LISTS))
        pool = StreamPool(live, max_streams=3, stride=STRIDE, rate=RATE, max_push=MAX_PUSH)
        outs, h = _schedule(pool, ticks, feats, call, LISTS)
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
            ref = live.classify_features(_materialised(feats[name][None, f0:f0 + n], T, STRIDE, RATE, nW), classes=LISTS[name])
            got = torch.cat([o.logits for o in pieces])
            worst = max(worst, maxdiff(got.cpu(), ref.cpu()))
            assert torch.equal(got.argmax(1), ref.argmax(1)), key
            windows += nW
        print("combine: |pool with lists - classify_features(classes=)| = %.2e over %d windows" % (worst, windows))
        assert worst <= 2e-5 and windows > 20, (worst, windows)
        for name in h:
            assert pool.stats(h[name]) == plain.stats(hb[name]), name


def _bits(sd):
    return {k: v for k, v in sd.items() if isinstance(v, torch.Tensor)}


def test_enrolment_and_the_smoothing_guard_over_a_combine_gallery():
    from clip_fsar_amd.pool import StreamPool
    with torch.no_grad():
        head, live, _ = _galleries("fp32", "combine")
        live.add_classes(_videos(12, 81), IDS)
        twin = _galleries("fp32", "combine")[1]
        twin.load_state_dict(live.state_dict())                                             # the sums come along
        eng = live._fresh_engine()
        n = T + 5
        feats = torch.empty(n, live.E, device=DEV)
        eng.vit.forward(_frames(ARCH, 1, n, seed=82)[0].contiguous(), feats)
        pool = StreamPool(live, max_streams=2, max_push=16)
        h = pool.open(classes=[9, 2])
        pool.push_features({h: feats})
        real_forward = eng.vit.forward

        def no_tower(*a, **kw):
            raise AssertionError("the tower ran")

        eng.vit.forward = no_tower
        try:
            assert pool.enroll(h, 2) == 4                                                   # the newest window: frames 5 .. 12
            assert pool.enroll(h, 17, window=1, join=True) == 1 and pool._sessions[h].classes == [9, 2, 17]
            assert twin.add_shots_features(feats[5:5 + T][None].contiguous(), [2]) == [4]   # the windows materialised by indexing
            assert twin.add_classes_features(feats[1:1 + T][None].contiguous(), [17]) == [6]
        finally:
            eng.vit.forward = real_forward
        a, b = live.state_dict(), twin.state_dict()
        assert a["class_ids"] == b["class_ids"] and a["counts"] == b["counts"]
        for k, v in _bits(a).items():                       # the sums of context2's outputs stop at its T frame rows: row T is never written
            assert torch.equal(v[:, :T], b[k][:, :T]) if k == "sums" else torch.equal(v, b[k]), k
        out = pool.push_features({h: feats[:3]})[h]
        assert out.logits.shape[1] == 3
        # smoothing: "remove one, add one" keeps the class count and changes what a column means
        smooth = StreamPool(live, max_streams=2, max_push=16, smooth=0.5)
        s = smooth.open()
        assert smooth.push_features({s: feats})[s].smoothed.shape == (6, 7)
        live.remove_classes([5])
        live.add_classes(_videos(1, 83), [3])
        assert len(live) == 7
        with pytest.raises(RuntimeError, match=r"reset\(\) the session"):
            smooth.push_features({s: feats[:2]})
        smooth.reset(s)
        assert smooth.push_features({s: feats})[s].smoothed.shape == (6, 7)
        # EVAL_TEXT: a further shot is refused before any launch, a new class is its text row
        etext = _galleries("fp32", "eval_text")[1]
        etext.add_text_classes([0, 1, 2])
        epool = StreamPool(etext, max_streams=2, max_push=16)
        e = epool.open()
        assert epool.push_features({e: feats})[e].logits.shape == (6, 3)
        with pytest.raises(ValueError, match="takes no shots"):
            epool.enroll(e, 1)
        assert epool.enroll(e, 5) == 0 and etext.class_ids == [0, 1, 2, 5] and epool._enroll_tables is None
        assert epool.push_features({e: feats[:1]})[e].logits.shape == (1, 4)
