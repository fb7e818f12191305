"""GPU: the OTAM alignment (libclipfsar_align.so, clip_fsar_amd.align.Aligner, StreamPool.explain) -- the kernel through the C ABI
against reference_alignment in float64 at every T, lambda, E, family and direction count of the case list, with pairs permuted, repeated
and outside the inputs; its logits against the exact scoring kernel; Aligner on a small LiveGallery (flat and ragged class lists, k=,
a reused slot, a growth); StreamPool.explain on a ring that has wrapped, and a session left untouched by it.

The reference is float64 throughout, on D computed in float64 from the same fp32 rows and the same fp32 norms the kernel is given.
Bounds: dists within e_d and logits within tol, both of tests/test_gpu_otam.py; plan within 4 x the worst |float32 restatement - float64
reference| over this file's own case list -- computed on the host from reference_alignment(dtype=float32), never from the kernel.  The 4
covers the device's expf / logf (a few ulp where the host's are nearly exact) and the one rounding more that D carries.

Every output lives inside a larger buffer of sentinels that must be intact afterwards, and every input is compared with its copy.

Measured on an MI355X (run with -s for every figure): see DESIGN.md, section "Alignment"."""
import functools

import pytest
import torch

import clip_fsar_amd.synth as synth
from test_align_abi import ALL_T, FAMILIES, dists_of, norms_of, rows_of
from test_gpu_gallery import DEV, _head
from test_gpu_otam import e_d_of, tol_of

pytestmark = pytest.mark.gpu
NAN = float("nan")
PAD = 64                                          # sentinels on each side of an output: 256 bytes, so views stay 16-byte aligned
NQ, CAP = 5, 7
ES = [4, 36, 512]
CASES = [(T, 0.5) for T in ALL_T] + [(T, lam) for T in (8, 32) for lam in (0.25, 1.0)]
MARGIN = 4.0


def _guarded(shape, fill, dtype=torch.float32):
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


# ------------------------------------------------------------------ 1: the kernel through the C ABI
@functools.lru_cache(maxsize=None)
def _inputs(family, T, E):
    """(Xq [NQ, T, E], qn, P [CAP, T, E], pn) on the host: fp32 rows and the fp32 norms the kernel is given"""
    Xq, P = rows_of(family, NQ, CAP, T, E, 7919 * FAMILIES.index(family) + 101 * T + E)
    return Xq, norms_of(Xq), P, norms_of(P)


@functools.lru_cache(maxsize=None)
def _reference(family, T, lam):
    """{E: D [NQ, CAP, T, T]}, and per direction count (value, plan) [len(ES), NQ, CAP, ...] in float64, and the float32 restatement's
    worst |difference| to them in plan -- one pass of the T * T host steps serves every E.  Computed once, never changed."""
    from clip_fsar_amd.align import _forward_backward
    D = torch.stack([dists_of(*_inputs(family, T, E)) for E in ES])
    d = D.reshape(-1, T, T)
    out, worst = {}, 0.0
    for dtype in (torch.float64, torch.float32):
        x = d.to(dtype)
        f0, g0 = _forward_backward(x, lam)
        f1, g1 = _forward_backward(x.transpose(1, 2).contiguous(), lam)
        both, single = (f0 + f1, g0 + g1.transpose(1, 2)), (f0, g0)
        if dtype == torch.float64:
            out = {0: both, 1: single, "c_dir": torch.maximum(f0.abs(), f1.abs())}
        else:
            assert bool(torch.isfinite(both[1]).all()) and bool(torch.isfinite(both[0]).all()), (family, T, lam)
            worst = max(float((both[1].double() - out[0][1]).abs().max()), float((single[1].double() - out[1][1]).abs().max()))
    shape = (len(ES), NQ, CAP)
    res = {sd: (v.reshape(shape), p.reshape(*shape, T, T)) for sd, (v, p) in ((0, out[0]), (1, out[1]))}
    return {"D": D, "c_dir": out["c_dir"].reshape(shape), "ref": res, "f32_err": worst}


@pytest.fixture(scope="module")
def plan_bound():
    """MARGIN x the worst float32-restatement error in plan over the whole case list, every family included"""
    worst = max(_reference(f, T, lam)["f32_err"] for f in FAMILIES for T, lam in CASES)
    print("plan: the float32 restatement's worst |difference| to float64 over the case list %.3e, bound %.3e" % (worst, MARGIN * worst))
    assert 0.0 < worst < 5e-5
    return MARGIN * worst


def _pairs(NP, seed):
    """NP pairs over NQ x CAP: every pair at least once (NP >= 35), permuted, repeats, and pair_q in {-1, NQ}, pair_slot in {-1, CAP}
    sprinkled in -> (pair_q, pair_slot) int32 on the host"""
    g = torch.Generator().manual_seed(seed)
    every = torch.arange(NQ * CAP)
    flat = torch.cat([every, torch.randint(0, NQ * CAP, (NP - NQ * CAP,), generator=g)])[torch.randperm(NP, generator=g)]
    pq, ps = (flat // CAP).to(torch.int32), (flat % CAP).to(torch.int32)
    bad = torch.randperm(NP, generator=g)[:24]
    pq[bad[:6]], pq[bad[6:12]] = -1, NQ
    ps[bad[12:18]], ps[bad[18:24]] = -1, CAP
    pq[bad[0]], ps[bad[0]] = NQ, -1                                               # both at once
    return pq, ps


def _run(inputs, pq, ps, lam, sd, with_dists=True):
    """one cfal_align call on guarded outputs -> (plan, dists or None, logits) on the host"""
    from clip_fsar_amd import align_hip as ah
    dev = [t.to(DEV) for t in inputs]
    q, s = pq.to(DEV), ps.to(DEV)
    NP, T = pq.shape[0], inputs[0].shape[1]
    plan, check_p = _guarded((NP, T, T), 7.0)
    dists, check_d = _guarded((NP, T, T), 5.0) if with_dists else (None, lambda: None)
    logits, check_l = _guarded((NP,), 3.0)
    ah.align(*dev, q, s, lam, sd, plan, dists, logits)
    torch.cuda.synchronize()
    for check in (check_p, check_d, check_l):
        check()
    for got, want in zip(dev + [q, s], list(inputs) + [pq, ps]):
        assert torch.equal(_bits(got.cpu()), _bits(want)), "an input changed"
    return plan.cpu(), None if dists is None else dists.cpu(), logits.cpu()


@pytest.mark.parametrize("family", FAMILIES)
def test_the_kernel_against_reference_alignment(family, plan_bound):
    worst = {"plan": 0.0, "dists": 0.0, "logits": 0.0}
    pq, ps = _pairs(300, 11 + FAMILIES.index(family))
    ok = (pq >= 0) & (pq < NQ) & (ps >= 0) & (ps < CAP)
    assert int(ok.sum()) == 300 - 24 and len(set(zip(pq[ok].tolist(), ps[ok].tolist()))) == NQ * CAP
    qi, si = pq[ok].long(), ps[ok].long()
    for T, lam in CASES:
        ref = _reference(family, T, lam)
        for ei, E in enumerate(ES):
            inputs = _inputs(family, T, E)
            for sd in (0, 1):
                what = "%s T %d lambda %g E %d single_direct %d" % (family, T, lam, E, sd)
                plan, dists, logits = _run(inputs, pq, ps, lam, sd)
                assert bool(plan[~ok].isnan().all()) and bool(dists[~ok].isnan().all()) and bool(logits[~ok].isnan().all()), what
                value, want = ref["ref"][sd]
                err_p = float((plan[ok].double() - want[ei][qi, si]).abs().max())
                err_d = float((dists[ok].double() - ref["D"][ei][qi, si]).abs().max())
                c_dir = value.abs() if sd else ref["c_dir"]                        # the larger per-direction cost of the pair
                tol = tol_of(T, E, lam, 1 if sd else 2, c_dir[ei][qi, si])
                ratio_l = float(((logits[ok].double() + value[ei][qi, si]).abs() / tol).max())
                print("%s: plan err %.3e (bound %.3e), dists err %.3e (e_d %.3e), logits err / tol %.3f" % (
                    what, err_p, plan_bound, err_d, e_d_of(E), ratio_l))
                worst = {"plan": max(worst["plan"], err_p / plan_bound), "dists": max(worst["dists"], err_d / e_d_of(E)),
                         "logits": max(worst["logits"], ratio_l)}
                assert bool(torch.isfinite(plan[ok]).all()) and bool(torch.isfinite(logits[ok]).all()), what   # T 32, lambda 0.25 included
                assert err_d <= e_d_of(E), what
                assert ratio_l <= 1.0, what
                assert err_p <= plan_bound, what
                assert float(plan[ok].min()) >= 0.0 and float(plan[ok].max()) <= (1.0 if sd else 2.0) + plan_bound, what
                # a pair that appears twice carries the same bytes, wherever it stands
                first = {}
                for i, key in enumerate(zip(pq.tolist(), ps.tolist())):
                    j = first.setdefault(key, i)
                    if j != i and ok[i]:
                        assert torch.equal(_bits(plan[i]), _bits(plan[j])) and torch.equal(_bits(logits[i]), _bits(logits[j])), what
                # a second run, dists NULL: identical bytes
                again = _run(inputs, pq, ps, lam, sd, with_dists=False)
                assert again[1] is None and torch.equal(_bits(again[0]), _bits(plan)) and torch.equal(_bits(again[2]), _bits(logits)), what
                # NP = 1: the pair's bytes of the large call, with and without dists
                i = int(ok.nonzero()[T % 7])
                for with_dists in (True, False):
                    one = _run(inputs, pq[i:i + 1], ps[i:i + 1], lam, sd, with_dists=with_dists)
                    assert torch.equal(_bits(one[0][0]), _bits(plan[i])) and torch.equal(_bits(one[2][0]), _bits(logits[i])), what
                    assert one[1] is None or torch.equal(_bits(one[1][0]), _bits(dists[i])), what
    print("%s: worst plan err / bound %.3f, dists err / e_d %.3f, logits err / tol %.3f" % (
        family, worst["plan"], worst["dists"], worst["logits"]))


def test_a_call_of_bad_pairs_alone_dereferences_nothing():
    """NQ = cap = 1 with one-row inputs: every pair is outside them, and every output NaN"""
    inputs = _inputs("gauss", 3, 4)
    tiny = (inputs[0][:1], inputs[1][:3], inputs[2][:1], inputs[3][:3])
    pq = torch.tensor([-1, 1, 0, 0, 1 << 30, -(1 << 31)], dtype=torch.int32)
    ps = torch.tensor([0, 0, -1, 1, 0, 1 << 30], dtype=torch.int32)
    plan, dists, logits = _run(tiny, pq, ps, 0.5, 0)
    assert bool(plan.isnan().all()) and bool(dists.isnan().all()) and bool(logits.isnan().all())


# ------------------------------------------------------------------ 2, 3: on the 24-class gallery of tests/test_gpu_shortlist.py
ARCH, T = "ViT-test/16", 8
C, N = 24, 20


class _World:
    pass


@pytest.fixture(scope="module")
def world():
    """test_gpu_shortlist.py's world, rebuilt: 24 classes of one shot each in 8 families of 3, and 20 clips, noisy copies of shots"""
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
        w.truth = [(5 * i + 2) % C for i in range(N)]
        w.Q = (w.V[torch.tensor(w.truth, device=DEV)] + 0.05 * torch.randn(N, T, *image, generator=g).to(DEV)).contiguous()
        w.feats = torch.empty(N, T, w.live.E, device=DEV)
        w.live._features(w.live._fresh_engine(), w.Q, w.feats)
        torch.cuda.synchronize()
    return w


def _by_abi(live, al, feats, pair_q, ids):
    """cfal_align on the gallery's store for the pairs (pair_q[i], class ids[i]) -> (plan, dists, logits)"""
    from clip_fsar_amd import align_hip as ah
    from clip_fsar_amd.gallery import LAMBDA
    Xq, qn = al._queries(live._fresh_engine(), feats, False)
    q = torch.tensor(pair_q, device=DEV, dtype=torch.int32)
    s = torch.tensor([live.slot_of(c) for c in ids], device=DEV, dtype=torch.int32)
    NP, t = len(pair_q), live.T
    plan, dists, logits = (torch.empty(NP, t, t, device=DEV), torch.empty(NP, t, t, device=DEV), torch.empty(NP, device=DEV))
    ah.align(Xq, qn, live._store["P"], live._store["pn"], q, s, LAMBDA, live.single_direct, plan, dists, logits)
    return plan, dists, logits


def _equal(a, want):
    return all(torch.equal(_bits(x), _bits(y)) for x, y in zip((a.plan, a.dists, a.logits), want))


def test_logits_against_the_exact_kernel(world):
    from clip_fsar_amd.align import Aligner, _forward_backward
    from clip_fsar_amd.gallery import LAMBDA
    live = world.live
    classes = [7, 0, 15, 3, 10, 22, 5, 19, 1, 20]
    with torch.no_grad():
        a = Aligner(live).align_features(world.feats, classes=classes)
        exact = live.classify_features(world.feats, classes=classes)
        torch.cuda.synchronize()
    assert tuple(a.logits.shape) == (N * len(classes),) and a.offsets == [i * len(classes) for i in range(N + 1)]
    assert a.pairs.cpu().tolist() == [[i, j] for i in range(N) for j in range(len(classes))]
    d = a.dists.cpu().double()
    c_dir = torch.maximum(_forward_backward(d, LAMBDA)[0].abs(), _forward_backward(d.transpose(1, 2).contiguous(), LAMBDA)[0].abs())
    tol = 2 * tol_of(T, live.E, LAMBDA, 2, c_dir)                                  # the sum of the two kernels' tol
    ratio = float(((a.logits.cpu().double() - exact.reshape(-1).cpu().double()).abs() / tol).max())
    print("align logits against cfsl_otam_indexed: worst err / (sum of the two tol) %.3f" % ratio)
    assert ratio <= 1.0
    assert a.class_ids() == [classes] * N
    assert tuple(a.frame_cost.shape) == tuple(a.frame_match.shape) == (len(a), T)
    assert bool((a.frame_match >= 0).all()) and bool((a.frame_match <= T - 1).all())
    # the value is the plan-weighted cost plus an entropy term that is never positive: <plan, D> >= F(D) + F(D^T) = -logit
    assert bool((a.frame_cost.sum(-1) >= -a.logits - 1e-4).all())


def test_aligner_equals_the_c_abi_bit_for_bit(world):
    from clip_fsar_amd.align import NONE, Aligner
    live = world.live
    with torch.no_grad():
        al = Aligner(live)
        before = world.feats.clone()
        flat = [9, 2, 23]
        a = al.align_features(world.feats, classes=flat)
        assert _equal(a, _by_abi(live, al, world.feats, [i for i in range(N) for _ in flat], flat * N))
        lists = [[(3 * i + j) % C for j in range(i % 4)] for i in range(N)]          # ragged: clips 0, 4, 8, .. have an empty list
        r = al.align_features(world.feats, classes=lists)
        pair_q = [i for i, l in enumerate(lists) for _ in l]
        assert _equal(r, _by_abi(live, al, world.feats, pair_q, [c for l in lists for c in l]))
        assert r.class_ids() == lists and r.offsets[:6] == [0, 0, 1, 3, 6, 6]
        assert r.pairs.cpu().tolist() == [[i, j] for i, l in enumerate(lists) for j in range(len(l))]
        px = al.align(world.Q, classes=flat)                                         # from pixels: the same features, the same bits
        assert _equal(px, (a.plan, a.dists, a.logits))
        # k = 3: the explicit call with the ids topk gives
        k = 3
        t = al.align_features(world.feats, k=k)
        values, index = live.topk(world.Q, k=k)
        ids = [[live.class_ids[c] for c in row] for row in index.cpu().tolist()]
        assert t.class_ids() == ids and t.offsets == [i * k for i in range(N + 1)]
        assert t.pairs.cpu().tolist() == [[i, c] for i, row in enumerate(index.cpu().tolist()) for c in row]
        assert all(c != NONE for row in index.cpu().tolist() for c in row)
        explicit = al.align_features(world.feats, classes=ids)
        assert _equal(t, (explicit.plan, explicit.dists, explicit.logits))
        assert torch.equal(world.feats, before)
        one = al.align_features(world.feats[:1], k=1)                                # the best class of clip 0 is its own
        assert one.class_ids() == [[world.truth[0]]]


def test_nothing_crosses_between_host_and_device_once_a_call_launches(world, monkeypatch):
    """tests/test_gpu_shortlist.py's watch, on Aligner: from its first launch (the first of _queries) to its return a k= call makes no
    torch.tensor(.., device=), no .to / .cuda of a host tensor, no .cpu / .tolist / .item of a device tensor and no synchronize -- the
    slot list is made on the device from the top-k index.  Neither does a call with class lists, whose lists go up before."""
    from clip_fsar_amd.align import Aligner
    live = world.live
    with torch.no_grad():
        quiet = Aligner(live).align_features(world.feats, k=3)
        al = Aligner(live)
        state, seen = {"launched": False}, []
        queries, tensor, to, cuda = al._queries, torch.tensor, torch.Tensor.to, torch.Tensor.cuda

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

        monkeypatch.setattr(al, "_queries", watched_queries)
        monkeypatch.setattr(torch, "tensor", watched_tensor)
        monkeypatch.setattr(torch.Tensor, "to", up(".to", to))
        monkeypatch.setattr(torch.Tensor, "cuda", up(".cuda", cuda))
        for name in ("cpu", "tolist", "item"):
            monkeypatch.setattr(torch.Tensor, name, down(name))
        monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **kw: seen.append("torch.cuda.synchronize"))

        def call(fn, *a, **kw):
            out = fn(*a, **kw)
            assert state["launched"]
            state["launched"] = False
            return out

        t = call(al.align_features, world.feats, k=3)
        call(al.align_features, world.feats, classes=[4, 8])
        call(al.align_features, world.feats[:3], classes=[[1], [], [5, 6]])
        assert seen == []
        state["launched"] = True                                                  # the watch itself: it sees each kind of crossing
        torch.tensor([1], device=DEV).tolist()
        torch.zeros(1).to(DEV).cpu()
        assert seen == ["torch.tensor(.., device=)", "tolist", ".to", "cpu"]
        monkeypatch.undo()
        assert _equal(t, (quiet.plan, quiet.dists, quiet.logits)) and t.class_ids() == quiet.class_ids()      # the one sync, after the call


def test_pairs_follow_the_ids_through_a_reused_slot_and_a_growth(world):
    from clip_fsar_amd.align import Aligner
    from clip_fsar_amd.live_gallery import LiveGallery
    E = world.live.E
    g = torch.Generator().manual_seed(5)
    f = lambda n: torch.randn(n, T, E, generator=g).to(DEV)
    with torch.no_grad():
        live = LiveGallery(world.head, DEV, capacity=8)
        live.add_classes_features(f(7), list(range(7)))
        al = Aligner(live)
        Q, v = f(3), f(1)

        def check(classes):
            a = al.align_features(Q, classes=classes)
            assert _equal(a, _by_abi(live, al, Q, [i for i in range(3) for _ in classes], classes * 3)) and a.class_ids() == [classes] * 3
            return a

        old = check([3, 5])
        slot = live.slot_of(3)
        live.remove_classes([3])
        with pytest.raises(ValueError, match="class 3 is not registered"):
            al.align_features(Q, classes=[3, 5])
        live.add_classes_features(v, [11])
        assert live.slot_of(11) == slot
        new = check([11, 5])
        alone = LiveGallery(world.head, DEV, capacity=2)                              # class 11's prototype, wherever it lives
        alone.add_classes_features(v, [11])
        want = Aligner(alone).align_features(Q, classes=[11])
        assert torch.equal(_bits(new.plan[0::2]), _bits(want.plan)) and torch.equal(_bits(new.logits[0::2]), _bits(want.logits))
        assert torch.equal(_bits(new.plan[1::2]), _bits(old.plan[1::2])) and not torch.equal(_bits(new.plan[0::2]), _bits(old.plan[0::2]))
        live.add_classes_features(f(3), [12, 13, 14])                                 # 10 classes: past the capacity of 8
        assert live.capacity > 8
        grown = check([14, 11, 5, 0])
        assert torch.equal(_bits(grown.plan[1::4]), _bits(new.plan[0::2])) and torch.equal(_bits(grown.plan[2::4]), _bits(new.plan[1::2]))
        top = al.align_features(Q, k=10)                                              # k = every class: no place is empty
        assert sorted(top.class_ids()[0]) == sorted(live.class_ids)


# ------------------------------------------------------------------ 4: StreamPool.explain
STRIDE, RATE, MAX_PUSH = 2, 2, 8                  # a window spans 15 frames, the ring holds 14 + 8 = 22
PUSHES = [5, 8, 3, 8, 7, 8, 1, 6, 8, 2, 8]        # 64 frames: the ring wraps nearly three times


def _window(frames, w):
    """[1, T, E]: window w of a session whose frames so far are `frames`"""
    return frames[torch.tensor([w * STRIDE + j * RATE for j in range(T)], device=DEV)].unsqueeze(0).contiguous()


def test_explain_is_align_features_of_the_window_alone(world):
    from clip_fsar_amd.align import Aligner
    from clip_fsar_amd.pool import StreamPool
    live = world.live
    rows = world.feats.reshape(N * T, -1)
    with torch.no_grad():
        p = StreamPool(live, max_streams=3, stride=STRIDE, rate=RATE, max_push=MAX_PUSH)
        assert p.cap == 22
        other, h = p.open(), p.open()                                                 # the session under test is not in slot 0
        al = Aligner(live)
        t, checked, wrapped = 0, 0, False
        for i, n in enumerate(PUSHES):
            p.push_features({h: rows[t:t + n].contiguous(), other: rows[100:100 + (i % 3)].contiguous()} if i % 3 else
                            {h: rows[t:t + n].contiguous()})
            t += n
            ok = p.enrolable(h)
            if not len(ok):
                with pytest.raises(ValueError, match="is not enrolable"):
                    p.explain(h, k=2)
                continue
            wrapped = wrapped or t > p.cap
            for w, kw in ((None, {"k": 3}), (ok[0], {"classes": [17, 2, 8]}), (ok[-1], {"classes": [[4]]})):
                a = p.explain(h, window=w, **kw)
                want = al.align_features(_window(rows[:t], ok[-1] if w is None else w), **kw)
                assert _equal(a, (want.plan, want.dists, want.logits)) and a.class_ids() == want.class_ids(), (i, w)
                assert a.offsets == want.offsets and torch.equal(a.pairs, want.pairs) and len(a.offsets) == 2
                checked += 1
            for w in (ok[0] - 1, ok[-1] + 1):
                with pytest.raises(ValueError, match="window %d is not enrolable" % w):
                    p.explain(h, [2], window=w)
        assert wrapped and checked >= 24 and t == sum(PUSHES) > 2 * p.cap


def test_explain_changes_nothing_of_the_session(world):
    """two pools of one recipe -- per-class smoothing, a baseline, a rule and a shortlist -- fed the same frames; one is asked to
    explain between its pushes (and refused once): its next pushes give the bits the other's give, and so do its events"""
    from clip_fsar_amd.baseline import Baseline
    from clip_fsar_amd.events import EventRule
    from clip_fsar_amd.pool import StreamPool
    from clip_fsar_amd.shortlist import Shortlist
    live = world.live
    rows = world.feats.reshape(N * T, -1)
    with torch.no_grad():
        def pool():
            return StreamPool(live, max_streams=3, stride=STRIDE, rate=RATE, max_push=MAX_PUSH, smooth=0.5, smooth_by="class",
                              events=EventRule(on=0.5, off=-0.5, min_on=1, min_off=1),
                              baseline=Baseline(rate=0.25, warm_rate=0.5, warmup=2, gate=3.0), shortlist=Shortlist(live, keep=6),
                              shortlist_hold=2)
        quiet, asked = pool(), pool()
        hq, ha = quiet.open(), asked.open()
        t, explained = 0, 0
        for i, n in enumerate(PUSHES):
            x = quiet.push_features({hq: rows[t:t + n].contiguous()})[hq]
            y = asked.push_features({ha: rows[t:t + n].contiguous()})[ha]
            t += n
            assert x.first_window == y.first_window
            for name in ("logits", "smoothed", "deviation", "columns"):
                u, v = getattr(x, name), getattr(y, name)
                assert (u is None and v is None) or (u.dtype == v.dtype and u.shape == v.shape and torch.equal(
                    u.view(torch.int32), v.view(torch.int32))), (i, name)
            if len(asked.enrolable(ha)):
                state = (asked.stats(ha), asked._sessions[ha].tick, asked._ring.clone())
                asked.explain(ha, k=3)
                asked.explain(ha, [5, 17], window=asked.enrolable(ha)[0])
                with pytest.raises(ValueError, match="is not enrolable"):
                    asked.explain(ha, [5], window=asked.enrolable(ha)[-1] + 1)
                assert (asked.stats(ha), asked._sessions[ha].tick) == state[:2] and torch.equal(asked._ring, state[2])
                explained += 1
        assert explained >= 8
        events = asked.take_events()
        assert repr(quiet.take_events()) == repr(events)
        assert repr(quiet.active(hq)) == repr(asked.active(ha)) and repr(quiet.baseline(hq)) == repr(asked.baseline(ha))
        assert quiet.stats() == asked.stats()
        for e in events:                                                            # of an event: the window it names, if still in the ring
            if e.window in asked.enrolable(e.session):
                a = asked.explain(e.session, [e.class_id], window=e.window)
                assert a.class_ids() == [[e.class_id]] and bool(torch.isfinite(a.plan).all())
