"""GPU: the shot ledger (clip_fsar_amd.live_gallery.LiveGallery(ledger=ShotLedger(...)) on libclipfsar_ledger.so) -- cfld_put against
index_copy_, cfld_resum against cfsl_accumulate on the gathered addends and against a sequential fp32 loop (bit for bit), cfld_fit
against reference_fit in float64 under a bound derived from its chain lengths; the gallery with the option against the gallery
without it, remove_shots against cfsl_accumulate over the stored addends and against a twin that only ever saw the remaining shots,
per_class against add-then-remove, move_shots, state dicts, unledgered classes, the audit on the test tower, and a StreamPool's
enrolment undone while its sessions run."""
import math

import numpy as np
import pytest
import torch

import clip_fsar_amd.synth as synth
from _cases import maxdiff
from test_gpu_gallery import BOUND, DEV, _head

pytestmark = pytest.mark.gpu

ARCH, T = "ViT-test/16", 8
L = T + 1
U = 2.0 ** -24                                    # fp32 unit roundoff
ES = [4, 8, 252, 512]
GUARD = 777.0


def _guarded(shape, fill=GUARD):
    """(a buffer with one guard item before and behind, its inner view of `shape`)"""
    buf = torch.full((shape[0] + 2,) + tuple(shape[1:]), fill, device=DEV)
    return buf, buf[1:-1]


def _i32(values):
    return torch.tensor(values, device=DEV, dtype=torch.int32)


def _bits(t):
    """a float tensor as its bits: slots nobody wrote may hold NaN patterns, which compare unequal as floats"""
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------ 1: the kernels through the binding
@pytest.mark.parametrize("rows_kept", [1, T, T + 1])
@pytest.mark.parametrize("E", ES)
def test_put_is_index_copy(E, rows_kept):
    from clip_fsar_amd import ledger_hip as lh
    shots, slots = 12, [7, -1, 0, 12, 3, 11, 1 << 30]          # two below / above the store and one far outside: not kept
    Nv = len(slots)
    X = torch.randn(Nv, L, E, generator=torch.Generator().manual_seed(E + rows_kept)).to(DEV)
    x0 = X.clone()
    buf, store = _guarded((shots, rows_kept, E))
    want = buf.clone()
    kept = [v for v, s in enumerate(slots) if 0 <= s < shots]
    want[1:-1].index_copy_(0, torch.tensor([slots[v] for v in kept], device=DEV), X[kept][:, :rows_kept])
    sl = _i32(slots)
    lh.put(X, store, sl)
    torch.cuda.synchronize()
    first = buf.clone()
    lh.put(X, store, sl)
    torch.cuda.synchronize()
    assert torch.equal(buf, want) and torch.equal(first, want) and torch.equal(X, x0) and sl.tolist() == slots


COUNTS = [1, 2, 3, 17, 2]                         # a class's N
CLASS_SLOTS = [5, 0, 6, 2, 8]                     # of a gallery store of 9


def _ledger_case(E, rows_kept, seed, scale=3.0):
    """a store of 40 addends, 25 of them the shots of five classes: ledger slots out of order and interleaved between the classes
    -> (store, rows [(class slot, first, n)], list of ledger slots)"""
    g = torch.Generator().manual_seed(seed)
    store = (torch.randn(40, rows_kept, E, generator=g) * scale).to(DEV)
    perm = torch.randperm(40, generator=g).tolist()
    mine = [[] for _ in COUNTS]
    while any(len(m) < n for m, n in zip(mine, COUNTS)):         # dealt round the classes
        for m, n in zip(mine, COUNTS):
            if len(m) < n:
                m.append(perm.pop())
    rows, flat = [], []
    for slot, m in zip(CLASS_SLOTS, mine):
        rows.append([slot, len(flat), len(m)])
        flat += m
    return store, rows, flat


def _sequential(store, slots):
    """a = 0; a = a + x in list order, fp32 on the device; and a * (1 / n) with the quotient rounded once"""
    a = torch.zeros_like(store[0])
    for s in slots:
        a = a + store[s]
    inv = (torch.tensor(1.0) / torch.tensor(float(len(slots)))).item()
    return a, a * inv


@pytest.mark.parametrize("rows_kept", [1, T, T + 1])
@pytest.mark.parametrize("E", ES)
def test_resum_is_accumulate_on_the_gathered_addends(E, rows_kept):
    from clip_fsar_amd import ledger_hip as lh
    from clip_fsar_amd import live_hip as live
    cap = 9
    store, rows5, flat5 = _ledger_case(E, rows_kept, 100 + E + rows_kept)
    s0 = store.clone()
    up, lup = lh.table_uploader(DEV, 8), live.table_uploader(DEV, 8)
    for rows, flat in ((rows5, flat5), ([[rows5[2][0], 0, 3]], flat5[rows5[2][1]:rows5[2][1] + 3])):         # 5 table rows, and 1
        S = len(rows)
        # the existing kernel is the reference: cfsl_accumulate, prior = 0, on the addends gathered in list order
        X = store[torch.tensor(flat, device=DEV)].contiguous()
        ref_sums = torch.full((cap, rows_kept, E), GUARD, device=DEV)
        ref_means = torch.full((cap, rows_kept, E), GUARD, device=DEV)
        live.accumulate(X, ref_sums, ref_means, lup.upload([[s, f, n, 0] for s, f, n in rows]), by_slot=True)
        for by_slot in (True, False):
            sbuf, sums = _guarded((cap, L, E))
            mbuf, means = _guarded((cap if by_slot else S, rows_kept, E))
            lst = _i32(flat)
            table = up.upload(rows)
            lh.resum(store, lst, sums, means, table, by_slot)
            torch.cuda.synchronize()
            again = (sbuf.clone(), mbuf.clone())
            lh.resum(store, lst, sums, means, table, by_slot)
            torch.cuda.synchronize()
            assert torch.equal(sbuf, again[0]) and torch.equal(mbuf, again[1])
            assert torch.equal(store, s0) and lst.tolist() == flat and bool((sbuf[0] == GUARD).all() and (sbuf[-1] == GUARD).all())
            assert bool((mbuf[0] == GUARD).all() and (mbuf[-1] == GUARD).all())
            touched = [r[0] for r in rows]
            for i, (slot, first, n) in enumerate(rows):
                a, mean = _sequential(store, flat[first:first + n])
                at = slot if by_slot else i
                assert torch.equal(sums[slot, :rows_kept], ref_sums[slot]) and torch.equal(means[at], ref_means[slot]), (slot, by_slot)
                assert torch.equal(sums[slot, :rows_kept], a) and torch.equal(means[at], mean), (slot, by_slot)
                assert bool((sums[slot, rows_kept:] == GUARD).all())                      # the rows cfsl_accumulate leaves alone
            rest = [s for s in range(cap) if s not in touched]
            assert bool((sums[rest] == GUARD).all()) and (not by_slot or bool((means[rest] == GUARD).all()))


def test_a_refused_row_and_a_slot_outside_the_store_write_nothing():
    from clip_fsar_amd import ledger_hip as lh
    E, rows_kept, cap = 8, T, 9
    store, rows, flat = _ledger_case(E, rows_kept, 7)
    good = lh.table_uploader(DEV, 8).upload(rows)
    for col, value in ((lh.N, 0), (lh.N, 26), (lh.FIRST, -1), (lh.SLOT, 9), (lh.SLOT, -1)):       # the DEVICE copy of row 1 alone is bad
        dev = good.dev.clone()
        dev[1, col] = value
        for by_slot in (True, False):
            sums = torch.full((cap, L, E), GUARD, device=DEV)
            means = torch.full((cap if by_slot else 5, rows_kept, E), GUARD, device=DEV)
            fit = torch.full((25,), GUARD, device=DEV)
            lh.resum(store, _i32(flat), sums, means, lh.Table(good.host, dev, 5), by_slot)
            lh.fit(store, sums, _i32(flat), fit, lh.Table(good.host, dev, 5), T)
            torch.cuda.synchronize()
            assert bool((sums[rows[1][0]] == GUARD).all()) and bool((means[rows[1][0] if by_slot else 1] == GUARD).all()), (col, value)
            for i in (0, 2, 3, 4):
                assert torch.equal(sums[rows[i][0], :rows_kept], _sequential(store, flat[rows[i][1]:rows[i][1] + rows[i][2]])[0])
            if col != lh.FIRST:                   # (a FIRST below 0 sends the bisection of the positions behind it elsewhere too)
                assert bool((fit[1:3] == GUARD).all()) and bool((fit[:1] != GUARD).all()) and bool((fit[3:] != GUARD).all())
    for bad in (40, -1, 1 << 30):                 # a ledger slot outside [0, 40) in class 3's list: the class keeps its sum
        broken = list(flat)
        broken[rows[3][1] + 5] = bad
        sums = torch.full((cap, L, E), GUARD, device=DEV)
        means = torch.full((cap, rows_kept, E), GUARD, device=DEV)
        fit = torch.full((25,), GUARD, device=DEV)
        lh.resum(store, _i32(broken), sums, means, good, True)
        torch.cuda.synchronize()
        assert bool((sums[rows[3][0]] == GUARD).all()) and bool((means[rows[3][0]] == GUARD).all())
        for i in (0, 1, 2, 4):
            assert torch.equal(sums[rows[i][0], :rows_kept], _sequential(store, flat[rows[i][1]:rows[i][1] + rows[i][2]])[0])
        lh.fit(store, sums, _i32(broken), fit, good, T)
        torch.cuda.synchronize()
        at = rows[3][1] + 5
        assert float(fit[at]) == GUARD and bool((fit[:at] != GUARD).all()) and bool((fit[at + 1:] != GUARD).all())


def _chain(E):
    """fused steps of one lane's chain in cfld_fit: a lane takes 4 elements per 256 of the row"""
    return 4 * math.ceil(E / 256)


def fit_bound(addends, T_, E):
    """|cfld_fit - reference_fit| per shot of one class, derived, not tuned.  addends [N, rows, E] float64.  Per row: each of the three
    dots is a chain of _chain(E) fused steps per lane plus 6 tree adds, so its error is at most (chain + 6) u of the sum of its
    terms' magnitudes -- for <x, x> and <m, m> the value itself, for <x, m> at most |x| |m| -- which moves the cosine by at most
    2 (chain + 6) u; the product, the square root and the division round once each: 3 u.  m itself is sums - x: a sequential fp32 sum
    of N addends and one subtraction, off per element by at most N u sum_i |x_i|, which turns m by at most N u kappa,
    kappa = |sum_i |x_i|| / |m|; twice that bounds the cosine's move, second order included.  The mean adds T - 1 sums and one
    product of values of at most 1: (T + 1) u."""
    x = np.asarray(addends, dtype=np.float64)[:, :T_]
    N = x.shape[0]
    mag = np.abs(x).sum(axis=0)                                                           # [T, E]
    m = np.stack([np.delete(x, i, axis=0).sum(axis=0) for i in range(N)])                # [N, T, E]
    with np.errstate(invalid="ignore", divide="ignore"):                                 # m = 0: the fit is NaN, and so is its bound
        kappa = np.linalg.norm(mag, axis=-1)[None] / np.linalg.norm(m, axis=-1)          # [N, T]
    per_row = U * (2 * (_chain(E) + 6) + 3 + 2 * N * kappa)
    return per_row.mean(axis=1) + (T_ + 1) * U, kappa


@pytest.mark.parametrize("rows_kept", [T, T + 1])
@pytest.mark.parametrize("E", ES)
def test_fit_against_the_float64_restatement(E, rows_kept):
    from clip_fsar_amd import ledger_hip as lh
    from clip_fsar_amd.ledger import reference_fit
    cap = 9
    store, rows, flat = _ledger_case(E, rows_kept, 300 + E + rows_kept, scale=0.3)
    g = torch.Generator().manual_seed(E)
    store += (2.0 + torch.rand(1, rows_kept, 1, generator=g)).to(DEV) * torch.randn(1, rows_kept, E, generator=g).sign().to(DEV)    # norms away from 0
    # a sixth class of three shots x, -x, y: the others of y cancel exactly, m = 0 -> NaN
    free = [s for s in range(40) if s not in flat][:3]
    store[free[1]] = -store[free[0]]
    rows = rows + [[1, len(flat), 3]]
    flat = flat + free
    sums = torch.full((cap, L, E), GUARD, device=DEV)
    for slot, first, n in rows:
        sums[slot, :rows_kept] = _sequential(store, flat[first:first + n])[0]
    s0, m0 = store.clone(), sums.clone()
    buf, fit = _guarded((len(flat),))
    table = lh.table_uploader(DEV, 8).upload(rows)
    lh.fit(store, sums, _i32(flat), fit, table, T)
    torch.cuda.synchronize()
    first_run = buf.clone()
    lh.fit(store, sums, _i32(flat), fit, table, T)
    torch.cuda.synchronize()
    assert torch.equal(buf.view(torch.int32), first_run.view(torch.int32))                # identical bytes, NaNs included
    assert torch.equal(store, s0) and torch.equal(sums, m0) and float(buf[0]) == GUARD and float(buf[-1]) == GUARD
    got = fit.cpu().double().numpy()
    worst = derived = 0.0
    kappas = []
    for slot, first, n in rows:
        x = store[torch.tensor(flat[first:first + n], device=DEV)].cpu().double().numpy()
        ref = reference_fit(x, T)
        mine = got[first:first + n]
        if n == 1:
            assert np.isnan(ref).all() and np.isnan(mine).all()
            continue
        nan = np.isnan(ref)
        assert np.array_equal(nan, np.isnan(mine)), (slot, ref, mine)
        assert nan.tolist() == ([False, False, True] if slot == 1 else [False] * n)
        bound, kappa = fit_bound(x, T, E)
        err = np.abs(mine - ref)[~nan]
        worst, derived = max(worst, float(err.max())), max(derived, float(bound[~nan].max()))
        if slot != 1:                             # but for the class built to cancel, the shots share a direction: m is well-conditioned
            assert float(kappa.max()) < 2.5, (slot, kappa.max())
            kappas.append(float(kappa.max()))
        assert bool((err <= bound[~nan]).all()), (slot, err, bound)
    print("cfld_fit E %d rows_kept %d: |fit - float64| max %.2e, derived bound (its largest) %.2e; kappa at most %.2f outside the "
          "cancelling class" % (E, rows_kept, worst, derived, max(kappas)))


@pytest.mark.parametrize("E", ES)
def test_fit_on_inputs_whose_dots_are_exact(E):
    """Small integers: every product, every partial sum of the three dots and the subtraction are exact in fp32 whatever the order, so
    nothing of the chain-length terms of fit_bound applies and a term dropped or taken twice anywhere in a chain shows at once.  What is
    left per row: the product <x, x> <m, m>, the square root and the division round once each (3 u on a cosine of at most 1); the mean
    adds (T + 1) u."""
    from clip_fsar_amd import ledger_hip as lh
    from clip_fsar_amd.ledger import reference_fit
    N, cap = 3, 4
    g = torch.Generator().manual_seed(500 + E)
    x = torch.randint(-3, 4, (N, T, E), generator=g).float()
    x[:, :, 0] = 2.0                                                                      # no row of x or m is zero
    assert float((x.abs().sum(0) ** 2).sum(-1).max()) < 2 ** 24                           # the largest dot any order could meet
    store = torch.full((8, T, E), GUARD)
    slots = [6, 1, 3]
    store[slots] = x
    store = store.to(DEV)
    sums = torch.full((cap, L, E), GUARD, device=DEV)
    sums[2, :T] = x.sum(0).to(DEV)
    fit = torch.full((N,), GUARD, device=DEV)
    lh.fit(store, sums, _i32(slots), fit, lh.table_uploader(DEV, 4).upload([[2, 0, N]]), T)
    torch.cuda.synchronize()
    err = np.abs(fit.cpu().double().numpy() - reference_fit(x.double().numpy(), T))
    print("cfld_fit on exact dots, E %d: |fit - float64| max %.2e, bound %.2e" % (E, err.max(), (T + 4) * U))
    assert bool((err <= (T + 4) * U).all()), err


# ------------------------------------------------------------------ 2: the gallery
CONFIGS = [("fp32", False), ("bf16", False), ("fp32", True), ("bf16", True)]


def _gallery(precision="fp32", merge_before=False, ledger=None, capacity=4):
    from clip_fsar_amd.live_gallery import LiveGallery
    head = _head(ARCH, precision, T)
    head.args.TRAIN.MERGE_BEFORE = merge_before
    head.args.TRAIN.SINGLE_DIRECT = False
    return LiveGallery(head, DEV, capacity=capacity, ledger=ledger) if ledger is not None else LiveGallery(head, DEV, capacity=capacity)


def _videos(n, seed):
    a = synth.ARCHS[ARCH]
    return (torch.randn(n, T, 3, a["res"], a["res"], generator=torch.Generator().manual_seed(seed)) * 0.5).to(DEV)


def _feats(n, E, seed):
    return torch.randn(n, T, E, generator=torch.Generator().manual_seed(seed)).to(DEV)


def _dense(live):
    """(prototypes, norms, sums) of a LiveGallery in column order"""
    idx = torch.tensor([live.slot_of(c) for c in live.class_ids], device=DEV)
    st = live._store
    return st["P"][idx], st["pn"].view(-1, T)[idx], st["sums"][idx][:, :(T + 1 if live.merge_before else T)]


def _same(a, b):
    return a.class_ids == b.class_ids and [a.shots(c) for c in a.class_ids] == [b.shots(c) for c in b.class_ids] and all(
        torch.equal(x, y) for x, y in zip(_dense(a), _dense(b)))


@pytest.mark.parametrize("precision,merge_before", CONFIGS)
def test_with_the_option_every_call_gives_the_bits_it_gave(precision, merge_before):
    from clip_fsar_amd.ledger import Shot, ShotLedger
    V, W, Q = _videos(6, 11), _videos(3, 12), _videos(5, 13)
    with torch.no_grad():
        plain, led = _gallery(precision, merge_before), _gallery(precision, merge_before, ShotLedger(shots=32, features=True))
        E = plain.E
        F, G = _feats(4, E, 14), _feats(3, E, 15)
        assert plain.add_classes(V, [0, 0, 1, 2, 2, 2]) == led.add_classes(V, [0, 0, 1, 2, 2, 2]) == [0, 1, 2]
        assert led.last_shots == [0, 1, 2, 3, 4, 5]
        assert plain.add_classes_features(F, [5, 7, 5, 9]) == led.add_classes_features(F, [5, 7, 5, 9]) == [3, 4, 5]      # the store grows
        assert led.last_shots == [6, 8, 7, 9]                                             # video order: class 5 holds serials 6 and 7
        assert plain.add_shots(W, [2, 0, 2]) == led.add_shots(W, [2, 0, 2]) == [5, 3]
        assert led.last_shots == [10, 12, 11]
        assert plain.add_shots_features(G, [7, 1, 7]) == led.add_shots_features(G, [7, 1, 7]) == [3, 2]
        assert led.last_shots == [13, 15, 14]
        assert _same(plain, led)
        assert torch.equal(plain.classify(Q), led.classify(Q))
        assert led.shot_list(2) == [Shot(3, 2, "add_classes"), Shot(4, 2, "add_classes"), Shot(5, 2, "add_classes"), Shot(10, 2, "add_shots"),
                                    Shot(11, 2, "add_shots")]
        assert led.shot_list(7) == [Shot(8, 7, "enroll"), Shot(13, 7, "enroll"), Shot(14, 7, "enroll")]
        assert torch.equal(led.shot_features(7), F[2]) and torch.equal(led.shot_features(14), G[2])
        assert led.shot_features(7).data_ptr() != led.shot_features(7).data_ptr()        # a copy
        plain.remove_classes([1, 5])
        led.remove_classes([1, 5])
        assert _same(plain, led) and torch.equal(plain.classify(Q), led.classify(Q, classes=None))
        assert sorted(led._lbook.free)[:4] == [2, 6, 7, 15] and "ledger" not in plain.state_dict() and "ledger" in led.state_dict()
        assert plain.add_classes_features(F[:1], [11]) == led.add_classes_features(F[:1], [11]) == [4]
        assert led._lbook.slot_of[16] == 2 and _same(plain, led)                          # the lowest freed ledger slot, a new serial


@pytest.mark.parametrize("precision,merge_before", CONFIGS)
def test_remove_shots_resums_the_remaining_addends(precision, merge_before):
    from clip_fsar_amd import gallery_hip as gh
    from clip_fsar_amd import live_hip as lh
    from clip_fsar_amd.ledger import ShotLedger
    ids = [0, 0, 0, 1, 2, 2, 2, 2, 5, 5]
    with torch.no_grad():
        led = _gallery(precision, merge_before, ShotLedger(shots=16), capacity=6)
        E, rk = led.E, (T + 1 if merge_before else T)
        F, Q = _feats(len(ids), E, 21), _feats(9, E, 22)
        led.add_classes_features(F[:8], ids[:8])
        led.add_shots_features(F[8:], [0, 2])                                            # class 0: serials 0 1 2 8, class 2: 4 5 6 7 9
        led.add_classes_features(_feats(2, E, 23), ids[8:])
        assert [s.serial for s in led.shot_list(0)] == [0, 1, 2, 8] and [s.serial for s in led.shot_list(2)] == [4, 5, 6, 7, 9]
        before = {k: v.clone() for k, v in led._store.items()}
        gens = [led.slot_generation(s) for s in range(led.capacity)]
        revs = [led.slot_revision(s) for s in range(led.capacity)]
        version, cols = led.layout_version, led.class_ids
        for bad, words in (([99], "not the serial"), ([1, 1], "twice"), ([3], "use remove_classes"), ([10, 11], "use remove_classes")):
            with pytest.raises(ValueError, match=words):
                led.remove_shots(bad)
        assert all(torch.equal(_bits(led._store[k]), _bits(v)) for k, v in before.items())
        assert led.remove_shots([5, 1, 9]) == [3, 3]                                       # classes 2 and 0, in that order
        torch.cuda.synchronize()
        st, touched = led._store, [led.slot_of(2), led.slot_of(0)]
        assert [s.serial for s in led.shot_list(0)] == [0, 2, 8] and [s.serial for s in led.shot_list(2)] == [4, 6, 7]
        assert led.shots(0) == 3 and led.shots(2) == 3 and led.shots(1) == 1 and led.shots(5) == 2
        # the touched slots: cfsl_accumulate over the stored addends of the remaining shots, in ledger order
        for c, slot in zip((2, 0), touched):
            addends = led._lstore["addends"][torch.tensor([led._lbook.slot_of[s.serial] for s in led.shot_list(c)], device=DEV)].contiguous()
            sums = torch.empty(1, rk, E, device=DEV)
            means = torch.empty(1, rk, E, device=DEV)
            lh.accumulate(addends, sums, means, lh.table_uploader(DEV, 4).upload([[0, 0, 3, 0]]), by_slot=True)
            assert torch.equal(st["sums"][slot, :rk], sums[0]), c
            if not merge_before:
                pn = torch.empty(T, device=DEV)
                gh.row_norms(means, pn)
                assert torch.equal(st["P"][slot], means[0]) and torch.equal(st["pn"].view(-1, T)[slot], pn), c
            assert not torch.equal(st["P"][slot], before["P"][slot])
        rest = [s for s in range(led.capacity) if s not in touched]
        for k in ("P", "sums", "text"):
            assert torch.equal(_bits(st[k][rest]), _bits(before[k][rest])), k
        assert torch.equal(_bits(st["pn"].view(-1, T)[rest]), _bits(before["pn"].view(-1, T)[rest]))
        assert torch.equal(_bits(st["sums"][touched][:, rk:]), _bits(before["sums"][touched][:, rk:]))
        assert [led.slot_generation(s) for s in range(led.capacity)] == gens and led.layout_version == version and led.class_ids == cols
        assert [led.slot_revision(s) - r for s, r in enumerate(revs)] == [int(s in touched) for s in range(led.capacity)]
        # a twin that only ever registered the remaining shots: "same clip, another batch"
        twin = _gallery(precision, merge_before, capacity=6)
        keep = [0, 2, 3, 4, 6, 7]
        twin.add_classes_features(F[keep], [ids[i] for i in keep])
        twin.add_shots_features(F[8:9], [0])
        twin.add_classes_features(_feats(2, E, 23), ids[8:])
        a, b = led.classify_features(Q), twin.classify_features(Q)
    d = maxdiff(a.cpu(), b.cpu())
    print("remove_shots vs a twin of the remaining shots, %s merge_before=%d: |dlogits| = %.2e" % (precision, merge_before, d))
    assert d <= BOUND, d
    assert torch.equal(a.argmax(1), b.argmax(1))


@pytest.mark.parametrize("precision,merge_before", CONFIGS)
def test_per_class_is_add_then_remove_step_by_step(precision, merge_before):
    from clip_fsar_amd.ledger import ShotLedger
    with torch.no_grad():
        cap, free = _gallery(precision, merge_before, ShotLedger(shots=6, per_class=2)), _gallery(precision, merge_before, ShotLedger(shots=16))
        E = cap.E
        F = _feats(3, E, 31)
        for g in (cap, free):
            g.add_classes_features(F, [3, 3, 4])
        #        five add_shots: one shot, one shot (class 4 reaches its cap), both classes at once, three at once, one
        for step, ids in enumerate([[3], [4], [4, 3], [3, 3, 3], [4]]):
            f = _feats(len(ids), E, 40 + step)
            got = cap.add_shots_features(f, ids)
            free.add_shots_features(f, ids)
            over = [s.serial for c in dict.fromkeys(ids) for s in free.shot_list(c)[:-2]]
            want = free.remove_shots(over) if over else [free.shots(c) for c in dict.fromkeys(ids)]
            assert got == want == [2] * len(set(ids)) and cap.last_shots == free.last_shots, step
            assert _same(cap, free), step
            assert [cap.shot_list(c) for c in (3, 4)] == [free.shot_list(c) for c in (3, 4)], step
            assert 6 - len(cap._lbook.free) == cap.shots(3) + cap.shots(4) <= 4           # a store of 6 never holds more than 2 + 2
        assert [s.serial for s in cap.shot_list(3)] == [8, 9] and torch.equal(cap.classify_features(F), free.classify_features(F))


def test_move_shots_is_remove_and_add_by_hand_and_a_full_store_refuses():
    from clip_fsar_amd.ledger import ShotLedger
    with torch.no_grad():
        a, b = (_gallery(ledger=ShotLedger(shots=5, features=True)) for _ in range(2))
        F = _feats(5, a.E, 51)
        for g in (a, b):
            g.add_classes_features(F, [0, 0, 0, "kite", "kite"], text={"kite": F[0, 0]})
        with pytest.raises(ValueError, match="not registered"):
            a.move_shots([1], "owl")
        with pytest.raises(ValueError, match="the shot ledger is full -- the call needs 1 more addends, 0 of 5 are free"):
            a.add_shots_features(F[:1], [0])
        with pytest.raises(ValueError, match="the shot ledger is full"):
            a.add_classes_features(F[:1], [9])
        assert _same(a, b) and a.last_shots == [0, 1, 2, 3, 4] and a.class_ids == [0, "kite"]
        assert a.move_shots([1], "kite") == [5]
        feats = b.shot_features(1)
        assert torch.equal(feats, F[1])
        assert b.remove_shots([1]) == [2] and b.add_shots_features(feats[None], ["kite"]) == [3]
        assert _same(a, b) and a.shot_list("kite") == b.shot_list("kite") and [s.serial for s in a.shot_list("kite")] == [3, 4, 5]
        assert a.shot_list("kite")[-1].origin == "enroll" and torch.equal(a.shot_features(5), F[1])
        # remove_classes frees the ledger slots for reuse
        a.remove_classes([0])
        assert sorted(a._lbook.free) == [0, 2] and a.add_classes_features(F[:2], [8, 8]) == [1]
        assert [a._lbook.slot_of[s] for s in a.last_shots] == [0, 2] and a._lbook.free == []
        a.clear()
        assert len(a._lbook.free) == 5 and a.add_classes_features(F[:1], [0]) == [0] and a.last_shots == [8]


def test_state_dict_round_trips_and_a_state_without_a_ledger_gives_unledgered_classes():
    from clip_fsar_amd.gallery import SupportGallery
    from clip_fsar_amd.ledger import ShotLedger
    with torch.no_grad():
        led = _gallery(ledger=ShotLedger(shots=16, features=True))
        E = led.E
        F, Q = _feats(7, E, 61), _feats(4, E, 62)
        led.add_classes_features(F[:5], [0, 0, 1, 2, 2])
        led.add_shots_features(F[5:], [2, 0])
        led.remove_shots([3])
        sd = led.state_dict()
        assert sd["ledger"]["serials"] == [0, 1, 6, 2, 4, 5] and sd["ledger"]["class_ids"] == [0, 0, 0, 1, 2, 2]
        assert tuple(sd["ledger"]["addends"].shape) == (6, T, E) and tuple(sd["ledger"]["features"].shape) == (6, T, E)
        other = _gallery(ledger=ShotLedger(shots=8, features=True), capacity=2)
        other.load_state_dict(sd)
        assert _same(led, other) and [other.shot_list(c) for c in (0, 1, 2)] == [led.shot_list(c) for c in (0, 1, 2)]
        assert led.remove_shots([1, 4]) == other.remove_shots([1, 4]) == [2, 1] and _same(led, other)
        assert torch.equal(led.classify_features(Q), other.classify_features(Q))
        f = _feats(1, E, 63)
        assert led.add_shots_features(f, [1]) == other.add_shots_features(f, [1]) and led.last_shots == other.last_shots == [7]
        with pytest.raises(ValueError, match="holds 6 shots, this gallery's ShotLedger\\(shots=4\\)"):
            _gallery(ledger=ShotLedger(shots=4)).load_state_dict(sd)
        sup = SupportGallery(led.head, DEV)
        sup.load_state_dict(sd)                                                            # it ignores the key
        assert sup.class_ids == sd["class_ids"]
        # a state without "ledger"
        plain = _gallery()
        plain.load_state_dict(sd)
        assert "ledger" not in plain.state_dict()
        un = _gallery(ledger=ShotLedger(shots=8))
        un.load_state_dict(plain.state_dict())
        assert _same(un, plain) and un.shot_list(0) == [] and un.shot_fits() == {}
        for call in (lambda: un.remove_shots([0]), lambda: un.shot_fit(0)):
            with pytest.raises(ValueError, match="not the serial of a ledgered shot|is unledgered"):
                call()
        assert un.add_shots_features(f, [0]) == plain.add_shots_features(f, [0]) == [4] and _same(un, plain) and un.shot_list(0) == []
        assert un.add_classes_features(f, [9]) == [3] and [s.serial for s in un.shot_list(9)] == un.last_shots     # a new class is ledgered


def test_shot_fit_finds_the_unrelated_clip():
    from clip_fsar_amd.ledger import ShotLedger, reference_fit
    with torch.no_grad():
        led = _gallery(ledger=ShotLedger(shots=8))
        clip, other = _videos(1, 71), _videos(1, 72)
        noise = torch.randn(4, *clip.shape[1:], generator=torch.Generator().manual_seed(73)).to(DEV) * 0.01
        led.add_classes(torch.cat([clip + noise, other]), [7] * 5)
        led.add_classes(_videos(1, 74), [8])
        fits = led.shot_fit(7)
        both = led.shot_fits()
    assert [s for s, _ in fits] == [0, 1, 2, 3, 4] and both[7] == fits and math.isnan(both[8][0][1]) and list(both) == [7, 8]
    values = [f for _, f in fits]
    x = led._lstore["addends"][:5].cpu().double().numpy()
    ref = reference_fit(x, T)
    err, bound = np.abs(np.array(values) - ref), fit_bound(x, T, led.E)[0]
    print("shot_fit, four noisy copies and an unrelated clip: fits %s; |fit - float64| max %.2e, derived bound %.2e" % (
        ["%.4f" % v for v in values], err.max(), bound.max()))
    assert bool((err <= bound).all())
    assert values.index(min(values)) == 4 and min(values[:4]) > values[4]


# ------------------------------------------------------------------ 3: the pool
def test_an_enrolment_is_undone_while_sessions_run():
    from clip_fsar_amd.ledger import ShotLedger
    from clip_fsar_amd.pool import StreamPool
    from clip_fsar_amd.shortlist import Shortlist
    from test_gpu_class_smooth import _smooth_reference
    alpha = 0.5
    with torch.no_grad():
        live = _gallery(ledger=ShotLedger(shots=16), capacity=6)
        E = live.E
        live.add_classes_features(_feats(5, E, 81), [1, 2, 7, 7, 9])
        pool = StreamPool(live, max_streams=2, max_push=16, smooth=alpha, smooth_by="class")
        sl = Shortlist(live, keep=2)
        Q = _feats(3, E, 82)
        sl.classify_features(Q)
        assert sl.stats["refreshed"] == 4
        h = pool.open()
        frames = torch.randn(3 * T, E, generator=torch.Generator().manual_seed(83)).to(DEV)
        raw, smooth = [], []

        def push(lo, hi):
            out = pool.push_features({h: frames[lo:hi]})[h]
            raw.append(out.logits)
            smooth.append(out.smoothed)
            return out

        push(0, T + 2)
        before = live._store["P"][live.slot_of(7)].clone()
        gens = live.slot_generations().clone()
        assert pool.enroll(h, 7) == 3                                                      # "that was not class 7"
        serials = live.last_shots
        assert len(serials) == 1 and live.shot_list(7)[-1].serial == serials[0] and live.shot_list(7)[-1].origin == "enroll"
        sl.classify_features(Q)
        assert sl.stats["refreshed"] == 5
        push(T + 2, T + 5)
        assert live.remove_shots(serials) == [2]
        torch.cuda.synchronize()
        assert torch.equal(live._store["P"][live.slot_of(7)], before) and torch.equal(live.slot_generations(), gens)
        sl.classify_features(Q)
        assert sl.stats["refreshed"] == 6                                                  # the touched slot alone
        out = push(T + 5, T + 9)                                                           # no reset(): the session goes on
        windows = torch.stack([frames[i:i + T] for i in range(6, 10)])
        assert torch.equal(out.logits, live.classify_features(windows))
        x, y = torch.cat(raw), torch.cat(smooth)
        assert x.shape[0] == 10 and torch.equal(y, _smooth_reference(x, alpha))            # one recurrence through it all


def test_enroll_windows_with_known_and_new_classes_under_per_class():
    """one enroll_windows call is two gallery calls, both planned before either runs: further shots that take class 7 over its cap, and a
    new class.  The result is add, then remove_shots of the oldest, bit for bit; the counts, the state and last_shots say so too."""
    from clip_fsar_amd.ledger import ShotLedger
    from clip_fsar_amd.pool import StreamPool
    with torch.no_grad():
        live, ref = _gallery(ledger=ShotLedger(shots=8, per_class=1), capacity=6), _gallery(ledger=ShotLedger(shots=16), capacity=6)
        E = live.E
        F = _feats(2, E, 91)
        for g in (live, ref):
            g.add_classes_features(F, [7, 9])
        pool = StreamPool(live, max_streams=2, max_push=16)
        h = pool.open()
        frames = torch.randn(T + 3, E, generator=torch.Generator().manual_seed(92)).to(DEV)
        pool.push_features({h: frames})
        text = {"new": F[0, 0]}
        assert pool.enroll_windows([(h, 0, "new"), (h, 1, 7), (h, 2, "new"), (h, 3, 7)], text=text) == {"new": 1, 7: 1}
        assert live.last_shots == [4, 2, 5, 3]                                            # by item: the further shots were made first
        W = torch.stack([frames[i:i + T] for i in range(4)])
        assert ref.add_shots_features(W[[1, 3]], [7, 7]) == [3] and ref.add_classes_features(W[[0, 2]], ["new", "new"], text=text) == [2]
        assert ref.remove_shots([0, 2, 4]) == [1, 1]
        assert _same(live, ref) and [live.shots(c) for c in (7, 9, "new")] == [1, 1, 1]
        assert [live.shot_list(c) for c in (7, 9, "new")] == [ref.shot_list(c) for c in (7, 9, "new")]
        assert [s.serial for s in live.shot_list(7)] == [3] and len(live._lbook.free) == 5
        sd = live.state_dict()
        assert sd["counts"] == [1, 1, 1] and sd["ledger"]["serials"] == [3, 1, 5]
        other = _gallery(ledger=ShotLedger(shots=8, per_class=1))
        other.load_state_dict(sd)
        assert other._lbook.unledgered == frozenset() and [other.shot_list(c) for c in (7, 9, "new")] == [live.shot_list(c) for c in (7, 9, "new")]
        f = _feats(1, E, 93)
        assert live.add_shots_features(f, [7]) == other.add_shots_features(f, [7]) == [1] and _same(live, other)
