"""The three OTAM kernels -- cos_otam_kernel (cfsar_cos_otam_logits, the episode path), otam_gallery_kernel (cfsg_otam_gallery, the dense
tile kernel) and otam_indexed_kernel (cfsl_otam_indexed, the tile kernel over a slot list) -- at every T, at the tile edges and at the
edges of the 32-float K chunk, against the oracle's cos_sim and otam_cum_dist in float64 on the operands as stored (the restatement of
tests/test_gpu_gallery.py::_restated, evaluated once per (family, T) for every E of that family, at the largest NQ and C, and sliced:
pairs are independent).  With them: cfsg_row_norms and cfsg_topk on what the live gallery hands them, and the entry points' refusals.

Input families (seeded; Xq [NQ, T, E], P [C, T, E]):
  gauss   _features of test_gpu_gallery.py: a shared direction plus noise, per-row scale spread;
  ortho   independent randn, d ~ 1 everywhere: the largest cumulative costs that stay in range;
  near    one base direction plus 0.05 noise on both sides, d ~ 0.003 .. 0.01: the + 0.01 of the cosine denominator matters, and the
          soft-min over many equal paths drives the cost NEGATIVE (about -0.55 T);
  scale   gauss with every row times 10 ** U(-3, 3), frame 0 of query 0 and frame T - 1 of class 0 all zero (norm 0: sim 0, d = 1);
  anti    queries near +base, classes near -base (noise 0.3), d ~ 2; T <= 16 only.

Range condition.  The DP is un-stabilised like the reference: expf(-c / lambda) leaves the fp32 normal range near c = 87 lambda.  Every
compared case has a float64 per-direction |cost| of at most 64 lambda (32 at the product's lambda = 0.5); the tests assert it.

Tolerance.  The soft-min -lambda log sum exp(-c_i / lambda) is 1-Lipschitz in the max norm of its inputs, and every DP step moves one
column to the right, so a result depends on its inputs through chains of at most T + 1 cells.  Each cell adds its own rounding: the error
e_d of its distance plus the error of the soft-min, a few ulp of |c| + lambda.  Per case, with n_dir = 1 (single_direct) or 2:

    tol = n_dir * (T + 1) * (e_d + 4 * 2**-24 * (c_dir + lambda)),      e_d = 1e-6 * max(1, sqrt(E / 1024))

c_dir is the largest per-direction float64 |cost| among the pairs of the case; 1e-6 is the bound tests/test_gpu_gallery.py holds dists_out
to at E <= 1024, the square root the random-walk growth of an fp32 chain beyond that.  dists_out itself is held to e_d.  Two CPU tests pin
this to the reference and not to the kernels: the oracle evaluated in float32 stays within tol of its float64 value, element by element
with c_dir = that element's own cost (the tightest reading; worst err / tol: gauss 0.19, ortho 0.07, near 0.40, scale 0.19, anti 0.26), and
every case meets the range condition (largest |cost| / lambda 47.9, anti at T = 16).

Guards.  Every operand is a view into a larger buffer of NaN (of an out-of-range slot for a column list), 256 bytes of it before and behind
the view; every output is a view into a buffer of 7.0 whose surroundings must still be 7.0 afterwards.

Finding and fix.  With one chain of E dependent products per similarity (the tile GEMM of fp32_tile_gemm.h as it was), dists_out of the
dense kernel MISSED e_d on the two families whose similarities are +-1, where 1 - sim carries the whole relative error of a sum of
like-signed products: err / e_d 1.54 on near (T 9, E 512; 14 of its 15 (T, E) over) and 1.53 on anti (T 12, E 512; 9 of 10 over); gauss
0.79, scale 0.68, ortho 0.23.  The oracle evaluated in float32 on the CPU misses it the same way (1.30, 1.10); the episode kernel, which
sums 64 lane partials, does not.  The GEMM now sums every 32-float K chunk from zero and adds the chunk to the running sum.  That changes
the last bits of the similarities, hence of the logits of otam_gallery_kernel, otam_indexed_kernel and text_logits_kernel, at every
E > 32; tests/golden/otam_tile_bits.npz pins the new bits of the dense kernel at three product shapes.  No other kernel bug was found:
the indexed kernel gives the dense kernel's bits everywhere, poison stays in its column, nothing is read or written outside the operands
and outputs.  cfsg_topk: a -inf logit kept its index when its lane already held a class and got 0x7fffffff when it was its lane's first;
the kernel now skips -inf as it skips NaN (never selectable), which the top-k test pins index by index.

Measured on an MI355X with the chunked GEMM (run with -s for every figure); every logit and every dists_out element is inside its bound.
Worst logit err / tol -- dense (and indexed, same bits): gauss 0.12, ortho 0.14, near 0.11, scale 0.10, anti 0.17 (0.18, 0.14, 0.44, 0.15,
0.32 before the fix); episode: gauss 0.14, ortho 0.17, near 0.13, scale 0.15, anti 0.18.
Worst dists_out err / e_d -- dense: gauss 0.32 (T 16, E 28), ortho 0.09, near 0.36 (T 9, E 512), scale 0.18, anti 0.36 (T 3, E 512);
episode: gauss 0.31, ortho 0.29, near 0.37, scale 0.24, anti 0.35.

Mutations of the tile body, each built apart and run once against this file and against tests/test_gpu_gallery.py + test_gpu_live.py as
they were before it: ones instead of zeros staged for columns >= E fails test_tile_kernels_vs_float64 here, the earlier tests pass;
DP rows indexed by tid modulo half the slot count fails it here, and one earlier case (test_gpu_live's T = 5 bit comparison); the
dir = 1 strides swapped fails it here and 37 earlier cases.  Norm 0 instead of 1 for padding rows cannot be observed: a padding row is
all zero, so its dot products are 0 and d = 1 - 0 / (0 + 0.01) = 1 either way, and no DP reads a padding cell of an existing pair.
"""
import functools
import math

import pytest
import torch

import clipfsar_oracle as orc
from test_gpu_gallery import BOUND, _features, _restated

gpu = pytest.mark.gpu
DEV = torch.device("cuda")

NAN = float("nan")
SENT = 7.0
G = 64                                   # guard elements on either side of a view: 256 bytes, so views stay 16-byte aligned
BAD_SLOT = 1 << 30
ALL_T = list(range(1, 33))
EDGE_T = [1, 3, 4, 5, 7, 8, 9, 12, 13, 16, 17, 21, 22, 31, 32]
FAMILIES = ["gauss", "ortho", "near", "scale", "anti"]
FAMILY_T = {"gauss": ALL_T, "ortho": EDGE_T, "near": EDGE_T, "scale": EDGE_T, "anti": [t for t in EDGE_T if t <= 16]}
FAMILY_CASES = [(f, t) for f in FAMILIES for t in FAMILY_T[f]]
TILE_EDGE_E = [4, 28, 32, 36, 64, 68, 100]
TILE_LONG_E = [2048, 8192]
EP_E = [4, 60, 64, 252, 256, 260, 1024, 2048]
EP_COMBOS = [(B, Q, way) for B in (1, 3) for Q in (1, 4) for way in (1, 5, 7)]
LAMBDAS = [0.25, 1.0]


def tile_videos(T):
    return min(64 // T, 16)


def tile_shapes(T):
    qb = tile_videos(T)
    return list(dict.fromkeys([(1, 1), (qb, qb), (qb + 1, max(qb - 1, 1)), (max(qb - 1, 1), qb + 1), (2 * qb + 1, qb + 2)]))


def ref_size(T):
    """(NQ, C) of the reference: the largest tile shape and the largest episode (B Q = 12 queries, B way = 21 classes)"""
    qb = tile_videos(T)
    return max(2 * qb + 1, 12), max(qb + 2, 21)


def episode_lds_bytes(T, E):
    return (T * E + 32 + T * T + (0 if T in (8, 16) else 2 * 2 * 34)) * 4


def tile_es(family, T):
    es = [512]
    if family == "gauss" and T in EDGE_T:
        es += TILE_EDGE_E
    if family == "gauss" and T in (5, 8):
        es += TILE_LONG_E
    return es


def episode_es(T):
    return [E for E in EP_E if episode_lds_bytes(T, E) <= 150 * 1024]


def e_d_of(E):
    return 1e-6 * max(1.0, math.sqrt(E / 1024.0))


def tol_of(T, E, lam, n_dir, c_dir):
    return n_dir * (T + 1) * (e_d_of(E) + 4.0 * 2.0 ** -24 * (c_dir + lam))


# ---------------------------------------------------------------------------------------------------------------- inputs, reference
@functools.lru_cache(maxsize=16)
def make_inputs(family, T, E):
    """(Xq [NQ, T, E], P [C, T, E]) of a family at the reference's size: a function of (family, T, E) alone"""
    NQ, C = ref_size(T)
    seed = 100003 * FAMILIES.index(family) + 131 * T + E
    g = torch.Generator().manual_seed(seed)
    if family in ("gauss", "scale"):
        Xq, P = _features(NQ, C, T, E, seed)
        if family == "scale":
            Xq = Xq * 10.0 ** (6.0 * torch.rand(NQ, T, 1, generator=g) - 3.0)
            P = P * 10.0 ** (6.0 * torch.rand(C, T, 1, generator=g) - 3.0)
            Xq[0, 0] = 0.0
            P[0, T - 1] = 0.0
    elif family == "ortho":
        Xq, P = torch.randn(NQ, T, E, generator=g), torch.randn(C, T, E, generator=g)
    elif family == "near":
        base = torch.randn(E, generator=g)
        Xq, P = base + 0.05 * torch.randn(NQ, T, E, generator=g), base + 0.05 * torch.randn(C, T, E, generator=g)
    elif family == "anti":
        base = torch.randn(E, generator=g)
        Xq, P = base + 0.3 * torch.randn(NQ, T, E, generator=g), -base + 0.3 * torch.randn(C, T, E, generator=g)
    else:
        raise ValueError(family)
    return Xq.float().contiguous(), P.float().contiguous()


def restated_costs(pairs, lam, dtype=torch.float64):
    """test_gpu_gallery._restated's arithmetic (oracle cos_sim -> 1 - sim -> oracle otam_cum_dist) for several (Xq, P) of one (NQ, C, T) at
    once, per direction and with lambda: -> [(c0 [NQ, C], c1 [NQ, C], d [NQ, C, T, T])].  One pass of the oracle's T * T python steps
    serves every E of a (family, T)."""
    NQ, T, _ = pairs[0][0].shape
    C = pairs[0][1].shape[0]
    ds = []
    for Xq, P in pairs:
        sim = orc.cos_sim(Xq.to(dtype).reshape(NQ * T, -1), P.to(dtype).reshape(C * T, -1))
        ds.append((1.0 - sim).reshape(NQ, T, C, T).permute(0, 2, 1, 3))
    d = torch.stack(ds).reshape(len(pairs) * NQ, C, T, T).contiguous()
    c0 = orc.otam_cum_dist(d, lam).reshape(len(pairs), NQ, C)
    c1 = orc.otam_cum_dist(d.transpose(-1, -2), lam).reshape(len(pairs), NQ, C)
    d = d.reshape(len(pairs), NQ, C, T, T)
    return [(c0[i], c1[i], d[i]) for i in range(len(pairs))]


def family_es(family, T, lam):
    if lam != 0.5:
        return [512]
    return sorted(set(tile_es(family, T)) | set(episode_es(T)))


@functools.lru_cache(maxsize=None)
def family_costs(family, T, lam=0.5):
    """{E: (c0, c1)}: the float64 per-direction costs [NQ, C] of one (family, T, lambda) at every E, computed once and never changed"""
    es = family_es(family, T, lam)
    return {E: r[:2] for E, r in zip(es, restated_costs([make_inputs(family, T, E) for E in es], lam))}


@functools.lru_cache(maxsize=8)
def dists_ref(family, T, E):
    """the float64 distances [NQ, C, T, T] (no DP: cheap enough to evaluate again rather than keep for every case)"""
    Xq, P = make_inputs(family, T, E)
    NQ, C = Xq.shape[0], P.shape[0]
    sim = orc.cos_sim(Xq.double().reshape(NQ * T, E), P.double().reshape(C * T, E))
    return (1.0 - sim).reshape(NQ, T, C, T).permute(0, 2, 1, 3).contiguous()


class Case:
    """one (family, T, E, lambda): the inputs (regenerated from their seed), the float64 costs (kept) and distances"""

    def __init__(self, family, T, E, lam=0.5):
        self.family, self.T, self.E, self.lam = family, T, E, lam
        self.c0, self.c1 = family_costs(family, T, lam)[E]

    @property
    def Xq(self):
        return make_inputs(self.family, self.T, self.E)[0]

    @property
    def P(self):
        return make_inputs(self.family, self.T, self.E)[1]

    @property
    def d(self):
        return dists_ref(self.family, self.T, self.E)

    def ref(self, rows, cols, single_direct):
        """(float64 logits of the pairs rows x cols, c_dir of them)"""
        c0, c1 = self.c0[rows][:, cols], self.c1[rows][:, cols]
        if single_direct:
            return -c0, float(c0.abs().max())
        return -(c0 + c1), float(torch.maximum(c0.abs(), c1.abs()).max())


# ---------------------------------------------------------------------------------------------------------------- CPU: the tolerance
def test_restated_costs_is_the_gallery_tests_restatement():
    Xq, P = make_inputs("gauss", 5, 36)
    (c0, c1, d), = restated_costs([(Xq, P)], 0.5)
    for sd in (False, True):
        ref, dref = _restated(Xq, P, sd)
        assert torch.equal(ref, -(c0 if sd else c0 + c1)) and torch.equal(dref, d)


@pytest.mark.parametrize("family", FAMILIES)
def test_float32_oracle_is_within_tol_and_every_case_is_in_range(family):
    worst, worst_c = 0.0, 0.0
    for T, lam in [(T, 0.5) for T in FAMILY_T[family]] + ([(8, l) for l in LAMBDAS] if family == "gauss" else []):
        es = family_es(family, T, lam)
        f32 = restated_costs([make_inputs(family, T, E) for E in es], lam, torch.float32)
        for E, (a0, a1, _) in zip(es, f32):
            c = Case(family, T, E, lam)
            cmax = float(torch.maximum(c.c0.abs(), c.c1.abs()).max())
            worst_c = max(worst_c, cmax / lam)
            assert cmax <= 64.0 * lam, (family, T, E, lam, cmax)                  # the range condition
            # element by element, c_dir = the element's own cost: every slice that holds the element has a tol at least this large
            t1 = tol_of(T, E, lam, 1, c.c0.abs())
            t2 = tol_of(T, E, lam, 2, torch.maximum(c.c0.abs(), c.c1.abs()))
            r1 = float(((a0.double() - c.c0).abs() / t1).max())
            r2 = float((((a0.double() + a1.double()) - (c.c0 + c.c1)).abs() / t2).max())
            worst = max(worst, r1, r2)
            assert r1 <= 1.0 and r2 <= 1.0, (family, T, E, lam, r1, r2)
    print("%s: float32 oracle worst err / tol %.3f, largest |cost| / lambda %.1f" % (family, worst, worst_c))


# ---------------------------------------------------------------------------------------------------------------- GPU helpers
def guarded_empty(shape, dtype=torch.float32, fill=NAN):
    """a contiguous device view of `shape` into a larger buffer of `fill`, G elements of it before and behind"""
    n = math.prod(shape)
    buf = torch.full((n + 2 * G,), fill, dtype=dtype, device=DEV)
    return buf[G:G + n].view(shape)


def guarded(t, fill=NAN):
    v = guarded_empty(tuple(t.shape), t.dtype, fill)
    v.copy_(t)
    return v


def norms(x):
    from clip_fsar_amd import gallery_hip as gh
    n = guarded_empty((x.numel() // x.shape[-1],))
    gh.row_norms(x, n)
    return n


class Out:
    """an output view into a buffer of SENT; get() returns it on the CPU after checking that nothing around it was written"""

    def __init__(self, *shape):
        self.shape, self.n = shape, math.prod(shape)
        self.buf = torch.full((self.n + 2 * G,), SENT, device=DEV)
        self.view = self.buf[G:G + self.n].view(shape)

    def get(self):
        b = self.buf.cpu()
        assert bool((b[:G] == SENT).all()) and bool((b[G + self.n:] == SENT).all()), "a store outside the output"
        return b[G:G + self.n].view(self.shape)


def scattered_store(p, pn, seed, spare=3):
    """p [C, T, E], pn [C T] on the device -> (store [cap, T, E], pn_store, slots [C]): the classes at a random subset of the slots of a
    NaN-filled store, in a random order"""
    C, T, E = p.shape
    cap = C + spare
    slots = torch.randperm(cap, generator=torch.Generator().manual_seed(seed))[:C].to(DEV)
    store, pns = guarded_empty((cap, T, E)), guarded_empty((cap * T,))
    store[slots] = p
    pns.view(cap, T)[slots] = pn.view(C, T)
    return store, pns, slots


def check(out, ref, tol, what):
    err = float((out.double() - ref).abs().max())
    assert err <= tol, "%s: err %.3e tol %.3e" % (what, err, tol)          # a NaN fails this too
    return err / tol


def report(kernel, family, T, ratio):
    print("otam-worst %s %s T=%d %.4f" % (kernel, family, T, ratio))


# ---------------------------------------------------------------------------------------------------------------- GPU: the tile kernels
def run_tile(case):
    """dense and indexed kernel of one Case at the five (NQ, C) of its T, both single_direct values: asserts the logits -> (worst logit
    err / tol, worst dists_out err / e_d); dists_out is asserted within e_d"""
    from clip_fsar_amd import gallery_hip as gh
    from clip_fsar_amd import live_hip as lh
    T, E, lam = case.T, case.E, case.lam
    pending = []
    for n, c in tile_shapes(T):
        xq, p = guarded(case.Xq[:n]), guarded(case.P[:c])
        qn, pn = norms(xq), norms(p)
        store, pns, slots = scattered_store(p, pn, seed=7 * n + c)
        cols = guarded(slots.int(), fill=BAD_SLOT)
        ident = guarded(torch.arange(c, dtype=torch.int32), fill=BAD_SLOT)
        twice = guarded(torch.cat([slots, slots[:1]]).int(), fill=BAD_SLOT)     # the first slot again, as a further column
        for sd in (False, True):
            lg, dd = Out(n, c), (None if sd else Out(n, c, T, T))
            gh.otam_gallery(xq, qn, p, pn, lg.view, lam, sd, dists_out=None if sd else dd.view)
            li, l1, l2 = Out(n, c), Out(n, c), Out(n, c + 1)
            lh.otam_indexed(xq, qn, store, pns, cols, li.view, lam, sd)
            lh.otam_indexed(xq, qn, p, pn, ident, l1.view, lam, sd)
            lh.otam_indexed(xq, qn, store, pns, twice, l2.view, lam, sd)
            pending.append((n, c, sd, lg, dd, li, l1, l2))
    torch.cuda.synchronize()
    worst, worst_d = 0.0, 0.0
    for n, c, sd, lg, dd, li, l1, l2 in pending:
        what = "%s T %d E %d lambda %g NQ %d C %d single_direct %d" % (case.family, T, E, lam, n, c, sd)
        ref, c_dir = case.ref(slice(0, n), slice(0, c), sd)
        assert c_dir <= 64.0 * lam, (what, c_dir)
        dense = lg.get()
        worst = max(worst, check(dense, ref, tol_of(T, E, lam, 1 if sd else 2, c_dir), what))
        if dd is not None:
            worst_d = max(worst_d, check(dd.get(), case.d[:n, :c], e_d_of(E), what + " dists_out"))
        assert torch.equal(li.get(), dense), what + ": indexed (scattered store) != dense"
        assert torch.equal(l1.get(), dense), what + ": indexed (identity) != dense"
        tw = l2.get()
        assert torch.equal(tw[:, :c], dense) and torch.equal(tw[:, c], tw[:, 0]), what + ": a slot named twice"
    return worst, worst_d


@gpu
@pytest.mark.parametrize("family,T", FAMILY_CASES)
def test_tile_kernels_vs_float64(family, T):
    for E in tile_es(family, T):
        r, rd = run_tile(Case(family, T, E))
        print("tile %s T %d E %d: worst err / tol %.4f, dists_out err / e_d %.4f" % (family, T, E, r, rd))
        report("dense", family, T, r)


@gpu
@pytest.mark.parametrize("lam", LAMBDAS)
def test_tile_kernels_other_lambda(lam):
    report("dense", "gauss", 8, run_tile(Case("gauss", 8, 512, lam))[0])


@gpu
@pytest.mark.parametrize("T", EDGE_T)
def test_tile_output_does_not_depend_on_its_place_in_a_tile(T):
    from clip_fsar_amd import gallery_hip as gh
    from clip_fsar_amd import live_hip as lh
    qb = tile_videos(T)
    n, c = 2 * qb + 1, qb + 2
    for E in (512, 36):
        case = Case("gauss", T, E)
        xq, p = guarded(case.Xq[:n]), guarded(case.P[:c])
        qn, pn = norms(xq), norms(p)
        store, pns, slots = scattered_store(p, pn, seed=T)
        cols = guarded(slots.int(), fill=BAD_SLOT)
        picks = sorted({(0, 0), (qb - 1, qb - 1), (qb, qb), (2 * qb, qb + 1), (1, qb), (qb, 0)})
        for sd in (False, True):
            full, fulli = Out(n, c), Out(n, c)
            gh.otam_gallery(xq, qn, p, pn, full.view, 0.5, sd)
            lh.otam_indexed(xq, qn, store, pns, cols, fulli.view, 0.5, sd)
            ones = []
            for q, k in picks:
                x1, p1 = guarded(case.Xq[q:q + 1]), guarded(case.P[k:k + 1])
                q1, n1 = guarded(qn[q * T:(q + 1) * T]), guarded(pn[k * T:(k + 1) * T])
                o, oi = Out(1, 1), Out(1, 1)
                gh.otam_gallery(x1, q1, p1, n1, o.view, 0.5, sd)
                lh.otam_indexed(x1, q1, store, pns, guarded(slots[k:k + 1].int(), fill=BAD_SLOT), oi.view, 0.5, sd)
                ones.append((q, k, o, oi))
            torch.cuda.synchronize()
            f, fi = full.get(), fulli.get()
            assert torch.equal(f, fi)
            for q, k, o, oi in ones:
                assert torch.equal(o.get()[0, 0], f[q, k]), (T, E, sd, q, k, "dense")
                assert torch.equal(oi.get()[0, 0], f[q, k]), (T, E, sd, q, k, "indexed")


@gpu
@pytest.mark.parametrize("T", [5, 16, 32])
def test_indexed_kernel_poisons_exactly_the_bad_column(T):
    from clip_fsar_amd import live_hip as lh
    qb = tile_videos(T)
    n, c = 2 * qb + 1, qb + 2
    case = Case("gauss", T, 512)
    xq, p = guarded(case.Xq[:n]), guarded(case.P[:c])
    qn, pn = norms(xq), norms(p)
    store, pns, slots = scattered_store(p, pn, seed=T + 1)
    cap = store.shape[0]
    for sd in (False, True):
        clean = Out(n, c)
        lh.otam_indexed(xq, qn, store, pns, guarded(slots.int(), fill=BAD_SLOT), clean.view, 0.5, sd)
        runs = []
        for col in sorted({0, qb - 1, qb, c - 1}):
            for bad in (-1, cap, BAD_SLOT):
                s = slots.int().clone()
                s[col] = bad
                o = Out(n, c)
                lh.otam_indexed(xq, qn, store, pns, guarded(s, fill=BAD_SLOT), o.view, 0.5, sd)
                runs.append((col, bad, o))
        torch.cuda.synchronize()
        ok = clean.get()
        assert bool(torch.isfinite(ok).all())
        for col, bad, o in runs:
            got = o.get()
            keep = [j for j in range(c) if j != col]
            assert bool(torch.isnan(got[:, col]).all()), (T, sd, col, bad)
            assert torch.equal(got[:, keep], ok[:, keep]), (T, sd, col, bad)


@gpu
def test_dense_kernel_writes_the_bits_of_the_chunked_tile_gemm():
    """tests/golden/otam_tile_bits.npz (tools/otam_tile_bits.py): what cfsg_otam_gallery wrote on an MI355X at three product shapes once
    fp32_tile_gemm.h summed every K chunk from zero.  That fix changed the last bits of every shipped configuration with E > 32; from here
    on they are pinned (the indexed kernel through its bit equality with the dense one, above and in tests/test_gpu_live.py)."""
    import json
    import os

    import numpy as np

    import clip_fsar_amd.synth as synth
    from clip_fsar_amd import gallery_hip as gh
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "otam_tile_bits.npz"))
    meta = json.loads(str(z["meta"]))
    assert sorted(meta["cases"]) == ["T16_E768", "T8_E1024", "T8_E512"]
    for name, c in meta["cases"].items():
        base = synth.pseudo_normal(c["E"], "otam_bits/base/" + name, meta["seed"])
        ops = []
        for side, n in (("q", c["NQ"]), ("p", c["C"])):
            x = synth.pseudo_normal(n * c["T"] * c["E"], "otam_bits/%s/%s" % (side, name), meta["seed"]).reshape(n, c["T"], c["E"])
            scale = 0.5 + 0.25 * np.abs(synth.pseudo_normal(n * c["T"], "otam_bits/%s_scale/%s" % (side, name), meta["seed"]))
            ops.append(guarded(torch.from_numpy(((base + 1.2 * x) * scale.reshape(n, c["T"], 1)).astype(np.float32))))
        xq, p = ops
        qn, pn = norms(xq), norms(p)
        for sd in (0, 1):
            lg, dd = Out(c["NQ"], c["C"]), Out(c["NQ"], c["C"], c["T"], c["T"])
            gh.otam_gallery(xq, qn, p, pn, lg.view, 0.5, bool(sd), dists_out=dd.view)
            torch.cuda.synchronize()
            want = torch.from_numpy(z["%s/logits_sd%d" % (name, sd)])
            got = lg.get()
            assert torch.equal(got, want), (name, sd, float((got - want).abs().max()))
            if not sd:
                assert torch.equal(dd.get(), torch.from_numpy(z[name + "/dists"])), name


# ---------------------------------------------------------------------------------------------------------------- GPU: the episode kernel
def run_episode(case):
    """cos_otam_kernel on one Case at every (B, Q, way) and both single_direct values, against float64 and the dense kernel: asserts the
    logits and dists_out (within e_d) -> (worst logit err / tol, worst dists_out err / e_d)"""
    from clip_fsar_amd import gallery_hip as gh
    from clip_fsar_amd import hip
    T, E, lam = case.T, case.E, case.lam
    NQ, C = 12, 21
    xq_all, p_all = guarded(case.Xq[:NQ]), guarded(case.P[:C])
    qn, pn = norms(xq_all), norms(p_all)
    dense = {}
    for sd in (False, True):
        dense[sd] = Out(NQ, C)
        gh.otam_gallery(xq_all, qn, p_all, pn, dense[sd].view, lam, sd)
    pending = []
    for B, Q, way in EP_COMBOS:
        xq, p = guarded(case.Xq[:B * Q].reshape(B, Q, T, E)), guarded(case.P[:B * way].reshape(B, way, T, E))
        for sd in (False, True):
            lg = Out(B, Q, way)
            dd = Out(B, Q, way, T, T) if (not sd and (B, Q, way) in ((1, 1, 1), (3, 1, 5), (3, 4, 7))) else None
            hip.cos_otam_logits(xq, p, lg.view, B, Q, way, T, E, lam, sd, dists_out=None if dd is None else dd.view)
            pending.append((B, Q, way, sd, lg, dd))
    torch.cuda.synchronize()
    dense = {sd: o.get().double() for sd, o in dense.items()}
    worst, worst_d = 0.0, 0.0
    for B, Q, way, sd, lg, dd in pending:
        what = "%s T %d E %d lambda %g B %d Q %d way %d single_direct %d" % (case.family, T, E, lam, B, Q, way, sd)
        got = lg.get()
        for b in range(B):
            rows, cols = slice(b * Q, (b + 1) * Q), slice(b * way, (b + 1) * way)
            ref, c_dir = case.ref(rows, cols, sd)
            assert c_dir <= 64.0 * lam, (what, c_dir)
            tol = tol_of(T, E, lam, 1 if sd else 2, c_dir)
            worst = max(worst, check(got[b], ref, tol, what))
            check(got[b], dense[sd][rows, cols], tol, what + " vs the dense kernel")
            if T <= 16 and case.family == "gauss" and lam == 0.5:
                check(got[b], dense[sd][rows, cols], BOUND, what + " vs the dense kernel (BOUND)")
            if dd is not None:
                worst_d = max(worst_d, check(dd.get()[b], case.d[rows, cols], e_d_of(E), what + " dists_out"))
    return worst, worst_d


@gpu
@pytest.mark.parametrize("family,T", FAMILY_CASES)
def test_episode_kernel_vs_float64_and_dense_kernel(family, T):
    for E in episode_es(T):
        r, rd = run_episode(Case(family, T, E))
        print("episode %s T %d E %d: worst err / tol %.4f, dists_out err / e_d %.4f" % (family, T, E, r, rd))
        report("episode", family, T, r)


@gpu
@pytest.mark.parametrize("lam", LAMBDAS)
def test_episode_kernel_other_lambda(lam):
    report("episode", "gauss", 8, run_episode(Case("gauss", 8, 512, lam))[0])


@gpu
def test_episode_kernel_lds_edge():
    """E = 2048: T = 18 needs 149 424 bytes of LDS and runs, T = 19 needs 157 764 and is refused"""
    from clip_fsar_amd import hip
    assert episode_lds_bytes(18, 2048) == 149424 and episode_lds_bytes(19, 2048) == 157764
    Xq, P = make_inputs("gauss", 18, 2048)
    (c0, c1, _), = restated_costs([(Xq[:2], P[:3])], 0.5)
    lg = Out(1, 2, 3)
    hip.cos_otam_logits(guarded(Xq[:2].unsqueeze(0)), guarded(P[:3].unsqueeze(0)), lg.view, 1, 2, 3, 18, 2048)
    torch.cuda.synchronize()
    c_dir = float(torch.maximum(c0.abs(), c1.abs()).max())
    assert c_dir <= 32.0
    report("episode", "gauss", 18, check(lg.get()[0], -(c0 + c1), tol_of(18, 2048, 0.5, 2, c_dir), "T 18 E 2048"))
    out = Out(1, 1, 1)
    with pytest.raises(RuntimeError, match="cfsar_cos_otam_logits: T\\*E too large for LDS"):
        hip.cos_otam_logits(guarded_empty((1, 1, 19, 2048)), guarded_empty((1, 1, 19, 2048)), out.view, 1, 1, 1, 19, 2048)
    torch.cuda.synchronize()
    assert bool((out.get() == SENT).all())


# ---------------------------------------------------------------------------------------------------------------- GPU: refusals
def _tile_args(NQ=2, C=3, T=4, E=8, cap=5):
    xq, p = guarded_empty((NQ, T, E)), guarded_empty((cap, T, E))
    return dict(xq=xq, qn=guarded_empty((NQ * T,)), p=p, pn=guarded_empty((cap * T,)),
                cols=guarded(torch.arange(C, dtype=torch.int32), fill=BAD_SLOT), NQ=NQ, C=C, T=T, E=E, cap=cap)


def _raw_call(a, which, out, **over):
    """a tile entry point called below its wrapper, with dimensions that the wrapper's tensors cannot express -> (rc, message)"""
    import ctypes
    from clip_fsar_amd import gallery_hip as gh
    from clip_fsar_amd import live_hip as lh
    d = dict(a, **over)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())                                                         # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    if which == "gallery":
        rc = gh.lib().cfsg_otam_gallery(ptr(a["xq"]), ptr(a["qn"]), ptr(a["p"]), ptr(a["pn"]), ptr(out.view), None, d["NQ"], d["C"], d["T"],
                                        d["E"], 0.5, 0, st)
        return rc, gh.lib().cfsg_last_error().decode()
    rc = lh.lib().cfsl_otam_indexed(ptr(a["xq"]), ptr(a["qn"]), ptr(a["p"]), ptr(a["pn"]), ptr(a["cols"]), ptr(out.view), d["NQ"], d["C"],
                                    d["cap"], d["T"], d["E"], 0.5, 0, st)
    return rc, lh.lib().cfsl_last_error().decode()


@gpu
def test_tile_entry_points_refuse_bad_arguments_before_any_launch():
    from clip_fsar_amd import gallery_hip as gh
    from clip_fsar_amd import live_hip as lh
    a = _tile_args()
    out = Out(a["NQ"], a["C"])
    # what no tensor shape can say: T = 0, E = 0, cap = 0
    for which, over in (("gallery", {"T": 0}), ("gallery", {"E": 0}), ("live", {"T": 0}), ("live", {"E": 0}), ("live", {"cap": 0})):
        rc, msg = _raw_call(a, which, out, **over)
        assert rc != 0 and msg.startswith("cfsg_otam_gallery: bad shape" if which == "gallery" else "cfsl_otam_indexed: bad shape"), (over, msg)
    torch.cuda.synchronize()
    assert bool((out.get() == SENT).all())

    def both(T, E, lam, pat_g, pat_l, NQ=2, C=3):
        xq, p = guarded_empty((NQ, T, E)), guarded_empty((C, T, E))
        qn, pn = guarded_empty((NQ * T,)), guarded_empty((C * T,))
        o = Out(NQ, C)
        with pytest.raises(RuntimeError, match=pat_g):
            gh.otam_gallery(xq, qn, p, pn, o.view, lam, False)
        with pytest.raises(RuntimeError, match=pat_l):
            lh.otam_indexed(xq, qn, p, pn, guarded(torch.arange(C, dtype=torch.int32), fill=BAD_SLOT), o.view, lam, False)
        torch.cuda.synchronize()
        assert bool((o.get() == SENT).all())

    both(33, 8, 0.5, "cfsg_otam_gallery: bad shape", "cfsl_otam_indexed: bad shape")
    both(4, 6, 0.5, "cfsg_otam_gallery: bad shape", "cfsl_otam_indexed: bad shape")
    both(1, 8196, 0.5, "cfsg_otam_gallery: bad shape", "cfsl_otam_indexed: bad shape")
    both(4, 8, 0.0, "cfsg_otam_gallery: lambda must be > 0", "cfsl_otam_indexed: lambda must be > 0")
    both(4, 8, -0.5, "cfsg_otam_gallery: lambda must be > 0", "cfsl_otam_indexed: lambda must be > 0")
    NQ = 65535 * tile_videos(32) + 1
    both(32, 4, 0.5, "cfsg_otam_gallery: NQ=%d too large for one launch" % NQ, "cfsl_otam_indexed: NQ=%d too large for one launch" % NQ, NQ=NQ,
         C=1)


@gpu
def test_episode_entry_point_refuses_bad_arguments_before_any_launch():
    from clip_fsar_amd import hip
    xq, p = guarded_empty((1, 1, 33, 2052)), guarded_empty((1, 1, 33, 2052))
    o = Out(1, 1, 1)
    for T, E in ((0, 8), (33, 8), (4, 6), (4, 0), (4, 2052)):
        with pytest.raises(RuntimeError, match="cfsar_cos_otam_logits: bad shape"):
            hip.cos_otam_logits(xq, p, o.view, 1, 1, 1, T, E)
    torch.cuda.synchronize()
    assert bool((o.get() == SENT).all())


@gpu
def test_misaligned_operands_are_refused():
    """a contiguous view that starts one float into its buffer: the kernels would read it as float4"""
    from clip_fsar_amd import gallery_hip as gh
    from clip_fsar_amd import hip
    from clip_fsar_amd import live_hip as lh
    NQ, C, T, E = 2, 3, 4, 8

    def off_by_one(*shape):
        n = math.prod(shape)
        return torch.zeros(n + 8, device=DEV)[1:1 + n].view(shape)

    good_q, good_p = guarded_empty((NQ, T, E)), guarded_empty((C, T, E))
    qn, pn = guarded_empty((NQ * T,)), guarded_empty((C * T,))
    cols = guarded(torch.arange(C, dtype=torch.int32), fill=BAD_SLOT)
    o = Out(NQ, C)
    assert off_by_one(NQ, T, E).data_ptr() % 16 == 4 and off_by_one(NQ, T, E).is_contiguous()
    for xq, p in ((off_by_one(NQ, T, E), good_p), (good_q, off_by_one(C, T, E))):
        with pytest.raises(RuntimeError, match="cfsg_otam_gallery: Xq and P must be 16-byte aligned"):
            gh.otam_gallery(xq, qn, p, pn, o.view, 0.5, False)
        with pytest.raises(RuntimeError, match="cfsl_otam_indexed: Xq and P_store must be 16-byte aligned"):
            lh.otam_indexed(xq, qn, p, pn, cols, o.view, 0.5, False)
    oe = Out(1, NQ, C)
    for xq, p in ((off_by_one(1, NQ, T, E), good_p.view(1, C, T, E)), (good_q.view(1, NQ, T, E), off_by_one(1, C, T, E))):
        with pytest.raises(RuntimeError, match="cfsar_cos_otam_logits: Xq and protos must be 16-byte aligned"):
            hip.cos_otam_logits(xq, p, oe.view, 1, NQ, C, T, E)
    torch.cuda.synchronize()
    assert bool((o.get() == SENT).all()) and bool((oe.get() == SENT).all())


# ---------------------------------------------------------------------------------------------------------------- GPU: row norms, top-k
@gpu
@pytest.mark.parametrize("E", [1, 4, 63, 64, 65, 100, 8192])
def test_row_norms_vs_float64(E):
    """relative bound (E / 64 + 8) 2^-24: a lane-strided fmaf chain of E / 64 positive terms, six shuffle adds and a square root"""
    from clip_fsar_amd import gallery_hip as gh
    for R in (1, 3, 4, 5, 131):
        g = torch.Generator().manual_seed(1000 * R + E)
        X = torch.randn(R, E, generator=g) * 10.0 ** (4.0 * torch.rand(R, 1, generator=g) - 2.0)
        if R >= 3:
            X[R // 2] = 0.0
        n = Out(R)
        gh.row_norms(guarded(X), n.view)
        torch.cuda.synchronize()
        got, ref = n.get().double(), X.double().norm(dim=1)
        bound = (E / 64.0 + 8.0) * 2.0 ** -24 * ref
        assert bool(((got - ref).abs() <= bound).all()), (R, E, float(((got - ref).abs() / ref.clamp_min(1e-300)).max()))
        if R >= 3:
            assert float(got[R // 2]) == 0.0


NO_CLASS = 0x7fffffff


def _topk_reference(row, k):
    """a stable descending sort of the selectable classes (neither NaN nor -inf); the places after them hold (-inf, NO_CLASS)"""
    order = sorted((j for j in range(len(row)) if row[j] > -math.inf), key=lambda j: (-row[j], j))[:k]
    return [row[j] for j in order] + [-math.inf] * (k - len(order)), order + [NO_CLASS] * (k - len(order))


@gpu
@pytest.mark.parametrize("C,k", [(7, 7), (70, 16), (300, 5), (1500, 16)])
def test_topk_on_poisoned_and_infinite_logits(C, k):
    from clip_fsar_amd import gallery_hip as gh
    g = torch.Generator().manual_seed(C)
    lg = torch.randn(8, C, generator=g)
    lg[:, ::3] = torch.randint(0, 3, (8, (C + 2) // 3), generator=g).float() + 2.0           # ties among the largest
    lg[0, torch.rand(C, generator=g) < 0.5] = NAN                                             # every second class poisoned
    lg[1] = NAN                                                                               # nothing selectable: NO_CLASS everywhere
    lg[2] = NAN
    lg[2, [C - 1, 2]] = torch.tensor([0.5, -1.0])                                             # two selectable classes, then NO_CLASS
    lg[3] = -math.inf                                                                         # -inf is not selectable: NO_CLASS everywhere
    lg[4, torch.rand(C, generator=g) < 0.7] = -math.inf                                       # the finite ones, then NO_CLASS
    lg[5] = NAN
    lg[5, [1, C - 2]] = -math.inf                                                             # NO_CLASS everywhere
    lg[6, 0] = NAN
    lg[6, C - 1] = math.inf
    vals, idx = Out(8, k), guarded_empty((8, k), torch.int32, fill=-5)
    gh.topk(guarded(lg), k, vals.view, idx)
    torch.cuda.synchronize()
    v, i = vals.get(), idx.cpu()
    for q in (1, 3, 5):
        assert i[q].tolist() == [NO_CLASS] * k and v[q].tolist() == [-math.inf] * k, q
    for q in range(8):
        rv, ri = _topk_reference(lg[q].tolist(), k)
        assert v[q].tolist() == rv and i[q].tolist() == ri, (C, k, q, i[q].tolist(), ri)
