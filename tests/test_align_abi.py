"""CPU: the OTAM alignment (libclipfsar_align.so, include/ext/clipfsar_align.h, clip_fsar_amd.align_hip, clip_fsar_amd.align.Aligner,
StreamPool.explain) -- the plug-in library's exports, ABI check at load, resource report and place in the build (one more name of the open
registry, build.PLUGIN_LIBS); every host validation of cfal_align without a GPU; reference_alignment against autograd through the
oracle's OTAM_cum_dist, on hand-written cases and at the sizes where the un-stabilised fp32 recurrence breaks down; every argument error of
Aligner and of StreamPool.explain on stub heads.

Measured (run with -s): reference_alignment in float64 against autograd through the oracle, worst |difference| 1.9e-14 (value and plan,
both directions and single, over the case list below); its float32 form against float64: plan 8.8e-6, value 5.1e-6."""
import ctypes
import json
import os
import re
from types import SimpleNamespace as NS

import pytest
import torch

import _abi
from _abi import check_abi_at_load, check_exports

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ext", "clipfsar_align.h")
KERNELS = {"otam_align_kernel": 1}
ROW = _abi._row("align", "align_hip", "cfal_", "ext/clipfsar_align.h", "version abi_version last_error align", KERNELS, 1)
ALL_T = [1, 2, 3, 7, 8, 9, 16, 31, 32]
LAMBDAS = [0.25, 0.5, 1.0]
FAMILIES = ["gauss", "near", "far"]
E_REF = 36


# ------------------------------------------------------------------ inputs (test_gpu_align.py builds its cases from these too)
def rows_of(family, n, c, T, E, seed):
    """(Xq [n, T, E], P [c, T, E]) fp32.  gauss: independent random rows with a per-row scale spread (d around 1 everywhere: a path
    costs about T, where exp(-c / lambda) has left the fp32 range); near: the prototypes' rows are the base rows, the queries near-copies
    of them (d around 0.01 on the diagonal, where the + 0.01 of the cosine's denominator matters, and around 1 off it); far: the queries
    near the opposite of the base rows (d around 2 on the diagonal: the largest costs)"""
    g = torch.Generator().manual_seed(seed)
    if family == "gauss":
        Xq = torch.randn(n, T, E, generator=g) * (0.5 + torch.rand(n, T, 1, generator=g))
        P = torch.randn(c, T, E, generator=g) * (0.5 + torch.rand(c, T, 1, generator=g))
    elif family in ("near", "far"):
        base = torch.randn(T, E, generator=g)
        sign = 1.0 if family == "near" else -1.0
        Xq = sign * base + 0.05 * torch.randn(n, T, E, generator=g)
        P = base + 0.05 * torch.randn(c, T, E, generator=g)
    else:
        raise ValueError(family)
    return Xq.float().contiguous(), P.float().contiguous()


def dists_of(Xq, qn, P, pn):
    """float64 D [n, c, T, T] of the fp32 rows and the fp32 norms given: 1 - dot / (qn * pn + 0.01)"""
    n, T, E = Xq.shape
    c = P.shape[0]
    dot = Xq.double().reshape(n * T, E) @ P.double().reshape(c * T, E).T
    den = qn.double().reshape(n * T, 1) * pn.double().reshape(1, c * T) + 0.01
    return (1.0 - dot / den).reshape(n, T, c, T).permute(0, 2, 1, 3).contiguous()


def norms_of(X):
    return torch.linalg.vector_norm(X.double(), dim=-1).float().reshape(-1)


def case_dists(family, T, E=E_REF, n=2, c=2):
    Xq, P = rows_of(family, n, c, T, E, 1009 * FAMILIES.index(family) + 31 * T + E)
    return dists_of(Xq, norms_of(Xq), P, norms_of(P)).reshape(n * c, T, T)


@pytest.fixture(scope="module")
def clib():
    import __graft_entry__ as ge
    ge.build()                                    # builds every library (no-op when up to date)
    from clip_fsar_amd import align_hip
    return align_hip.lib()


# ------------------------------------------------------------------ the library and its place in the build
def test_header_exported_exactly_and_arity_matches(clib):
    check_exports(ROW)
    assert ROW.exports == {"cfal_" + e for e in ("version", "abi_version", "last_error", "align")}
    from clip_fsar_amd import align_hip as ah
    from clip_fsar_amd import live_hip
    text = open(HEADER).read()
    for name in ("MAX_T", "MIN_E", "MAX_E"):
        assert int(re.search(r"#define CFAL_%s (\d+)" % name, text).group(1)) == getattr(ah, name), name
    assert ah.MAX_T == live_hip.MAX_T == 32 and (ah.MIN_E, ah.MAX_E) == (4, 8192)
    assert len(ah.SIGNATURES["cfal_align"]) == 17 and ah.SIGNATURES["cfal_align"][11] is ctypes.c_float
    for other in _abi.LIBS:                       # its prefix hides no other library's, and none hides it
        assert not other.prefix.startswith(ROW.prefix) and not ROW.prefix.startswith(other.prefix), other.name
    for prefix in ("cfcs_", "cfev_", "cfbl_", "cfsh_", "cfps_"):
        assert not prefix.startswith(ROW.prefix) and not ROW.prefix.startswith(prefix)


def test_abi_version_is_checked_at_load(clib, monkeypatch):
    check_abi_at_load(ROW, monkeypatch)


def test_the_kernel_is_the_listed_one_and_uses_no_scratch(clib):
    from clip_fsar_amd import align_hip as ah
    from clip_fsar_amd import build as b
    pl = b.PLUGIN_LIBS["align"]
    if not os.path.exists(pl.usage):
        b.build_plugin("align", force=True, verbose=False)
    usage = json.load(open(pl.usage))
    assert len(usage) == ROW.total == sum(KERNELS.values()), sorted(usage)
    for fragment, count in KERNELS.items():
        assert sum(fragment in n for n in usage) == count, (fragment, sorted(usage))
    for n, u in usage.items():
        assert u.get("scratch", 0) == 0 and u.get("spills", 0) == 0, (n, u)
    assert pl.lib == ah.LIB_PATH and pl.lib.endswith(os.sep + "libclipfsar_align.so") and os.path.exists(pl.lib)
    others = [b.USAGE] + [x.usage for reg in (b.SIDE_LIBS, b.EXT_LIBS, b.ADDON_LIBS) for x in reg.values()]
    others += [x.usage for n, x in b.PLUGIN_LIBS.items() if n != "align"]
    for path in others:                           # no other library's report names it, and it carries no other library's fragment
        if os.path.exists(path):
            assert not any(fragment in n for n in json.load(open(path)) for fragment in KERNELS), path
    import test_baseline_abi, test_events_abi, test_pool_select_abi, test_shortlist_abi
    claimed = [f for row in _abi.SIDE for f in row.kernels]
    claimed += [f for mod in (test_baseline_abi, test_events_abi, test_pool_select_abi, test_shortlist_abi) for f in mod.KERNELS]
    for n in usage:
        assert not any(f in n for f in claimed), n
    # the conventions: the shared error plumbing and nothing else of csrc/ or ext/ (the recurrence is restated: it is another one);
    # plain C++, no allocation, no stream of its own, no loop that could wait on anything
    source = open(pl.source).read()
    assert re.findall(r'^#include "([^"]+)"', source, flags=re.M) == ["../csrc/side_lib.h", "../../include/ext/clipfsar_align.h"]
    for body in ("asm", "atomic", "malloc", "hipMalloc", "hipStreamCreate", "hipMemcpy", "hipDeviceSynchronize", "while"):
        assert body not in source, body
    assert "contract(off)" in source and "__shared__" in source
    size = {"MAX_T": 32, "CW": 34}
    lds = 0
    for n, dim in re.findall(r"__shared__ float \w+(?:\[(\d+)\])?\[([^\]]+)\];", source):
        floats = int(n or 1)
        for factor in dim.split("*"):
            floats *= size.get(factor.strip()) or int(factor)
        lds += 4 * floats
    assert 20 * 1024 < lds < 64 * 1024, lds        # static LDS at any T: D, the two grids, the adjoint rows, the two gradients


def test_align_is_a_name_of_the_open_registry_and_follows_the_recipe():
    from clip_fsar_amd import build as b
    assert "align" in b.PLUGIN_LIBS and "align" in b.plugin_lib_names()
    assert all("align" not in reg for reg in (b.SIDE_LIBS, b.EXT_LIBS, b.ADDON_LIBS))
    pl = b.PLUGIN_LIBS["align"]
    assert isinstance(pl, b.ExtLib)
    assert pl.source == os.path.join(b.EXT, "align.hip") and os.path.exists(pl.source)
    assert pl.header == HEADER and os.path.exists(pl.header)
    assert pl.lib == os.path.join(b.HERE, "libclipfsar_align.so")
    assert pl.usage == os.path.join(b.HERE, "build", "align", "resource_usage.json")
    deps = b._plugin_deps("align")
    assert sorted(deps) == sorted([pl.source, pl.header, os.path.abspath(b.__file__), os.path.join(b.CSRC, "side_lib.h"),
                                   os.path.join(b.CSRC, "common.h"), os.path.join(ROOT, "include", "clipfsar_hip.h")])
    for call in (b.build_side, b._side_deps, b.build_ext, b._ext_deps, b.build_addon, b._addon_deps):       # the three closed registries
        with pytest.raises(KeyError):
            call("align")
    assert not os.path.exists(os.path.join(b.CSRC, "align.hip"))
    assert not any("clipfsar_align" in open(os.path.join(b.CSRC, f)).read() for f in os.listdir(b.CSRC))     # nothing of csrc/ knows it


def test_staleness_of_the_align_library_and_of_no_other(monkeypatch):
    from clip_fsar_amd import build as b
    from test_build_recipe import NAMES, STALE, P
    monkeypatch.setattr(b.os.path, "exists", lambda p: True)

    def stale_after(edited):
        monkeypatch.setattr(b.os.path, "getmtime", lambda p: 2.0 if p.endswith(os.sep + edited) else 1.0)
        old = {P} if b._stale(b.LIB, b._product_deps()) else set()
        old |= {n for n in NAMES if b._stale(b.SIDE_LIBS[n].lib, b._side_deps(n))}
        old |= {n for n in b.EXT_LIBS if b._stale(b.EXT_LIBS[n].lib, b._ext_deps(n))}
        old |= {n for n in b.ADDON_LIBS if b._stale(b.ADDON_LIBS[n].lib, b._addon_deps(n))}
        return old, {n for n in b.PLUGIN_LIBS if b._stale(b.PLUGIN_LIBS[n].lib, b._plugin_deps(n))}

    for edited in ("align.hip", "clipfsar_align.h"):                              # its own files: it alone
        assert stale_after(edited) == (set(), {"align"}), edited
    for edited in ("side_lib.h", "build.py", "common.h"):                         # what every library reaches
        old, plugins = stale_after(edited)
        assert STALE[edited] <= old and plugins == set(b.PLUGIN_LIBS), edited
    for edited in ("otam_dp.h", "otam_tile.h", "fp32_tile_gemm.h", "select_keys.h", "chunk_row.h", "ring_rows.h", "shortlist.hip",
                   "pool_select.hip", "baseline.hip", "live.hip", "groups.hip", "gallery.hip", "gemm.hip"):
        assert "align" not in stale_after(edited)[1], edited
    assert stale_after("no_such_file.h") == (set(), set())


# ------------------------------------------------------------------ validation, without a GPU
def test_align_validation_without_gpu(clib):
    p = ctypes.c_void_p(4096)                     # never dereferenced: every call below fails validation before any device work
    err = clib.cfal_last_error

    # align(Xq, qn, P, pn, pair_q, pair_slot, NP, NQ, cap, T, E, lambda, single_direct, plan, dists, logits, stream)
    def call(NP=3, NQ=5, cap=7, T=8, E=512, lam=0.5, sd=0, ptrs=None):
        a = ptrs or [p] * 9
        return clib.cfal_align(*a[:6], NP, NQ, cap, T, E, lam, sd, *a[6:], None)

    for i in (0, 1, 2, 3, 4, 5, 6, 8):            # dists (7) alone may be null
        ptrs = [p] * 9
        ptrs[i] = None
        assert call(ptrs=ptrs) != 0 and b"null pointer" in err(), i
    for NP in (0, -1):
        assert call(NP=NP) != 0 and b"NP=" in err(), NP
    for NQ in (0, -5):
        assert call(NQ=NQ) != 0 and b"NQ=" in err(), NQ
    for cap in (0, -7):
        assert call(cap=cap) != 0 and b"cap=" in err(), cap
    for T in (0, -1, 33):
        assert call(T=T) != 0 and b"T=%d outside 1 .. 32" % T in err(), T
    for E in (0, 2, 3, 6, 510, 8196, -4):
        assert call(E=E) != 0 and b"E=%d" % E in err(), E
    assert call(NP=1 << 21, T=32) != 0 and b"NP * T * T" in err()                 # 2^31 plan cells
    assert call(NQ=1 << 26, T=32) != 0 and b"NQ * T" in err()
    assert call(cap=1 << 26, T=32) != 0 and b"cap * T" in err()
    for lam in (0.0, -0.5, float("inf"), float("nan")):
        assert call(lam=lam) != 0 and b"lambda=" in err(), lam
    for sd in (2, -1):
        assert call(sd=sd) != 0 and b"single_direct=%d" % sd in err(), sd
    for i, word in ((0, b"Xq 0x1008"), (2, b"P 0x1008")):                          # 16-byte alignment of the two row arrays
        ptrs = [p] * 9
        ptrs[i] = ctypes.c_void_p(4096 + 8)
        assert call(ptrs=ptrs) != 0 and b"16-byte aligned" in err() and word in err(), i


def test_python_wrapper_rejects_cpu_tensors_and_bad_shapes(clib):
    from clip_fsar_amd import align_hip as ah
    i32 = dict(dtype=torch.int32)
    NQ, cap, T, E, NP = 2, 3, 4, 8, 5
    args = lambda: [torch.zeros(NQ, T, E), torch.zeros(NQ * T), torch.zeros(cap, T, E), torch.zeros(cap * T), torch.zeros(NP, **i32),
                    torch.zeros(NP, **i32), 0.5, False, torch.zeros(NP, T, T), torch.zeros(NP, T, T), torch.zeros(NP)]
    with pytest.raises(RuntimeError, match="HIP device tensor"):
        ah.align(*args())
    for i, t in ((1, torch.zeros(NQ * T + 1)), (2, torch.zeros(cap, T, E + 4)), (3, torch.zeros(cap)), (5, torch.zeros(NP + 1, **i32)),
                 (8, torch.zeros(NP, T, T + 1)), (9, torch.zeros(NP - 1, T, T)), (10, torch.zeros(NP, 1))):
        a = args()
        a[i] = t
        with pytest.raises(RuntimeError, match="shape"):
            ah.align(*a)


# ------------------------------------------------------------------ reference_alignment
def _autograd(D, lam, single_direct):
    """(value, plan) in float64 by autograd through the oracle's recurrence"""
    import clipfsar_oracle as orc
    d = D.double().clone().requires_grad_(True)
    value = orc.otam_cum_dist(d[None], lam)[0]
    if not single_direct:
        value = value + orc.otam_cum_dist(d[None].transpose(-1, -2), lam)[0]
    plan, = torch.autograd.grad(value.sum(), d)
    return value.detach(), plan


@pytest.mark.parametrize("family", FAMILIES)
def test_reference_alignment_in_float64_is_autograd_through_the_oracle(family):
    from clip_fsar_amd.align import reference_alignment
    worst = 0.0
    for T in ALL_T:
        D = case_dists(family, T)
        for lam in LAMBDAS:
            for sd in (False, True):
                want_v, want_p = _autograd(D, lam, sd)
                value, plan = reference_alignment(D, lam, single_direct=sd)
                assert value.dtype == plan.dtype == torch.float64 and tuple(plan.shape) == tuple(D.shape)
                err = max(float((value - want_v).abs().max()), float((plan - want_p).abs().max()))
                worst = max(worst, err)
                assert err <= 1e-12, (family, T, lam, sd, err)
                assert float(plan.min()) >= 0.0 and float(plan.max()) <= (1.0 if sd else 2.0) + 1e-12
    print("%s: reference_alignment (float64) against autograd through the oracle, worst |difference| %.2e" % (family, worst))


def test_reference_alignment_hand_cases():
    from clip_fsar_amd.align import reference_alignment
    for D in ([[0.3]], [[7.0]]):                                                  # T = 1: F = d, whatever lambda
        value, plan = reference_alignment(D, 0.5)
        assert plan.tolist() == [[2.0]] and float(value) == 2 * D[0][0]
        value, plan = reference_alignment(D, 0.25, single_direct=True)
        assert plan.tolist() == [[1.0]] and float(value) == D[0][0]
    # D = 0 everywhere: lambda drops out, the weights are ratios of path counts, and both directions are one by symmetry
    for T in (2, 5):
        for lam in LAMBDAS:
            value, plan = reference_alignment(torch.zeros(T, T), lam)
            single = reference_alignment(torch.zeros(T, T), lam, single_direct=True)[1]
            assert torch.allclose(plan, single + single.T, atol=1e-15) and float(plan.min()) >= 0.0
            assert torch.allclose(single, reference_alignment(torch.zeros(T, T), 0.5, single_direct=True)[1], atol=1e-14)
    # T = 2 by hand.  exp(-c / lambda) of the padded grid: row 0 all 1; row 1: 1, 3, 4, 6.  The last cell (1, 3) hands 1/6 to (0, 2),
    # 1/6 to (0, 3) and 4/6 to (1, 2); (1, 2) hands 1/4 of its 2/3 to (0, 1) and 3/4 to (1, 1); (1, 1) hands 1/3 of its 1/2 to (0, 1) --
    # the other two thirds flow into the padding and are dropped.  a[0] = (., 1/3, 1/6, 1/6), and row 0 is a running sum.
    value, single = reference_alignment(torch.zeros(2, 2), 0.5, single_direct=True)
    assert torch.allclose(single, torch.tensor([[2.0 / 3.0, 1.0 / 3.0], [1.0 / 2.0, 2.0 / 3.0]], dtype=torch.float64), atol=1e-15), single
    assert abs(float(value) + 0.5 * torch.log(torch.tensor(6.0, dtype=torch.float64)).item()) < 1e-15
    # a batch is its members
    D = case_dists("gauss", 7)
    value, plan = reference_alignment(D, 0.5)
    for i in range(D.shape[0]):
        v, p = reference_alignment(D[i], 0.5)
        assert torch.equal(v, value[i]) and torch.equal(p, plan[i])
    for bad in (torch.zeros(3), torch.zeros(2, 3), torch.zeros(0, 0)):
        with pytest.raises(ValueError, match=r"D must be \[\.\.\., T, T\]"):
            reference_alignment(bad, 0.5)
    with pytest.raises(ValueError, match="lambda must be positive"):
        reference_alignment(torch.zeros(2, 2), 0.0)


@pytest.mark.parametrize("T", [8, 16, 32])
def test_a_prototype_equal_to_the_query_aligns_on_the_diagonal(T):
    """Independent random rows: d is about 0 on the diagonal and about 1 off it.  At lambda 0.25 and 0.5 (the gallery's) a step off the
    diagonal costs two to four lambda and the diagonal holds every row's largest entry.  lambda = 1 is left out on purpose: there the
    soft-min weighs the number of paths as much as their cost, and a path may enter any row for free from the padding column, so the first
    rows' mass leaks to column 0 once T gives those entries enough paths (seen at T = 16 and 32) -- a property of the soft alignment,
    not of its restatement."""
    from clip_fsar_amd.align import reference_alignment
    X = torch.randn(1, T, E_REF, generator=torch.Generator().manual_seed(T)).float()
    D = dists_of(X, norms_of(X), X, norms_of(X))[0, 0]
    for lam in (0.25, 0.5):
        for sd in (False, True):
            _, plan = reference_alignment(D, lam, single_direct=sd)
            assert plan.argmax(dim=1).tolist() == list(range(T)), (T, lam, sd)


def _unstabilised_float32(D, lam):
    """csrc/otam_dp.h's recurrence, every step in float32: -lambda * log(sum exp(-c / lambda)) -> (F, dF/dD by autograd)"""
    import clipfsar_oracle as orc
    d = D.float().clone().requires_grad_(True)
    value = orc.otam_cum_dist(d[None], lam)[0]
    plan, = torch.autograd.grad(value.sum(), d)
    return value.detach(), plan


@pytest.mark.parametrize("family", FAMILIES)
def test_float32_is_finite_where_the_unstabilised_recurrence_is_not(family):
    from clip_fsar_amd.align import reference_alignment
    D = case_dists(family, 32)
    value, plan = reference_alignment(D, 0.25, dtype=torch.float32)
    assert value.dtype == plan.dtype == torch.float32
    assert bool(torch.isfinite(value).all()) and bool(torch.isfinite(plan).all())
    ref_v, ref_p = reference_alignment(D, 0.25)
    print("%s T 32 lambda 0.25: float32 restatement against float64: plan %.2e, value %.2e" % (
        family, float((plan.double() - ref_p).abs().max()), float((value.double() - ref_v).abs().max())))
    v0, p0 = _unstabilised_float32(D, 0.25)
    assert not (bool(torch.isfinite(v0).all()) and bool(torch.isfinite(p0).all())), family     # the reason for the stabilisation


def test_float32_restatement_is_finite_and_close_at_every_size():
    from clip_fsar_amd.align import reference_alignment
    worst_p = worst_v = 0.0
    for family in FAMILIES:
        for T in ALL_T:
            D = case_dists(family, T)
            for lam in LAMBDAS:
                value, plan = reference_alignment(D, lam, dtype=torch.float32)
                assert bool(torch.isfinite(value).all()) and bool(torch.isfinite(plan).all()), (family, T, lam)
                ref_v, ref_p = reference_alignment(D, lam)
                worst_p = max(worst_p, float((plan.double() - ref_p).abs().max()))
                worst_v = max(worst_v, float((value.double() - ref_v).abs().max()))
    print("float32 restatement against float64: plan %.2e, value %.2e" % (worst_p, worst_v))
    assert worst_p < 5e-5 and worst_v < 5e-5      # fp32 rounding over at most 33 * 32 cells of cost <= 2 * 33, not a loss of the result


# ------------------------------------------------------------------ the Python surface, on stub heads
def _stub_head(T=4, **train):
    engine = NS(arch={"embed": 8})
    return NS(args=NS(TRAIN=NS(**train), DATA=NS(NUM_INPUT_FRAMES=T)), _get_engine=lambda dev: engine, _engine_key=("stub",),
              arch_name="stub", precision="fp32", depth=1)


def _live(capacity=4, ids=(0, 1, 2), T=4):
    from clip_fsar_amd import live_gallery as lg
    g = lg.LiveGallery(_stub_head(T), "cpu", capacity=capacity)
    if ids:
        g._install(lg.plan_add(g._book, list(ids)).book)       # registered on the host alone: nothing below reaches the device
    return g


def test_aligner_refusals_are_raised_before_the_device_is_touched():
    from clip_fsar_amd.align import Aligner
    from clip_fsar_amd.gallery import SupportGallery
    from clip_fsar_amd.live_text_gallery import LiveTextGallery
    g = _live()
    al = Aligner(g)
    assert al.gallery is g
    text = LiveTextGallery.__new__(LiveTextGallery)
    with pytest.raises(ValueError, match="Aligner: a LiveTextGallery is refused"):
        Aligner(text)
    for bad in (SupportGallery.__new__(SupportGallery), "gallery", None):
        with pytest.raises(TypeError, match="Aligner: needs a LiveGallery"):
            Aligner(bad)
    feats = torch.zeros(2, 4, 8)
    for kw in ({}, {"classes": [0], "k": 1}):
        with pytest.raises(ValueError, match="Aligner: give exactly one of classes= and k="):
            al.align_features(feats, **kw)
    for k in (0, 4, 17, True, 2.0, "2"):                                           # three classes: k in [1, 3]
        with pytest.raises(ValueError, match=r"Aligner: k must be in \[1, min\(16, number of classes = 3\)\]"):
            al.align_features(feats, k=k)
    with pytest.raises(ValueError, match=r"Aligner: class 9 is not registered \(classes=\)"):
        al.align_features(feats, classes=[0, 9])
    with pytest.raises(ValueError, match="Aligner: a class appears twice in classes="):
        al.align_features(feats, classes=[1, 1])
    with pytest.raises(ValueError, match="Aligner: classes= needs at least one class"):
        al.align_features(feats, classes=[])
    with pytest.raises(ValueError, match="Aligner: 3 class lists for 2 clips"):
        al.align_features(feats, classes=[[0], [1], [2]])
    with pytest.raises(ValueError, match=r"Aligner: clip 1: class 7 is not registered"):
        al.align_features(feats, classes=[[0], [7]])
    with pytest.raises(ValueError, match="Aligner: clip 0: a class appears twice"):
        al.align_features(feats, classes=[[2, 2], []])
    with pytest.raises(ValueError, match="every clip's class list is empty"):
        al.align_features(feats, classes=[[], []])
    for ok in ({"classes": [2, 0]}, {"classes": [[1], []]}, {"classes": ((0, 1), ())}, {"k": 3}):      # past the arguments: the device
        with pytest.raises(RuntimeError, match="feats must be a HIP device tensor"):
            al.align_features(feats, **ok)
    for bad in (None, [[0.0]], torch.zeros(2, 4)):
        with pytest.raises(RuntimeError, match="feats must be a HIP device tensor"):
            al.align_features(bad, classes=[0])
    with pytest.raises(RuntimeError, match="queries must be a HIP device tensor"):
        al.align(torch.zeros(2, 4, 3, 8, 8), k=1)
    with pytest.raises(ValueError, match="Aligner: give exactly one"):
        al.align(torch.zeros(2, 4, 3, 8, 8))
    with pytest.raises(RuntimeError, match="Aligner: no classes registered"):
        Aligner(_live(ids=())).align_features(feats, k=1)
    # the plan of a call, on the host: pairs clip-major, columns into the clip's own list, the slots behind them
    p = al._plan(3, [[2, 0], [], [1]], None)
    assert (p.pair_q, p.column, p.slot, p.offsets) == ([0, 0, 2], [0, 1, 0], [g.slot_of(2), g.slot_of(0), g.slot_of(1)], [0, 2, 2, 3])
    p = al._plan(2, [1, 2], None)
    assert (p.pair_q, p.column, p.slot, p.offsets) == ([0, 0, 1, 1], [0, 1, 0, 1], [g.slot_of(1), g.slot_of(2)] * 2, [0, 2, 4])
    p = al._plan(2, None, 3)
    assert (p.k, p.offsets, p.ids) == (3, [0, 3, 6], [0, 1, 2])
    assert g._store is None


def test_alignment_views():
    from clip_fsar_amd.align import NONE, Alignment
    plan = torch.tensor([[[0.5, 0.5], [0.0, 2.0]], [[1.0, 0.0], [0.25, 0.75]]])
    dists = torch.tensor([[[1.0, 3.0], [5.0, 0.5]], [[2.0, 9.0], [4.0, 8.0]]])
    pairs = torch.tensor([[0, 1], [1, NONE]], dtype=torch.int32)
    a = Alignment(pairs, [0, 1, 2], plan, dists, torch.zeros(2), ["x", "y"])
    assert len(a) == 2 and a.class_ids() == [["y"], [None]]
    assert a.frame_cost.tolist() == [[2.0, 1.0], [2.0, 7.0]]
    assert a.frame_match.tolist() == [[0.5, 1.0], [0.0, 0.75]]
    ragged = Alignment(torch.tensor([[0, 0], [0, 1], [2, 0]], dtype=torch.int32), [0, 2, 2, 3], plan, dists, torch.zeros(3), [[5, 6], [], [7]])
    assert ragged.class_ids() == [[5, 6], [], [7]]


def test_explain_refusals_are_raised_before_the_device_is_touched():
    from clip_fsar_amd.pool import StreamPool
    g = _live()
    p = StreamPool(g, max_streams=2, stride=2, rate=2, max_push=4)
    h = p.open()
    with pytest.raises(ValueError, match="StreamPool: session 5 is not open"):
        p.explain(5, [0])
    with pytest.raises(ValueError, match="Aligner: give exactly one of classes= and k="):
        p.explain(h)
    with pytest.raises(ValueError, match=r"Aligner: k must be in \[1, min\(16, number of classes = 3\)\]"):
        p.explain(h, k=4)
    with pytest.raises(ValueError, match=r"Aligner: class 9 is not registered"):
        p.explain(h, [9])
    with pytest.raises(ValueError, match="Aligner: 2 class lists for 1 clips"):
        p.explain(h, [[0], [1]])
    # the window: plan_enroll's errors and wording.  T = 4, rate = 2: a window spans 7 frames; cap = 6 + 4 = 10
    with pytest.raises(ValueError, match=r"StreamPool: session 0: window None \(the newest complete one\) is not enrolable -- the ring "
                                         r"holds its windows range\(0, 0\) \(0 frames since open\(\) / reset\(\), cap = 10\)"):
        p.explain(h, [0])
    p._sessions[h].t = 17                                      # frames 7 .. 16 retained: windows 4 (frames 8 .. 14) and 5 (10 .. 16)
    assert p.enrolable(h) == range(4, 6)
    for w in (3, 6, -1, True, 4.0, "4"):
        with pytest.raises(ValueError, match=r"StreamPool: session 0: window %s is not enrolable -- the ring holds its windows "
                                             r"range\(4, 6\)" % re.escape(repr(w))):
            p.explain(h, [0], window=w)
    before = dict(p.stats(h)), p._sessions[h].t, p._sessions[h].tick
    for w in (None, 4, 5):                                     # a good window: the call gets as far as the device
        with pytest.raises(RuntimeError, match="feats must be a HIP device tensor|HIP device tensor"):
            p.explain(h, k=2, window=w)
    assert (dict(p.stats(h)), p._sessions[h].t, p._sessions[h].tick) == before and g._store is None
    from clip_fsar_amd.live_text_gallery import LiveTextGallery
    q = StreamPool(g, max_streams=2)
    q.gallery = LiveTextGallery.__new__(LiveTextGallery)
    with pytest.raises(ValueError, match="Aligner: a LiveTextGallery is refused"):
        q.explain(q.open(), [0])
