"""The few-shot tail kernels of csrc/tail.hip other than the attention and the OTAM kernel -- class_text_logits, build_sequences,
prototypes, text_match_probs, combine_logits, episode_top1, embed_tokens, gather_rows -- at the edges of their class groups, label sets
and E strides, each against a float64 reference of the same operation on the operands as stored in fp32 (oracle/clipfsar_oracle.py:
cos_sim, class_means, text_match_probs, context2_forward, otam_cum_dist), and HipTemporalHead.forward as a whole on synthetic features.

Input families (seeded; feats [n, T, E], text [C, E]):
  gauss   (base + 1.5 randn) * (0.3 + 3 rand) per video / text row: the family of tests/test_gpu_gallery_text.py;
  ortho   independent randn;
  near    base + 0.05 randn on both sides: cosines about 1;
  scale   gauss with every video and text row times 10 ** U(-3, 3), video 0 and text row 0 all zero.  text_match_probs has no epsilon in
          its cosine (0 / 0 for a zero row, in the reference too), so it gets this family without the two zero rows.

Guards.  Every operand is a contiguous view into a larger buffer of NaN (of 2^30 for int32 operands), 64 elements (256 bytes) of it
before and behind the view; every output is a view into a buffer of 7.0 whose surroundings must still be 7.0 afterwards.  The operands
of episode_top1 have 64 EPISODES of NaN around them and its output 64 elements: a lane beyond `episodes` that ran would read NaN and
write into the 7.0.

Label sets of build_sequences / prototypes / text_match_probs.  The episodes of a batch take turns among: a permutation of 0 .. way-1
(the only kind the suite had), {3, 9, 1, 20, 5}, and {7.25, -2, 7, 0.5, 100} (fractional and negative; 7 and 7.25 differ only behind the
point), each continued with further distinct values for way > 5 and cut for way < 5; shots per class 1, 2, 3 or uneven (way 3 with
1, 2 and 3 shots); way 64 with 2 shots reaches S = 128 and, in text_match_probs, the class limit with it (there at Q 4 and T 4 alone: the
reference's 64 class means per episode are its cost).  Real labels are drawn independently of the support labels, so the text row of a
class is a true mean of different rows.

Tolerances, each pinned to the reference by an unmarked CPU test that evaluates the oracle in float32:
  class_text_logits   tol[v, c] = scale * (e_c(E) + 2**-23 k_v), e_c = 1e-6 max(1, sqrt(E / 1024)) (e_d of tests/test_gpu_otam.py),
                      k_v = max_t |x_vt|_2 / |mean_t x_vt|_2 the condition number of the frame mean.  Condition, asserted: k_v <= 32 for
                      every video of every case with E >= 4 (E = 1 is exempt and leans on the per-element term).  A zero video's logits
                      and a zero text row's column are exactly 0.0.
  class means         (build_sequences with merge_before, prototypes without): elementwise (cnt + 1) 2**-24 max_s |x_s[e]|: a sequential
                      fp32 sum of cnt terms, then one multiply by the rounded 1 / cnt.  Every copy is bit-equal.
  text_match_probs    per query scale * (e_c(E) + 2**-23 k) + 2**-22, k the larger of the query's frame-mean condition number and the
                      largest condition number max_s |t_s|_2 / |mean_s t_s|_2 of the episode's class text means: softmax moves a
                      probability by at most half the largest logit error.  Row sums within 1e-5 of 1.
  combine_logits      4 x the worst error of the same formula in float32 torch on the CPU against float64 on the same inputs (the factor:
                      powf and expf of the device may differ from the host's by a few ulp); that product may not exceed BOUND = 2e-5.
                      Float32 torch: 1.48e-07, hence tol 5.93e-07; the tests evaluate both again and assert tol <= BOUND.
  temporal head       BOUND = 2e-5 of tests/test_gpu_gallery.py against the float64 restatement of oracle head_forward lines 226-241.
  episode_top1, embed_tokens, gather_rows: exact (torch.equal).
Float32 oracle on the CPU, worst err / tol: class_text_logits gauss 0.46, ortho 0.18, near 0.65, scale 0.39 (largest k_v at E >= 4: 20.7,
ortho at E 4; near: cosines of about 1 at scale 100, where the host's single chain per dot product and norm carries the whole relative
error); sequential float32 class mean 0.62 (two or three terms and the rounded 1 / 3 come close to the worst case the bound is made
of); text_match_probs 0.06.

Findings and fixes (csrc/tail.hip), both known from reading before any launch:
  text_match_kernel kept its four per-wave dot partials at floats E .. E + 3 of a dynamic LDS block of 2 E floats, outside it for E < 4.
  The partials now have a static __shared__ array of their own and the dynamic block is E floats; the entry keeps accepting every
  E > 0 (class_text_logits serves E = 1 too, and a refusal would have been a new limit of the episode path), and E 1, 2, 3 are cases here.
  episode_top1_kernel took a NaN logit for the maximum only in column 0 (l[c] > bv is false for a NaN on either side), where torch.argmax
  and torch.topk take the first NaN; the tail writes NaN rows for invalid labels, so such rows reach it.  The kernel now takes the first
  NaN and keeps it; rows with a NaN at the first, a middle and the last column and all-NaN rows are cases here.
No other kernel bug was found: every result is inside its bound, nothing is written outside an output, poison stays where the contracts
put it.

Measured on an MI355X with both fixes (run with -s for every figure), worst err / tol:
  class_text_logits   gauss 0.18, ortho 0.19, near 0.25, scale 0.17: at or below the float32 oracle everywhere (64 lane partials per dot).
  build_sequences     class means 0.61 (way 5, 3 shots), 0.56 (uneven), 0.33 (way 64, 2 shots); prototypes 0.61, 0.51, 0.33.  Above half
                      of the bound for the reason the float32 model on the CPU is (0.62): the kernel does exactly that arithmetic.
  text_match_probs    gauss 0.04, ortho 0.04, near 0.06, scale 0.04.
  combine_logits      way 1: 0, way 5: 0.25, way 64: 0.21 (err at most 1.5e-07, the float32 formula's own).
  temporal head       err / BOUND 0.03 at depth 1 and at depth 2, both merge_before values, one and two directions.

Mutations of csrc/tail.hip, each built apart and run once against this file and against the tail tests as they were before it
(tests/test_gpu_kernels.py: test_class_text_logits, test_build_sequences_and_prototypes, test_episode_top1;
tests/test_gpu_gallery_text.py::test_text_kernels_vs_float64_and_episode_kernels -- the earlier tests that launch these kernels directly):
  1. the c0 + j < n_cls write guard of class_text_logits_kernel removed: every class_text case whose n_cls is no multiple of 16 fails
     here (49 cases: wrong values in the next video's row, stores behind the output); the earlier tests pass.
  2. labels[t] < labels[s] of label_ranks on (int) casts: 21 cases fail here (build_sequences / prototypes at every way > 1, both poison
     contracts, text_match_probs, the temporal head); the earlier tests pass.
  3. rl[s] replaced by rl[c] in text_match_kernel: text_match_probs fails here at every way > 1, and its poison test; the earlier tests pass.
  4. the e >= episodes return of episode_top1_kernel removed: all six episode_top1 cases fail here (stores behind acc); the earlier
     test passes.
"""
import functools
import math
import zlib

import pytest
import torch

import clipfsar_oracle as orc
from test_gpu_gallery_text import BOUND
from test_gpu_gallery_text import _restated as _restated_text

gpu = pytest.mark.gpu
DEV = torch.device("cuda")

NAN = float("nan")
SENT = 7.0
G = 64                                   # guard elements on either side of a view: 256 bytes
BAD_INT = 1 << 30
FAMILIES = ["gauss", "ortho", "near", "scale"]
SCALES = [1.0, 4.0, 100.0]


def seed_of(*xs):
    return zlib.crc32(repr(xs).encode())


def e_c(E):
    return 1e-6 * max(1.0, math.sqrt(E / 1024.0))


# ---------------------------------------------------------------------------------------------------------------- inputs
def make_family(family, n, T, E, C, seed, zeros=True):
    """(feats [n, T, E], text [C, E]) of a family: a function of its arguments alone"""
    g = torch.Generator().manual_seed(seed)
    base = torch.randn(E, generator=g)
    if family in ("gauss", "scale"):
        feats = (base + 1.5 * torch.randn(n, T, E, generator=g)) * (0.3 + 3 * torch.rand(n, 1, 1, generator=g))
        text = (base + 1.5 * torch.randn(C, E, generator=g)) * (0.3 + 3 * torch.rand(C, 1, generator=g))
        if family == "scale":
            feats = feats * 10.0 ** (6.0 * torch.rand(n, 1, 1, generator=g) - 3.0)
            text = text * 10.0 ** (6.0 * torch.rand(C, 1, generator=g) - 3.0)
            if zeros:
                feats[0] = 0.0
                text[0] = 0.0
    elif family == "ortho":
        feats, text = torch.randn(n, T, E, generator=g), torch.randn(C, E, generator=g)
    elif family == "near":
        feats, text = base + 0.05 * torch.randn(n, T, E, generator=g), base + 0.05 * torch.randn(C, E, generator=g)
    else:
        raise ValueError(family)
    return feats.float().contiguous(), text.float().contiguous()


def mean_condition(x):
    """x [n, m, E] float64 -> [n]: max_m |x_nm|_2 / |mean_m x_nm|_2, the condition number of the mean over m (0 where every row is zero)"""
    top, mn = x.norm(dim=2).amax(1), x.mean(1).norm(dim=1)
    return torch.where(top > 0, top / mn, torch.zeros_like(top))


L_PLAIN = [3.0, 9.0, 1.0, 20.0, 5.0]
L_FRACT = [7.25, -2.0, 7.0, 0.5, 100.0]
WAY_SHOT = [(1, 1), (5, 1), (5, 3), (3, "uneven"), (64, 2)]          # the last: S = 128 = MAX_S, way 64: both limits at once


def label_values(kind, way):
    if kind == 0:
        return [float(i) for i in range(way)]
    if kind == 1:
        return (L_PLAIN + [22.0 + 3.0 * i for i in range(way)])[:way]
    return (L_FRACT + [v for i in range(way) for v in (100.5 + 0.25 * i, -2.5 - 0.5 * i)])[:way]


def shot_counts(way, shot):
    return [1, 2, 3] if shot == "uneven" else [shot] * way


def make_labels(B, way, shot, n_test, seed, kind0=1):
    """(support labels [B, S], real labels [B, S]) as float32: episode b takes label kind (kind0 + b) % 3, its classes get the shot counts in
    a random order, its supports a random order; the real labels are independent draws from [0, n_test)"""
    g = torch.Generator().manual_seed(seed)
    counts = shot_counts(way, shot)
    S = sum(counts)
    lab = torch.empty(B, S)
    for b in range(B):
        vals = torch.tensor(label_values((kind0 + b) % 3, way))[torch.randperm(way, generator=g)]
        lab[b] = vals.repeat_interleave(torch.tensor(counts))[torch.randperm(S, generator=g)]
    real = torch.randint(0, n_test, (B, S), generator=g).float()
    return lab, real


# ---------------------------------------------------------------------------------------------------------------- GPU helpers
def guarded_empty(shape, dtype=torch.float32, fill=NAN, g=G):
    """a contiguous device view of `shape` into a larger buffer of `fill`, g elements of it before and behind"""
    n = math.prod(shape)
    buf = torch.full((n + 2 * g,), fill, dtype=dtype, device=DEV)
    return buf[g:g + n].view(shape)


def guarded(t, fill=None, g=G):
    v = guarded_empty(tuple(t.shape), t.dtype, (NAN if t.dtype.is_floating_point else BAD_INT) if fill is None else fill, g)
    v.copy_(t)
    return v


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


def check(got, ref, tol, what):
    """every element within its tolerance (tol: a number or a tensor that broadcasts) -> worst err / tol; a NaN fails"""
    err = (got.double() - ref).abs()
    tol = torch.as_tensor(tol, dtype=torch.float64).expand_as(err)
    ok = err <= tol
    assert bool(ok.all()), "%s: %d of %d outside, worst err %.3e at tol %.3e" % (
        what, int((~ok).sum()), ok.numel(), float(err[~ok].nan_to_num(math.inf).max()), float(tol[~ok].min()))
    return float((err / tol).max()) if err.numel() else 0.0


def check_mixed(got, ref, tol, what):
    """tol == 0: bit-equal to ref rounded to fp32 (a copy); tol > 0: within tol -> worst err / tol over the latter"""
    exact = tol == 0
    assert torch.equal(got[exact], ref.float()[exact]), what + ": a copy is not bit-equal"
    if bool(exact.all()):
        return 0.0
    return check(got[~exact], ref[~exact], tol[~exact], what)


def report(kernel, family, ratio):
    print("tail-worst %s %s %.4f" % (kernel, family, ratio))


# ================================================================================================================ 1: class_text_logits
CT_NCLS = [1, 3, 4, 5, 15, 16, 17, 31, 64, 70]                       # the edges of the wave's 4 classes and the workgroup's 16
CT_E = [1, 4, 63, 64, 65, 255, 256, 257, 512, 1024, 15000]           # 15000: the largest E the entry accepts
CT_T = [1, 8, 16]
CT_NV = 30
CT_CASES = list(dict.fromkeys([("gauss", E, c) for E in CT_E for c in (17, 70)] + [("gauss", E, c) for E in (64, 257) for c in CT_NCLS]
                              + [(f, E, c) for f in FAMILIES for E in (4, 512) for c in (17, 70)] + [(f, 1, 17) for f in FAMILIES]))


def ct_inputs(family, E, n_cls, T):
    return make_family(family, CT_NV, T, E, n_cls, seed_of("ct", family, E, n_cls, T))


def ct_reference(feats, text):
    """float64 -> (cos_sim(mean_T feats, text) [n, C], k_v [n])"""
    x = feats.double()
    return orc.cos_sim(x.mean(1), text.double()), mean_condition(x)


def ct_tol(E, k, scale):
    return scale * (e_c(E) + 2.0 ** -23 * k[:, None])


@pytest.mark.parametrize("family", FAMILIES)
def test_class_text_float32_oracle_is_within_tol_and_inputs_meet_the_condition(family):
    worst, worst_plain, worst_k = 0.0, 0.0, 0.0
    for fam, E, n_cls in CT_CASES:
        if fam != family:
            continue
        for T in CT_T:
            feats, text = ct_inputs(fam, E, n_cls, T)
            ref, k = ct_reference(feats, text)
            if E >= 4:
                worst_k = max(worst_k, float(k.max()))
                assert float(k.max()) <= 32.0, (fam, E, n_cls, T, float(k.max()))                     # the condition
            for scale in SCALES:
                f32 = orc.cos_sim(feats.mean(1), text) * torch.tensor(scale)
                worst = max(worst, check(f32, scale * ref, ct_tol(E, k, scale), "float32 oracle %s E %d C %d T %d" % (fam, E, n_cls, T)))
                worst_plain = max(worst_plain, float(((f32.double() - scale * ref).abs() / (scale * e_c(E))).max()))
    print("class_text %s: float32 oracle worst err / tol %.3f (err / e_c alone %.3f), largest k_v at E >= 4 %.1f" % (family, worst, worst_plain,
                                                                                                                   worst_k))


@gpu
@pytest.mark.parametrize("family,E,n_cls", CT_CASES)
def test_class_text_logits_vs_float64(family, E, n_cls):
    from clip_fsar_amd import hip
    pending = []
    for T in CT_T:
        feats, text = ct_inputs(family, E, n_cls, T)
        ref, k = ct_reference(feats, text)
        assert E < 4 or float(k.max()) <= 32.0
        tx = guarded(text)
        for nv, lo in ((CT_NV, 0), (1, CT_NV - 1)):
            f = guarded(feats[lo:lo + nv])
            for scale in SCALES:
                out = Out(nv, n_cls)
                hip.class_text_logits(f, tx, guarded(torch.tensor([scale])), out.view, nv, T, E)
                pending.append((T, nv, lo, scale, out, ref[lo:lo + nv], k[lo:lo + nv]))
    torch.cuda.synchronize()
    worst = 0.0
    for T, nv, lo, scale, out, ref, k in pending:
        what = "%s E %d C %d T %d videos %d scale %g" % (family, E, n_cls, T, nv, scale)
        got = out.get()
        worst = max(worst, check(got, scale * ref, ct_tol(E, k, scale), what))
        if family == "scale":
            assert bool((got[:, 0] == 0.0).all()), what + ": the zero text row's column"
            if lo == 0:
                assert bool((got[0] == 0.0).all()), what + ": the zero video's logits"
    report("class_text_logits", family, worst)


@gpu
def test_class_text_logits_refusals():
    from clip_fsar_amd import hip
    import ctypes
    out = Out(1, 2)
    sc, tx = guarded(torch.tensor([1.0])), guarded_empty((2, 15001))
    with pytest.raises(RuntimeError, match="cfsar_class_text_logits: bad shape"):
        hip.class_text_logits(guarded_empty((1, 1, 15001)), tx, sc, out.view, 1, 1, 15001)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())                                                         # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    f = guarded_empty((1, 1, 4))
    for args in ((None, ptr(tx), ptr(sc), ptr(out.view)), (ptr(f), None, ptr(sc), ptr(out.view)), (ptr(f), ptr(tx), None, ptr(out.view)),
                 (ptr(f), ptr(tx), ptr(sc), None)):
        rc = hip.lib().cfsar_class_text_logits(*args, 1, 1, 4, 2, st)
        with pytest.raises(RuntimeError, match="cfsar_class_text_logits: null pointer"):
            hip._check(rc, "cfsar_class_text_logits")
    torch.cuda.synchronize()
    assert bool((out.get() == SENT).all())


# ================================================================================================================ 2: build_sequences, prototypes
SEQ_B, SEQ_Q, SEQ_T, SEQ_NTEST = [1, 3], [1, 4], [1, 4], [1, 24]
SEQ_E = [1, 64, 127, 128, 129, 300]                                   # around the 128-thread stride


def seq_combos(way, shot, es=SEQ_E):
    i = 0
    for B in SEQ_B:
        for Q in SEQ_Q:
            for T in SEQ_T:
                for E in es:
                    for n_test in SEQ_NTEST:
                        yield i, B, Q, T, E, n_test
                        i += 1


def seq_inputs(way, shot, i, B, Q, T, E, n_test, family="gauss", zeros=True):
    S = sum(shot_counts(way, shot))
    feats, text = make_family(family, B * (S + Q), T, E, n_test, seed_of("seq", way, shot, i), zeros)
    lab, real = make_labels(B, way, shot, n_test, seed_of("lab", way, shot, i), kind0=1 + i)
    return S, feats.reshape(B, S + Q, T, E), text, lab, real


def class_mean_reference(x, labels):
    """x [S, ...] fp32, labels [S] -> (float64 class means [way, ...] in ascending label order (oracle class_means), their tolerance
    (cnt + 1) 2**-24 max_s |x_s|)"""
    means, uniq = orc.class_means(x.double(), labels)
    tol = torch.stack([(float((labels == c).sum()) + 1.0) * 2.0 ** -24 * x[labels == c].double().abs().amax(0) for c in uniq])
    return means, tol


def seq_reference(feats, text, lab, real, S, merge_before):
    """-> (X [rows, E] float64, tol [rows, E]; tol 0 marks a copy)"""
    B, _, T, E = feats.shape
    xq = feats[:, S:].reshape(-1, E).double()
    rows, tols = [xq], [torch.zeros_like(xq)]
    for b in range(B):
        seq = torch.cat([feats[b, :S], text[real[b].long()].unsqueeze(1)], 1)                  # [S, T + 1, E]
        if merge_before:
            m, t = class_mean_reference(seq, lab[b])
        else:
            m, t = seq.double(), torch.zeros(S, T + 1, E, dtype=torch.float64)
        rows.append(m.reshape(-1, E))
        tols.append(t.reshape(-1, E))
    return torch.cat(rows), torch.cat(tols)


def proto_reference(Xs, lab, merge_before):
    """Xs [B, Sp, T + 1, E] fp32 as build_sequences wrote it -> (protos [B, way, T, E] float64, tol; tol 0 marks a copy)"""
    if merge_before:
        return Xs[:, :, :-1].double(), torch.zeros_like(Xs[:, :, :-1], dtype=torch.float64)
    pairs = [class_mean_reference(Xs[b, :, :-1], lab[b]) for b in range(Xs.shape[0])]
    return torch.stack([p[0] for p in pairs]), torch.stack([p[1] for p in pairs])


def test_float32_sequential_class_mean_is_within_tol():
    """the kernels' arithmetic -- a sequential fp32 sum over the class's supports, then one multiply by the rounded 1 / cnt -- in float32
    torch, against the float64 class_means: inside (cnt + 1) 2**-24 max |x|"""
    worst = 0.0
    for way, shot in WAY_SHOT:
        for family in FAMILIES:
            S = sum(shot_counts(way, shot))
            feats, _ = make_family(family, S, 4, 129, 1, seed_of("cm", way, shot, family))
            lab, _ = make_labels(1, way, shot, 1, seed_of("cml", way, shot), kind0=2)
            ref, tol = class_mean_reference(feats, lab[0])
            for i, c in enumerate(torch.unique(lab[0])):
                acc = torch.zeros(4, 129)
                for s in range(S):
                    if lab[0, s] == c:
                        acc = acc + feats[s]
                cnt = int((lab[0] == c).sum())
                got = acc * (torch.tensor(1.0) / torch.tensor(float(cnt)))
                nz = tol[i] > 0
                worst = max(worst, check(got[nz], ref[i][nz], tol[i][nz], "class mean way %d shot %s %s" % (way, shot, family)))
                assert bool((got[~nz] == 0).all())
    print("sequential float32 class mean: worst err / tol %.3f" % worst)


@gpu
@pytest.mark.parametrize("merge_before", [False, True])
@pytest.mark.parametrize("way,shot", WAY_SHOT)
def test_build_sequences_and_prototypes_vs_float64(way, shot, merge_before):
    from clip_fsar_amd import hip
    worst = {"build_sequences": 0.0, "prototypes": 0.0}
    for i, B, Q, T, E, n_test in seq_combos(way, shot):
        S, feats, text, lab, real = seq_inputs(way, shot, i, B, Q, T, E, n_test, family="scale" if i % 4 == 3 else "gauss")
        Sp = way if merge_before else S
        rows_q = B * Q * T
        labd = guarded(lab)
        X = Out(rows_q + B * Sp * (T + 1), E)
        hip.build_sequences(guarded(feats), guarded(text), labd, guarded(real), X.view, B, S, Q, T, E, way, merge_before)
        xs = guarded(X.view[rows_q:])                                      # the support rows as an operand of their own
        protos = Out(B, way, T, E)
        hip.prototypes(xs, labd, protos.view, B, S, Sp, T, E, way, merge_before)
        torch.cuda.synchronize()
        what = "way %d shot %s merge %d B %d Q %d T %d E %d n_test %d" % (way, shot, merge_before, B, Q, T, E, n_test)
        got = X.get()
        ref, tol = seq_reference(feats, text, lab, real, S, merge_before)
        worst["build_sequences"] = max(worst["build_sequences"], check_mixed(got, ref, tol, "build_sequences " + what))
        pref, ptol = proto_reference(got[rows_q:].reshape(B, Sp, T + 1, E), lab, merge_before)
        worst["prototypes"] = max(worst["prototypes"], check_mixed(protos.get(), pref, ptol, "prototypes " + what))
    for k, v in worst.items():
        report(k, "mixed", v)


def _poison_case(merge_before):
    way, shot, B, Q, T, E, n_test = 5, 2, 3, 2, 4, 129, 24
    S, feats, text, lab, real = seq_inputs(way, shot, 0, B, Q, T, E, n_test)
    return way, B, S, Q, T, E, n_test, feats, text, lab, real


def _run_sequences(hip, feats, text, lab, real, B, S, Q, T, E, way, merge_before):
    Sp = way if merge_before else S
    rows_q = B * Q * T
    X = Out(rows_q + B * Sp * (T + 1), E)
    labd = guarded(lab)
    hip.build_sequences(guarded(feats), guarded(text), labd, guarded(real), X.view, B, S, Q, T, E, way, merge_before)
    protos = Out(B, way, T, E)
    hip.prototypes(guarded(X.view[rows_q:]), labd, protos.view, B, S, Sp, T, E, way, merge_before)
    torch.cuda.synchronize()
    return X.get()[:rows_q], X.get()[rows_q:].reshape(B, Sp, T + 1, E), protos.get()


@gpu
@pytest.mark.parametrize("merge_before", [False, True])
def test_an_out_of_range_real_label_poisons_exactly_its_text_row(merge_before):
    from clip_fsar_amd import hip
    way, B, S, Q, T, E, n_test, feats, text, lab, real = _poison_case(merge_before)
    clean = _run_sequences(hip, feats, text, lab, real, B, S, Q, T, E, way, merge_before)
    assert all(bool(torch.isfinite(c).all()) for c in clean)
    bad = real.clone()
    bad[0, 3], bad[2, S - 1] = -1.0, float(n_test)
    xq, xs, protos = _run_sequences(hip, feats, text, lab, bad, B, S, Q, T, E, way, merge_before)
    want = torch.zeros_like(xs, dtype=torch.bool)
    for b, s in ((0, 3), (2, S - 1)):
        row = int((torch.unique(lab[b]) < lab[b, s]).sum()) if merge_before else s
        want[b, row, T] = True
    assert torch.equal(torch.isnan(xs), want)
    assert torch.equal(xs[~want], clean[1][~want]) and torch.equal(xq, clean[0])
    assert torch.equal(protos, clean[2])                                   # a prototype never holds the text token


@gpu
@pytest.mark.parametrize("merge_before", [False, True])
def test_a_missing_class_poisons_exactly_its_rows(merge_before):
    """episode 1 of 3 holds 4 distinct labels for way 5: with merge_before every row of class 4 is NaN (frames and text), the prototype of
    class 4 is NaN with either merge_before, and the other classes of that episode are the means of the labels as they are"""
    from clip_fsar_amd import hip
    way, B, S, Q, T, E, n_test, feats, text, lab, real = _poison_case(merge_before)
    clean = _run_sequences(hip, feats, text, lab, real, B, S, Q, T, E, way, merge_before)
    few = lab.clone()
    top = few[1].max()
    few[1][few[1] == top] = few[1].min()                                   # the largest label's supports join the smallest: 4 classes
    assert len(torch.unique(few[1])) == way - 1
    xq, xs, protos = _run_sequences(hip, feats, text, few, real, B, S, Q, T, E, way, merge_before)
    want = torch.zeros_like(xs, dtype=torch.bool)
    if merge_before:
        want[1, way - 1] = True
    assert torch.equal(torch.isnan(xs), want) and torch.equal(xq, clean[0])
    pwant = torch.zeros_like(protos, dtype=torch.bool)
    pwant[1, way - 1] = True
    assert torch.equal(torch.isnan(protos), pwant)
    for b in (0, 2):
        assert torch.equal(xs[b], clean[1][b]) and torch.equal(protos[b], clean[2][b])
    seq = torch.cat([feats[1, :S], text[real[1].long()].unsqueeze(1)], 1)
    if merge_before:
        ref, tol = class_mean_reference(seq, few[1])
        check(xs[1, :way - 1], ref, tol, "the four classes that exist")
        assert torch.equal(protos[1, :way - 1], xs[1, :way - 1, :T])
    else:
        assert torch.equal(xs[1], seq)
        ref, tol = class_mean_reference(xs[1, :, :T], few[1])
        check(protos[1, :way - 1], ref, tol, "the four prototypes that exist")


@gpu
def test_sequence_entry_points_refuse_bad_arguments_before_any_launch():
    from clip_fsar_amd import hip
    E, T, Q = 4, 1, 1
    X, protos = Out(200 * (T + 1), E), Out(1, 5, T, E)
    text, feats = guarded_empty((2, E)), guarded_empty((1, 130 + Q, T, E))
    lab = guarded_empty((1, 130))
    with pytest.raises(RuntimeError, match="cfsar_build_sequences: S=129 > 128"):
        hip.build_sequences(feats, text, lab, lab, X.view, 1, 129, Q, T, E, 1, False)
    with pytest.raises(RuntimeError, match="cfsar_build_sequences: S=7 is not a multiple of way=5"):
        hip.build_sequences(feats, text, lab, lab, X.view, 1, 7, Q, T, E, 5, True)
    xs = guarded_empty((1, 130, T + 1, E))
    with pytest.raises(RuntimeError, match="cfsar_prototypes: bad shape"):
        hip.prototypes(xs, lab, protos.view, 1, 129, 129, T, E, 5, False)
    for Sp, merge_before in ((5, False), (10, True), (6, True)):
        with pytest.raises(RuntimeError, match="cfsar_prototypes: Sp=%d inconsistent with merge_before" % Sp):
            hip.prototypes(xs, lab, protos.view, 1, 10, Sp, T, E, 5, merge_before)
    torch.cuda.synchronize()
    assert bool((X.get() == SENT).all()) and bool((protos.get() == SENT).all())


# ================================================================================================================ 3: text_match_probs, combine_logits
TM_E = [1, 2, 3, 4, 60, 64, 252, 256, 260, 1024]                     # 1, 2, 3: since the per-wave partials left the dynamic LDS block
TM_FAMILIES = ["gauss", "ortho", "near", "scale"]                    # scale: without the zero rows (no epsilon in this cosine)


def tm_inputs(way, shot, i, B, Q, T, E, n_test, family):
    """feats [B, S + Q, T, E] whose support part is NaN (the kernel reads the queries alone), text, labels"""
    S = sum(shot_counts(way, shot))
    q, text = make_family(family, B * Q, T, E, n_test, seed_of("tm", way, shot, i), zeros=False)
    feats = torch.full((B, S + Q, T, E), NAN)
    feats[:, S:] = q.reshape(B, Q, T, E)
    lab, real = make_labels(B, way, shot, n_test, seed_of("tml", way, shot, i), kind0=1 + i)
    return S, feats, text, lab, real


def tm_condition(feats, text, lab, real, S):
    """-> k [B, Q]: the larger of the query's frame-mean condition number and the largest of the episode's class text means"""
    B = feats.shape[0]
    ks = []
    for b in range(B):
        rows = text[real[b].long()].double()
        kc = max(float(mean_condition(rows[lab[b] == c].unsqueeze(0))) for c in torch.unique(lab[b]))
        ks.append(mean_condition(feats[b, S:].double()).clamp_min(kc))
    return torch.stack(ks)


def tm_reference(feats, text, lab, real, S, scale, dtype=torch.float64):
    return torch.stack([orc.text_match_probs(feats[b, S:].to(dtype), text.to(dtype), lab[b], real[b], scale) for b in range(feats.shape[0])])


def tm_tol(E, k, scale):
    return (scale * (e_c(E) + 2.0 ** -23 * k) + 2.0 ** -22)[:, :, None]


def tm_combos(way, shot):
    """way 64 (S 128) at Q 4 and T 4 alone: its limits do not meet Q or T, and the reference's 64 class means per episode are its cost"""
    for i, B, Q, T, E, n_test in seq_combos(way, shot, TM_E):
        if way < 64 or (Q == 4 and T == 4):
            yield i, B, Q, T, E, n_test, TM_FAMILIES[(i // 2 + i // 20) % 4]


@pytest.mark.parametrize("way,shot", WAY_SHOT)
def test_text_match_float32_oracle_is_within_tol(way, shot):
    worst = 0.0
    for i, B, Q, T, E, n_test, family in tm_combos(way, shot):
        S, feats, text, lab, real = tm_inputs(way, shot, i, B, Q, T, E, n_test, family)
        k = tm_condition(feats, text, lab, real, S)
        for scale in SCALES:
            ref = tm_reference(feats, text, lab, real, S, scale)
            f32 = tm_reference(feats, text, lab, real, S, scale, torch.float32)
            worst = max(worst, check(f32, ref, tm_tol(E, k, scale), "float32 oracle way %d shot %s %s B %d Q %d T %d E %d n_test %d scale %g" % (
                way, shot, family, B, Q, T, E, n_test, scale)))
    print("text_match way %d shot %s: float32 oracle worst err / tol %.3f" % (way, shot, worst))


@gpu
@pytest.mark.parametrize("way,shot", WAY_SHOT)
def test_text_match_probs_vs_float64(way, shot):
    from clip_fsar_amd import hip
    worst = dict.fromkeys(TM_FAMILIES, 0.0)
    for i, B, Q, T, E, n_test, family in tm_combos(way, shot):
        S, feats, text, lab, real = tm_inputs(way, shot, i, B, Q, T, E, n_test, family)
        k = tm_condition(feats, text, lab, real, S)
        f, tx, labd, reald = guarded(feats), guarded(text), guarded(lab), guarded(real)
        outs = []
        for scale in SCALES:
            p = Out(B, Q, way)
            hip.text_match_probs(f, tx, labd, reald, guarded(torch.tensor([scale])), p.view, B, S, Q, T, E, way)
            outs.append((scale, p))
        torch.cuda.synchronize()
        for scale, p in outs:
            what = "way %d shot %s %s B %d Q %d T %d E %d n_test %d scale %g" % (way, shot, family, B, Q, T, E, n_test, scale)
            got = p.get()
            worst[family] = max(worst[family], check(got, tm_reference(feats, text, lab, real, S, scale), tm_tol(E, k, scale), what))
            assert float((got.double().sum(2) - 1.0).abs().max()) <= 1e-5, what + ": row sums"
    for family, v in worst.items():
        report("text_match_probs", family, v)


@gpu
def test_text_match_poison_stays_in_its_episode():
    from clip_fsar_amd import hip
    way, shot, B, Q, T, E, n_test = 5, 2, 4, 3, 4, 260, 24
    S, feats, text, lab, real = tm_inputs(way, shot, 0, B, Q, T, E, n_test, "gauss")
    bad_real, few = real.clone(), lab.clone()
    bad_real[0, 2], bad_real[2, S - 1] = float(n_test), -1.0
    few[3][few[3] == few[3].max()] = few[3].min()                          # episode 3: 4 distinct labels for way 5
    f, tx, sc = guarded(feats), guarded(text), guarded(torch.tensor([4.0]))
    clean, got = Out(B, Q, way), Out(B, Q, way)
    hip.text_match_probs(f, tx, guarded(lab), guarded(real), sc, clean.view, B, S, Q, T, E, way)
    hip.text_match_probs(f, tx, guarded(few), guarded(bad_real), sc, got.view, B, S, Q, T, E, way)
    torch.cuda.synchronize()
    c, g = clean.get(), got.get()
    assert bool(torch.isfinite(c).all())
    for b in (0, 2, 3):
        assert bool(torch.isnan(g[b]).all()), b
    assert torch.equal(g[1], c[1])


@gpu
def test_text_match_refuses_way_65():
    from clip_fsar_amd import hip
    p = Out(1, 1, 65)
    lab = guarded_empty((1, 130))
    for way, S in ((65, 65), (65, 130), (5, 129)):
        with pytest.raises(RuntimeError, match="cfsar_text_match_probs: bad shape"):
            hip.text_match_probs(guarded_empty((1, S + 1, 1, 4)), guarded_empty((2, 4)), lab, lab, guarded(torch.tensor([1.0])), p.view, 1, S, 1, 1,
                                 4, way)
    torch.cuda.synchronize()
    assert bool((p.get() == SENT).all())


CB_COFF, CB_WAY, CB_NQ = [0.0, 0.5, 0.9, 1.0], [1, 5, 64], [1, 70]


def cb_inputs(way, nq):
    """(stored text probabilities [nq, way], visual logits [nq, way] in [-64, 0]): softmax rows of several sharpnesses, probabilities of
    exactly 0, rows where one class holds all the mass, visual logits of exactly -64 and 0"""
    g = torch.Generator().manual_seed(seed_of("cb", way, nq))
    p = torch.softmax(torch.randn(nq, way, generator=g) * 10.0 ** (3.0 * torch.rand(nq, 1, generator=g) - 1.0), 1)
    p[torch.rand(nq, way, generator=g) < 0.1] = 0.0
    hot = torch.arange(nq) % 4 == 0                                        # query 0 among them
    p[hot] = torch.nn.functional.one_hot(torch.randint(0, way, (int(hot.sum()),), generator=g), way).float()
    vis = -64.0 * torch.rand(nq, way, generator=g)
    vis[torch.rand(nq, way, generator=g) < 0.05] = -64.0
    vis[torch.rand(nq, way, generator=g) < 0.05] = 0.0
    return p.float().contiguous(), vis.float().contiguous()


def cb_reference(p, vis, coff, dtype=torch.float64):
    """the combine formula of test_gpu_gallery_text._restated on stored probabilities"""
    return p.to(dtype).pow(coff) * torch.softmax((8.0 + vis.to(dtype)) / 8.0, 1).pow(1.0 - coff)


@functools.lru_cache(maxsize=1)
def cb_float32_error():
    """the worst error of the formula in float32 torch on the CPU, over every case"""
    worst = 0.0
    for way in CB_WAY:
        for nq in CB_NQ:
            p, vis = cb_inputs(way, nq)
            for coff in CB_COFF:
                worst = max(worst, float((cb_reference(p, vis, coff, torch.float32).double() - cb_reference(p, vis, coff)).abs().max()))
    return worst


def test_combine_reference_is_the_restated_formula_and_its_float32_error_is_below_bound():
    feats, text = make_family("gauss", 7, 1, 16, 5, 1)
    vis = -8.0 * torch.rand(7, 5, generator=torch.Generator().manual_seed(2))
    _, p = _restated_text(feats[:, 0], text, 4.0)
    assert torch.equal(_restated_text(feats[:, 0], text, 4.0, vis, 0.9)[1], cb_reference(p, vis, 0.9))
    err = cb_float32_error()
    print("combine: float32 torch worst err %.3e, tol %.3e" % (err, 4.0 * err))
    assert 0.0 < 4.0 * err <= BOUND


@gpu
@pytest.mark.parametrize("way", CB_WAY)
def test_combine_logits_vs_float64(way):
    from clip_fsar_amd import hip
    tol = 4.0 * cb_float32_error()
    assert tol <= BOUND
    pending = []
    for nq in CB_NQ:
        p, vis = cb_inputs(way, nq)
        pd, vd = guarded(p), guarded(vis)
        for coff in CB_COFF:
            out = Out(nq, way)
            hip.combine_logits(pd, vd, out.view, nq, way, coff)
            pending.append((nq, coff, out, cb_reference(p, vis, coff)))
    torch.cuda.synchronize()
    worst = 0.0
    for nq, coff, out, ref in pending:
        worst = max(worst, check(out.get(), ref, tol, "combine way %d queries %d coff %g" % (way, nq, coff)))
    report("combine_logits", "way%d" % way, worst)


# ================================================================================================================ 4: exact kernels
def top1_inputs(episodes, Q, way):
    g = torch.Generator().manual_seed(seed_of("top1", episodes, Q, way))
    logits = torch.randn(episodes, Q, way, generator=g)
    labels = torch.randint(0, way, (episodes, Q), generator=g).float()
    mid = way // 2
    rows = logits.view(-1, way)
    n = rows.shape[0]
    # ties first / last, middle / last and all equal, a lone maximum in the middle and in the last column; NaN at the first, a middle,
    # the last column and at two columns; an all-NaN row
    for r, (cols, v) in enumerate([((0, way - 1), 9.0), ((mid, way - 1), 9.0), ((mid, mid), 9.0), ((way - 1, way - 1), 9.0), ((0, 0), NAN),
                                   ((mid, mid), NAN), ((way - 1, way - 1), NAN), ((mid, way - 1), NAN), (tuple(range(way)), NAN),
                                   (tuple(range(way)), 1.0)]):
        for r2 in range(r, n, 11):                                         # every 11th row from r: all the episodes, the last ones too
            rows[r2, list(cols)] = v
    ref = logits.argmax(2)
    lab = labels.view(-1)
    lab[0::3] = ref.view(-1)[0::3].float()                                 # a third of the queries hit for certain
    lab[1::7] = -1.0                                                       # labels outside [0, way) never hit
    lab[2::7] = float(way)
    lab[4::7] = float(way + 3)
    return logits, labels


@gpu
@pytest.mark.parametrize("way", [1, 5, 64])
@pytest.mark.parametrize("Q", [1, 5])
def test_episode_top1_is_argmax(Q, way):
    from clip_fsar_amd import hip
    pending = []
    for episodes in (1, 63, 64, 65, 200):
        logits, labels = top1_inputs(episodes, Q, way)
        acc = Out(episodes)
        hip.episode_top1(guarded(logits, g=64 * Q * way), guarded(labels, g=64 * Q), acc.view)
        pending.append((episodes, logits, labels, acc))
    torch.cuda.synchronize()
    for episodes, logits, labels, acc in pending:
        hits = logits.argmax(2) == labels.long()
        assert way == 1 or 0 < int(hits.sum()) < hits.numel() or episodes * Q < 4
        assert torch.equal(acc.get(), hits.float().mean(1)), (episodes, Q, way)


EX_W = [1, 127, 128, 129, 512]


@gpu
@pytest.mark.parametrize("W", EX_W)
def test_embed_tokens_is_one_add(W):
    from clip_fsar_amd import hip
    vocab = 50
    pending = []
    for L in (1, 77):
        for n_seq in (1, 5):
            g = torch.Generator().manual_seed(seed_of("embed", W, L, n_seq))
            table, pos = torch.randn(vocab, W, generator=g), torch.randn(L, W, generator=g)
            tokens = torch.randint(0, vocab, (n_seq, L), generator=g, dtype=torch.int32)
            special = torch.tensor([0, vocab - 1, -3, vocab + 5], dtype=torch.int32)
            tokens.view(-1)[:4] = special[:n_seq * L]
            tokens.view(-1)[-1] = special[(W + L) % 4]
            out = Out(n_seq * L, W)
            hip.embed_tokens(guarded(tokens), guarded(table), guarded(pos), out.view)
            pending.append((table, pos, tokens, out))
    torch.cuda.synchronize()
    for table, pos, tokens, out in pending:
        n_seq, L = tokens.shape
        ref = (table[tokens.long().clamp(0, vocab - 1)] + pos[None]).reshape(n_seq * L, W)
        assert torch.equal(out.get(), ref), (W, L, n_seq)


@gpu
@pytest.mark.parametrize("D", EX_W)
def test_gather_rows_is_a_clamped_copy(D):
    from clip_fsar_amd import hip
    pending = []
    for rows_in in (1, 9):
        for n in (1, 13):
            g = torch.Generator().manual_seed(seed_of("gather", D, rows_in, n))
            x = torch.randn(rows_in, D, generator=g)
            idx = torch.randint(0, rows_in, (n,), generator=g, dtype=torch.int32)
            special = torch.tensor([rows_in, -1, rows_in - 1, rows_in - 1, 0, 0], dtype=torch.int32)     # out of range, repeated
            idx[:6] = special[:n]
            out = Out(n, D)
            hip.gather_rows(guarded(x), guarded(idx), out.view)
            pending.append((x, idx, out))
    torch.cuda.synchronize()
    for x, idx, out in pending:
        assert torch.equal(out.get(), x[idx.long().clamp(0, x.shape[0] - 1)]), (D, tuple(x.shape), idx.tolist())


# ================================================================================================================ 5: the temporal head
HEAD_E, HEAD_T, HEAD_B, HEAD_Q, HEAD_WAY, HEAD_NTEST = 64, 4, 2, 3, 3, 24


@functools.lru_cache(maxsize=2)
def head_case(depth):
    import clip_fsar_amd.synth as synth
    sd = {k: torch.from_numpy(v) for k, v in synth.context2_state_dict(HEAD_E, 8, HEAD_E // 8, depth=depth, seed=18, prefix="context2.").items()}
    S = sum(shot_counts(HEAD_WAY, "uneven"))
    feats, text = make_family("gauss", HEAD_B * (S + HEAD_Q), HEAD_T, HEAD_E, HEAD_NTEST, seed_of("head", depth))
    lab, real = make_labels(HEAD_B, HEAD_WAY, "uneven", HEAD_NTEST, seed_of("headl", depth), kind0=1)      # {3, 9, 1}, then {7.25, -2, 7}
    return sd, S, feats.reshape(HEAD_B, S + HEAD_Q, HEAD_T, HEAD_E), text, lab, real


@functools.lru_cache(maxsize=4)
def head_reference(depth, merge_before):
    """oracle head_forward lines 226-241 in float64 on synthetic features -> per-direction costs (c0, c1) [B, Q, way]"""
    sd, S, feats, text, lab, real = head_case(depth)
    sd = {k: v.double() for k, v in sd.items()}
    T, E = HEAD_T, HEAD_E
    c0, c1 = [], []
    for b in range(HEAD_B):
        Fs, Fq = feats[b, :S].double(), feats[b, S:].double()
        ctx = text.double()[real[b].long()].unsqueeze(1)
        Fq2 = orc.context2_forward(Fq, sd, depth=depth)
        if merge_before:
            Fs, _ = orc.class_means(Fs, lab[b])
            ctx, _ = orc.class_means(ctx, lab[b])
        Fs2 = orc.context2_forward(torch.cat([Fs, ctx], dim=1), sd, depth=depth)[:, :T, :]
        if not merge_before:
            Fs2, _ = orc.class_means(Fs2, lab[b])
        nq, ns = Fq2.shape[0], Fs2.shape[0]
        sim = orc.cos_sim(Fq2.reshape(nq * T, E), Fs2.reshape(ns * T, E))
        dists = (1.0 - sim).reshape(nq, T, ns, T).permute(0, 2, 1, 3)
        c0.append(orc.otam_cum_dist(dists))
        c1.append(orc.otam_cum_dist(dists.transpose(-1, -2)))
    return torch.stack(c0), torch.stack(c1)


@gpu
@pytest.mark.parametrize("merge_before", [False, True])
@pytest.mark.parametrize("depth", [1, 2])
def test_temporal_head_vs_float64_restatement(depth, merge_before):
    from clip_fsar_amd.engine import HipTemporalHead
    sd, S, feats, text, lab, real = head_case(depth)
    c0, c1 = head_reference(depth, merge_before)
    head = HipTemporalHead(sd, HEAD_E, depth=depth, device=DEV)
    f, tx, labd, reald = guarded(feats), guarded(text), guarded(lab), guarded(real)
    for single_direct in (False, True):
        logits = head.forward(f, tx, labd, reald, HEAD_B, S, HEAD_Q, HEAD_T, HEAD_WAY, merge_before, single_direct)
        torch.cuda.synchronize()
        ref = -c0 if single_direct else -(c0 + c1)
        r = check(logits.cpu(), ref, BOUND, "temporal head depth %d merge %d single_direct %d" % (depth, merge_before, single_direct))
        print("temporal head depth %d merge %d single_direct %d: err / BOUND %.4f (|logits| up to %.2f)" % (depth, merge_before, single_direct, r,
                                                                                                          float(ref.abs().max())))
        report("temporal_head", "depth%d" % depth, r)
