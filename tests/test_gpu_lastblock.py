"""GPU: the three kernels of libclipfsar_lastblock.so (key fold -> class attend -> value fold, include/clipfsar_lastblock.h) against a
float64 CPU evaluation of the UNFOLDED definition on the same rounded inputs: LayerNorm from the row statistics handed in, K and V from
Wk', Wv' and d, softmax(q K^T / 8) V for the one query per frame.

Pass condition: no constant.  Every case also runs the two-launch path the kernels replace (cfsar_gemm_lnfold with N = 2 D into bf16 K | V
rows, then cfsar_vit_attention_cls) on the same inputs, and the new path's maximum error against the reference must not exceed that path's.
One head (D = 64) is below cfsar_gemm_lnfold's K >= 128: there the yardstick is the float64 evaluation with K and V rounded to bf16 and
the result rounded to bf16, which is a LOWER bound of that path's error (its probabilities are rounded as well).

Both paths deliver oc in bf16, and that last rounding (2^-9 relative) is most of either path's maximum error, so the ratio of the two
reads near 1.  Each case therefore also prints the new path's error BEFORE that rounding (Wv' z + d_v in float64 from the kernel's fp32 z):
that is the figure the algebra is about.  Measured on an MI355X over the cases below: after oc's rounding today's error is 1.0 ... 1.9
times the new path's (1.0 in 26 of 46 lines: the same element's rounding); before it, 9 ... 43 times on the plain cases, 144 ... 358 times
with the outlier channels, and 3e4 and more where one token takes the whole softmax (the new path is then exact to 2e-7).

Shapes: heads 1, 2, 12, 16; token counts 1, 2, 17, 197, 257 and c - 1, c, c + 1, 2 c + 1 around the token chunk c = CFLB_TOKEN_CHUNK;
frame counts 1, 3 and b - 1, b, b + 1 around the folds' frame batch b = CFLB_FRAME_BATCH; both statistics forms."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

C, B = 32, 16          # CFLB_TOKEN_CHUNK, CFLB_FRAME_BATCH (asserted below)
EPS = 1e-5


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def test_the_edges_are_the_kernels_constants():
    from clip_fsar_amd import lastblock_hip as lb
    assert (lb.TOKEN_CHUNK, lb.FRAME_BATCH) == (C, B)


_WEIGHTS = {}


def weights(heads, kscale=1.0):
    """(Wk', Wv' fp16 [D, D], d_k, d_v fp32 [D]) of a head count, made once"""
    key = (heads, kscale)
    if key not in _WEIGHTS:
        D = 64 * heads
        gen = torch.Generator().manual_seed(1000 + heads)
        wk = (torch.randn(D, D, generator=gen) * (kscale / math.sqrt(D))).to(torch.float16)
        wv = (torch.randn(D, D, generator=gen) / math.sqrt(D)).to(torch.float16)
        dk, dv = torch.randn(D, generator=gen) * 0.3, torch.randn(D, generator=gen) * 0.3
        _WEIGHTS[key] = (wk, wv, dk, dv)
    return _WEIGHTS[key]


def make_case(heads, ntok, F, form, seed=0, kscale=1.0, peak=None, outliers=False, flat_stats=False):
    """the rounded inputs of a case, on the CPU.  form: "part" (the producer's raw partial sums, slots = D / 64) or "rstat" (finalized
    rows).  peak = token: that token's row of every frame is moved along the frame's summed key direction (hard softmax).  outliers: two
    channels offset by +60 and -35.  flat_stats: the statistics handed in are the SAME (mean, sd) for every row (not the rows' own), so
    that a change of G shifts every score of a head by one constant."""
    D = 64 * heads
    wk, wv, dk, dv = weights(heads, kscale)
    gen = torch.Generator().manual_seed(7 * seed + 13 * heads + 101 * ntok + F)
    x = torch.randn(F * ntok, D, generator=gen) * (0.5 + torch.rand(F * ntok, 1, generator=gen)) + 0.4 * torch.randn(F * ntok, 1, generator=gen)
    q = torch.randn(F, D, generator=gen).to(torch.bfloat16)
    if outliers:
        x[:, 3] += 60.0
        x[:, D - 7] -= 35.0
    if peak is not None:
        g = torch.einsum("fhj,hjk->fk", q.double().view(F, heads, 64), wk.double().view(heads, 64, D))      # sum over heads of Wk'_h^T q_h
        x.view(F, ntok, D)[:, peak] = (4.0 * g / g.std(1, keepdim=True)).float()
    x = x.to(torch.float16)
    xf = x.float()
    part = torch.stack([xf.view(-1, heads, 64).sum(2), (xf * xf).view(-1, heads, 64).sum(2)], 2).contiguous()         # [M, slots, 2]
    s, ss = part[:, :, 0].double().sum(1), part[:, :, 1].double().sum(1)
    mean = s / D
    sd = ((ss / D - mean * mean).clamp_min(0) + EPS).sqrt()
    if flat_stats:
        mean, sd = torch.full_like(mean, 0.37), torch.full_like(sd, 1.21)
        form = "rstat"
    rstat = torch.stack([mean, sd, 1 / sd, torch.zeros_like(sd)], 1).float().contiguous()
    return dict(heads=heads, D=D, ntok=ntok, F=F, form=form, x=x, q=q, wk=wk, wv=wv, dk=dk, dv=dv, part=part, rstat=rstat)


def reference(c, round_kv=False):
    """float64: (o [F, D], p [F, heads, ntok]).  The statistics are the ones handed in: rstat's (mean, sd) -- with form "part" they are
    the partials' sums through cfsar_ln_stats_finalize's formula, which make_case put into rstat as well.  round_kv: K and V through bf16."""
    F, N, H, D = c["F"], c["ntok"], c["heads"], c["D"]
    mean, sd = c["rstat"][:, 0].double(), c["rstat"][:, 1].double()
    xh = (c["x"].double() - mean[:, None]) / sd[:, None]
    K = xh @ c["wk"].double().t() + c["dk"].double()
    V = xh @ c["wv"].double().t() + c["dv"].double()
    if round_kv:
        K, V = K.to(torch.bfloat16).double(), V.to(torch.bfloat16).double()
    K, V = K.view(F, N, H, 64), V.view(F, N, H, 64)
    s = torch.einsum("fhj,fnhj->fhn", c["q"].double().view(F, H, 64), K) / 8
    p = torch.softmax(s, 2)
    return torch.einsum("fhn,fnhj->fhj", p, V).reshape(F, D), p


def run_new(c, frames=None, G_shift=0.0, want_z=False):
    """key fold -> class attend -> value fold on the GPU, oc [F, D] bf16 (want_z: z [F, heads, D] fp32) on the CPU (frames: the first
    `frames` frames alone)"""
    from clip_fsar_amd import lastblock_hip as lb
    F, N, H, D = c["F"] if frames is None else frames, c["ntok"], c["heads"], c["D"]
    dev = torch.device("cuda")
    x, q = c["x"][:F * N].to(dev), c["q"][:F].to(dev)
    g, G = torch.empty(F, H, D, device=dev, dtype=torch.float16), torch.empty(F, H, device=dev)
    z, oc = torch.empty(F, H, D, device=dev), torch.empty(F, D, device=dev, dtype=torch.bfloat16)
    lb.key_fold(q, lb.key_weight(c["wk"].to(dev), H), g, G)
    if G_shift:
        G += G_shift
    if c["form"] == "part":
        lb.class_attend(x, g, G, z, N, partial=c["part"][:F * N].to(dev), eps=EPS)
    else:
        lb.class_attend(x, g, G, z, N, rowstats=c["rstat"][:F * N].to(dev), eps=EPS)
    lb.value_fold(z, c["wv"].to(dev), c["dv"].to(dev), oc)
    torch.cuda.synchronize()
    return (z.cpu() if want_z else oc.cpu())


def run_today(c):
    """the two launches the kernels replace: K | V rows in bf16 from the LN-folded GEMM (statistics finalized first when they come as
    partials, as the engine does without fuse_stats), then the class-token attention kernel.  One head: None (K = 64 < 128)."""
    from clip_fsar_amd import hip
    F, N, H, D = c["F"], c["ntok"], c["heads"], c["D"]
    if D < 128:
        return None
    dev = torch.device("cuda")
    M = F * N
    x, q = c["x"].to(dev), c["q"].to(dev)
    wg = torch.cat([c["wk"], c["wv"]]).contiguous().to(dev)
    cvec = torch.cat([c["wk"], c["wv"]]).double().sum(1).float().to(dev)
    dvec = torch.cat([c["dk"], c["dv"]]).to(dev)
    if c["form"] == "part":
        rstat = torch.empty(M, 4, device=dev)
        hip.ln_stats_finalize(c["part"].to(dev), rstat, M, H, D, eps=EPS)
    else:
        rstat = c["rstat"].to(dev)
    kv = torch.empty(M, 2 * D, device=dev, dtype=torch.bfloat16)
    oc = torch.empty(F, D, device=dev, dtype=torch.bfloat16)
    hip.gemm_lnfold(x, wg, kv, cvec, dvec, rstat, M=M)
    hip.vit_attention_cls(None, oc, F, N, D, H, q=q, kv=kv)
    torch.cuda.synchronize()
    return oc.cpu()


def check(c, label):
    """the pass condition; -> (error of the new path, error of today's, the reference's peak probability)"""
    ref, p = reference(c)
    new, old = run_new(c), run_today(c)
    if old is None:
        old = reference(c, round_kv=True)[0].to(torch.bfloat16)
    e_new, e_old = float((new.double() - ref).abs().max()), float((old.double() - ref).abs().max())
    z = run_new(c, want_z=True).double().view(c["F"], c["heads"], c["D"])
    pre = torch.einsum("fhk,hjk->fhj", z, c["wv"].double().view(c["heads"], 64, c["D"])).reshape(c["F"], c["D"]) + c["dv"].double()
    e_pre = float((pre - ref).abs().max())
    print("lastblock %-28s heads %2d ntok %3d F %2d %-5s  new %.3e  today %.3e  ratio %.1f  new before oc's rounding %.3e  ratio %.0f  "
          "peak p %.3f" % (label, c["heads"], c["ntok"], c["F"], c["form"], e_new, e_old, e_old / max(e_new, 1e-30), e_pre,
                           e_old / max(e_pre, 1e-30), float(p.max())))
    assert torch.isfinite(new.float()).all()
    assert e_new <= e_old, (label, e_new, e_old)
    return e_new, e_old, float(p.max())


FORMS = ("part", "rstat")


@pytest.mark.parametrize("ntok", [1, 2, 17, C - 1, C, C + 1, 2 * C + 1, 197, 257])
def test_token_counts_two_heads(ntok):
    check(make_case(2, ntok, 3, FORMS[ntok % 2]), "ntok")
    check(make_case(2, ntok, 3, FORMS[(ntok + 1) % 2], seed=1), "ntok, the other form")


@pytest.mark.parametrize("F", [1, 3, B - 1, B, B + 1])
def test_frame_counts_around_the_fold_batch(F):
    check(make_case(2, C + 1, F, FORMS[F % 2]), "frames")


@pytest.mark.parametrize("heads,ntok,F,form", [(1, C + 1, 3, "rstat"), (1, 2, 1, "part"), (12, 197, 3, "part"), (12, 2 * C + 1, 2, "rstat"),
                                               (16, 257, 2, "part"), (16, C + 1, B + 1, "rstat")])
def test_head_counts(heads, ntok, F, form):
    check(make_case(heads, ntok, F, form), "heads")


@pytest.mark.parametrize("heads", [2, 12])
@pytest.mark.parametrize("ntok,peak,where", [(2 * C + 1, 5, "first chunk"), (2 * C + 1, 2 * C - 3, "last whole chunk"),
                                             (C + 1, C, "alone after a chunk of smaller scores")])
def test_hard_softmax_takes_every_rescale_step(heads, ntok, peak, where):
    """Wk' scaled by 6 and one token along the key direction: a peak probability above 0.9.  Peak first: the later chunks are added at a
    maximum they do not move; peak in a later chunk or alone in the last one: what was accumulated before is rescaled by exp of a large
    negative number."""
    for form in FORMS:
        c = make_case(heads, ntok, 3, form, kscale=6.0, peak=peak)
        _, _, pmax = check(c, "hard softmax, " + where)
        assert pmax > 0.9, pmax
        p = reference(c)[1]
        assert int(p.view(-1, ntok)[p.view(-1, ntok).max(1).values.argmax()].argmax()) == peak


@pytest.mark.parametrize("heads,ntok,form", [(2, C + 1, "part"), (12, 197, "rstat"), (16, 2 * C + 1, "part")])
def test_outlier_channels(heads, ntok, form):
    check(make_case(heads, ntok, 3, form, outliers=True), "outlier channels +60 / -35")


@pytest.mark.parametrize("heads,ntok", [(2, 2 * C + 1), (12, 197)])
def test_constant_score_shift_leaves_z(heads, ntok):
    """With the same (mean, sd) handed in for every row, G + delta shifts every score of a head by -mean delta / sd, a constant the softmax
    cancels.  z may move by the rounding of the weights alone: they are fp16 values (relative step 2^-11), normalised by their own sum, so
    |dz| <= 2 * 2^-11 * max |x_hat| however many of them round the other way; the fp32 rounding of the shifted scores is far below that."""
    c = make_case(heads, ntok, 3, "rstat", flat_stats=True)
    check(c, "flat statistics")
    z0, z1 = run_new(c, want_z=True), run_new(c, G_shift=5.0, want_z=True)             # every score moves by -0.37 * 5 / 1.21 = -1.53
    xh_max = float(((c["x"].double() - 0.37) / 1.21).abs().max())
    d = float((z0 - z1).abs().max())
    print("lastblock constant shift: heads %d ntok %d  max |dz| %.3e  bound %.3e" % (heads, ntok, d, 2 * 2.0 ** -11 * xh_max))
    assert torch.isfinite(z1).all() and d <= 2 * 2.0 ** -11 * xh_max, d


@pytest.mark.parametrize("heads,ntok", [(2, C + 1), (12, 197)])
def test_frame_0_has_the_same_bits_alone_and_in_a_batch(heads, ntok):
    c = make_case(heads, ntok, B + 1, "part")
    alone, batch = run_new(c, frames=1), run_new(c)
    assert torch.equal(alone[0].view(torch.int16), batch[0].view(torch.int16))
    again = run_new(c)
    assert torch.equal(again.view(torch.int16), batch.view(torch.int16))
