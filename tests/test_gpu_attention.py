"""The softmax-attention kernels at their token-count edges and on hard softmaxes: cfsar_vit_attention (fp32 / bf16 / fp16, with its
_means and _pair forms), cfsar_vit_attention_cls, cfsar_seq_attention and cfsar_attnpool_attend against a float64 softmax(scale q k^T) v
of the operands AS STORED (after their rounding to the case's type), per (frame, head).

Input families (deterministic, seeded; `e` is a fixed unit vector of +-1 / sqrt(head_dim)):
  gauss   randn * 1.5 (the distribution of the older attention tests; randn for the two fp32 tail / pool kernels, as in theirs);
  spike   gauss, then per (frame, head) one query row = c e and one key row = c e with c^2 scale ~ 90: without the max subtraction exp
          overflows fp32, and the spiked query's probabilities are one-hot (the runner-up is ~ e^-70), so its output row IS the v row of the
          spiked key.  Key at token 0 for head 0, at token ntok - 1 (the last valid key of a partial tile) for the last head; the query is the
          last row of the last query tile (the class-token form spikes query 0);
  deep    q = c e + noise, k = -c e + noise: every scaled score is ~ -90 and only the noise separates the keys.  A row maximum that sees a
          padded key as 0 instead of -1e30, or misses a lane group, gives 0 / 0 or a wrong distribution here and only here;
  marker  gauss q / k, v[t, d] = (d == t % 64): the output reads back the probabilities themselves (summed over t = d mod 64), so one padded
          key let through or one real key masked moves an element by a whole probability.

The bound is a formula of the INPUTS only.  With u = 2^-8 (bf16), 2^-11 (fp16), 2^-23 (fp32), s = the unscaled scores q . k:

    tol = (3 u + 32 * 2^-23 * max|s| * log2(e) * scale) * max|v| + 1e-6          (scale = 1 / 8 for the ViT kernels)

Derivation.  The kernels compute o = sum_j p_j v_j / sum_j p_j with p_j = exp2((s_j - m) scale log2(e)) from fp32 scores.
  * A score carries an fp32 error d_s (64 products summed in fp32; we allow 32 ulps of the largest score: 32 * 2^-23 * max|s|).  exp2 sees
    d_s * scale * log2(e), so p_j is off by the relative amount eps = ln2 * d_s * scale * log2(e) <= 32 * 2^-23 * max|s| * log2(e) * scale.
    A relative error eps on every p_j moves the numerator by at most eps * max|v| * sum p and the denominator by eps * sum p; errors COMMON to
    all keys of a row (the rounded m * scale * log2(e)) cancel, so the score term enters once, not twice, to first order in the differences.
  * The 16-bit kernels round p_j to the operand type (relative u each): numerator off by at most u * max|v| * sum p, denominator by u * sum p;
    the sums themselves are fp32 on the matrix pipe.  Rounding the output to the operand type adds u * |o| <= u * max|v|.  Together 3 u max|v|.
    (fp16 probabilities below 2^-14 are subnormal and carry an ABSOLUTE error of up to 2^-25 each: at most 288 * 2^-25 ~ 9e-6 of max|v| per
    row against 3 u = 1.5e-3 -- inside the slack the rounding errors' random signs leave.)  The fp32 kernels and the class-token form keep p in
    fp32; the same formula with their u is then generous in its first term.
  * 1e-6: the flush of exp2 results below 2^-126 and of products with them.
`test_tol_holds_for_an_emulation_of_the_kernels_roundings` checks the formula on the CPU, without a GPU, against a torch emulation of exactly
these roundings (fp32 scores, p rounded to T, fp32 sums, output rounded to T) on every case of this file.  On the gauss family the fixed
tolerances of the older tests (tests/test_gpu_kernels.py) stay in force as well: the smaller of the two bounds is asserted.

Every input buffer is followed by 16 rows of NaN and every output buffer by 16 rows of a sentinel: the kernels clamp their re-reads of
padded rows to row ntok - 1, so every access stays inside the operand; a clamp that is off by one shows as a NaN in the output, a store
past the end as a changed sentinel.

Every GPU test prints its measured error beside tol (run with -s); the CPU check prints the emulation's worst error / tol per type
(0.26 for bf16 and fp16, 0.015 for fp32, 0.022 for the two fp32 tail / pool kernels).
Measured on an MI355X, worst error / tol over the cases of this file: cfsar_vit_attention bf16 0.20 (gauss 0.20, spike 0.19, deep 0.20,
marker 0.19), fp16 0.20 (0.20, 0.17, 0.16, 0.19), fp32 0.016 (0.010, 0.002, 0.011, 0.016); _cls bf16 0.26, fp16 0.26, fp32 0.004 (spike: 0 error);
_means' token means 0.44 of tol alone; cfsar_seq_attention 0.022 (deep, head_dim 128); cfsar_attnpool_attend 0.006.
"""
import functools
import math

import pytest
import torch

from _cases import maxdiff  # noqa: F401
from test_gpu_kernels import _rand, hip  # noqa: F401

gpu = pytest.mark.gpu

LOG2E = 1.4426950408889634
U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 2.0 ** -23}
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
FIXED_VIT = {torch.float32: 2e-5, torch.bfloat16: 3e-2, torch.float16: 4e-3}           # test_vit_attention
FIXED_CLS = {torch.float32: 2e-5, torch.bfloat16: 1.5e-2, torch.float16: 2e-3}         # test_vit_attention_cls
FAMILIES = ["gauss", "spike", "deep", "marker"]
SENTINEL = -77.0
GUARD = 16

NTOK_16BIT = [1, 15, 16, 17, 32, 33, 112, 113, 196, 197, 198, 208, 209, 223, 224, 225, 240, 256, 257, 258, 272, 273, 288]
NTOK_GRID = [17, 197, 225, 257]
NTOK_F32 = [1, 16, 17, 197, 257, 319, 320]
NTOK_MEANS = [16, 17, 130, 197, 208, 224, 225, 240, 257, 273, 288]
NTOK_CLS = [1, 7, 8, 9, 64, 197, 257, 319, 320]
CLS_GRIDS = [(1, 1), (2, 1), (1, 3), (2, 2), (5, 1), (5, 3)]                            # F heads = 1, 2, 3, 4, 5, 15: the last workgroup holds 1, 2, 3, 4, 1, 3 items
SEQ_SHAPES = [(1, 1), (8, 9), (9, 8), (33, 5), (128, 127)]
SEQ_HD = [8, 64, 128]
POOL_T = [1, 5, 50, 63, 64, 65, 512]
POOL_HD = [4, 8, 64, 128]


def tol_of(smax, vmax, dtype, scale=0.125):
    return (3.0 * U[dtype] + 32.0 * 2.0 ** -23 * smax * LOG2E * scale) * vmax + 1e-6


def unit_vector(hd):
    return torch.tensor([-1.0 if d % 3 == 0 else 1.0 for d in range(hd)]) / math.sqrt(hd)


def spike_key(f, h, heads, n):
    """token of the spiked key: 0 for head 0, the last token for the last head (one head: by frame parity), the middle otherwise"""
    if heads == 1:
        return 0 if f % 2 == 0 else n - 1
    return 0 if h == 0 else (n - 1 if h == heads - 1 else n // 2)


def spike_amplitude(scale):
    return math.sqrt(90.0 / scale)                                # c: c^2 scale = 90 (26.8 at scale 1 / 8: fits fp16)


# ---------------------------------------------------------------------------------------------------------------- ViT families
def vit_family(family, F_, ntok, heads, dtype, seed, spike_query=None):
    """(F, ntok, heads, dtype, seed) -> qkv [F ntok, 3 D] in `dtype` (row f ntok + t = [q | k | v] of token t, head h at columns 64 h)"""
    D = heads * 64
    x = (_rand(F_ * ntok, 3 * D, seed=seed) * 1.5).reshape(F_, ntok, 3, heads, 64).clone()
    e = unit_vector(64)
    if family == "spike":
        c = spike_amplitude(0.125)
        tq = ntok - 1 if spike_query is None else spike_query
        for f in range(F_):
            for h in range(heads):
                x[f, tq, 0, h] = c * e
                x[f, spike_key(f, h, heads, ntok), 1, h] = c * e
    elif family == "deep":
        x[:, :, 0] += 27.0 * e
        x[:, :, 1] -= 27.0 * e
    elif family == "marker":
        x[:, :, 2] = torch.eye(64)[torch.arange(ntok) % 64].reshape(1, ntok, 1, 64)
    elif family != "gauss":
        raise ValueError(family)
    return x.reshape(F_ * ntok, 3 * D).to(dtype)


def vit_reference(qkv, F_, ntok, heads):
    """float64 softmax(q k^T / 8) v per (frame, head) of the stored operands -> (ref [F ntok, D], max |q . k|, max |v|)"""
    q, k, v = qkv.double().reshape(F_, ntok, 3, heads, 64).permute(2, 0, 3, 1, 4)
    s = q @ k.transpose(-1, -2)
    ref = (torch.softmax(s * 0.125, dim=-1) @ v).permute(0, 2, 1, 3).reshape(F_ * ntok, heads * 64)
    return ref, float(s.abs().max()), float(v.abs().max())


def vit_emulation(qkv, F_, ntok, heads, round_p=True):
    """the kernels' roundings in torch on the CPU: fp32 scores, exp2 of the fp32 difference to the row maximum, P rounded to the operand type
    (round_p; the class-token form keeps it in fp32), fp32 sums, output rounded to the operand type"""
    td = qkv.dtype
    q, k, v = qkv.float().reshape(F_, ntok, 3, heads, 64).permute(2, 0, 3, 1, 4)
    s = q @ k.transpose(-1, -2)
    c = torch.tensor(0.125 * LOG2E, dtype=torch.float32)
    p = torch.exp2(s * c - s.max(dim=-1, keepdim=True).values * c)
    if round_p:
        p = p.to(td).float()
    o = (p @ v) / p.sum(dim=-1, keepdim=True)
    return o.to(td).float().permute(0, 2, 1, 3).reshape(F_ * ntok, heads * 64)


@functools.lru_cache(maxsize=None)
def vit_case(family, F_, ntok, heads, dtype, seed=41, spike_query=None):
    """one case, computed once and shared (nobody writes to it): qkv, float64 reference, tol"""
    qkv = vit_family(family, F_, ntok, heads, dtype, seed, spike_query)
    ref, smax, vmax = vit_reference(qkv, F_, ntok, heads)
    return qkv, ref, tol_of(smax, vmax, dtype)


def vit_bound(family, tol, fixed):
    return min(tol, fixed) if family == "gauss" else tol


def guarded(t, fill=float("nan")):
    """device copy of t's rows followed by GUARD rows of `fill`; -> (whole buffer, view of the leading rows)"""
    buf = torch.full((t.shape[0] + GUARD, t.shape[1]), fill, dtype=t.dtype, device="cuda")
    buf[:t.shape[0]] = t.cuda()
    return buf, buf[:t.shape[0]]


def out_buffer(rows, cols, dtype):
    """NaN rows the kernel has to fill + GUARD rows of SENTINEL it must leave alone"""
    buf = torch.full((rows + GUARD, cols), float("nan"), dtype=dtype, device="cuda")
    buf[rows:] = SENTINEL
    return buf, buf[:rows]


def check_untouched(buf, rows, what):
    assert not torch.isnan(buf[:rows].float()).any(), "%s: NaN in the output (an unwritten element, or a read past row ntok - 1)" % what
    assert bool((buf[rows:].float() == SENTINEL).all()), "%s: rows past the output were written" % what


def check_spiked_rows(rows, qkv, F_, ntok, heads, what):
    """rows [F, D]: the output row of every frame's spiked query.  It is the v row of the spiked key, to the output rounding."""
    v = qkv.double().reshape(F_, ntok, 3, heads, 64)[:, :, 2]
    o = rows.double().reshape(F_, heads, 64)
    for f in range(F_):
        for h in range(heads):
            want = v[f, spike_key(f, h, heads, ntok), h]
            diff = (o[f, h] - want).abs()
            assert bool((diff <= U[qkv.dtype] * want.abs() + 1e-9).all()), \
                "%s: frame %d head %d: the spiked query does not return the spiked key's v row (max diff %.3e)" % (what, f, h, float(diff.max()))


def run_vit(hip, family, F_, ntok, heads, dtype):
    D = heads * 64
    qkv, ref, tol = vit_case(family, F_, ntok, heads, dtype)
    _, qd = guarded(qkv)
    obuf, out = out_buffer(F_ * ntok, D, dtype)
    hip.vit_attention(qd, out, F_, ntok, D, heads)
    torch.cuda.synchronize()
    what = "vit_attention %s %s ntok=%d F=%d heads=%d" % (str(dtype).split(".")[-1], family, ntok, F_, heads)
    check_untouched(obuf, F_ * ntok, what)
    got = out.cpu()
    err = float((got.double() - ref).abs().max())
    bound = vit_bound(family, tol, FIXED_VIT[dtype])
    print("%s: err %.3e tol %.3e (asserted %.3e)" % (what, err, tol, bound))
    assert err < bound, (what, err, bound)
    if family == "spike":
        check_spiked_rows(got.view(F_, ntok, D)[:, ntok - 1], qkv, F_, ntok, heads, what)


@gpu
@pytest.mark.parametrize("ntok", NTOK_16BIT)
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_vit_attention_edges(hip, dtype, family, ntok):
    """The 16-bit kernel's four instances (197, 257, the generic <7,0,7,4> up to 224 tokens, <9,0,4,2> for 225..288) on both sides of every
    dispatch boundary, at exact multiples of the 16-key tile, one past a 16- / 32-key block, and at one token."""
    run_vit(hip, family, 2, ntok, 2, DT[dtype])


@gpu
@pytest.mark.parametrize("ntok", NTOK_GRID)
@pytest.mark.parametrize("F_,heads", [(1, 1), (3, 5)])
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_vit_attention_grid(hip, dtype, F_, heads, ntok):
    """one frame of one head, and a head index of 4, on each instance"""
    run_vit(hip, "gauss", F_, ntok, heads, DT[dtype])


@gpu
@pytest.mark.parametrize("ntok", NTOK_F32)
@pytest.mark.parametrize("family", FAMILIES)
def test_vit_attention_f32_edges(hip, family, ntok):
    """the fp32 kernel up to its limit of 320 tokens (160 KiB of LDS)"""
    run_vit(hip, family, 2, ntok, 2, torch.float32)


@gpu
def test_vit_attention_refusals(hip):
    """above 288 tokens (16-bit), above 320 (fp32, class-token form): an error, and nothing written"""
    F_, heads = 2, 2
    D = heads * 64
    for dtype, ntok, msg in ((torch.bfloat16, 289, "> 288"), (torch.float16, 289, "> 288"), (torch.float32, 321, "too large")):
        qkv = vit_family("gauss", F_, ntok, heads, dtype, 41).cuda()
        out = torch.full((F_ * ntok, D), SENTINEL, dtype=dtype, device="cuda")
        with pytest.raises(RuntimeError, match=msg):
            hip.vit_attention(qkv, out, F_, ntok, D, heads)
        torch.cuda.synchronize()
        assert bool((out == SENTINEL).all())
        if dtype == torch.float16:
            om = torch.full((F_, D), SENTINEL, dtype=torch.bfloat16, device="cuda")
            with pytest.raises(RuntimeError, match=msg):
                hip.vit_attention_means(qkv, out, om, F_, ntok, D, heads)
            pair = torch.full((F_ * ntok, 2 * D), SENTINEL, dtype=dtype, device="cuda")
            with pytest.raises(RuntimeError, match=msg):
                hip.vit_attention_pair(qkv, pair, om, F_, ntok, D, heads)
            torch.cuda.synchronize()
            assert bool((out == SENTINEL).all()) and bool((om == SENTINEL).all()) and bool((pair == SENTINEL).all())
    for dtype in (torch.bfloat16, torch.float16, torch.float32):
        qkv = vit_family("gauss", F_, 321, heads, dtype, 41).cuda()
        out = torch.full((F_, D), SENTINEL, dtype=dtype, device="cuda")
        with pytest.raises(RuntimeError, match="ntok <= 320"):
            hip.vit_attention_cls(qkv, out, F_, 321, D, heads)
        torch.cuda.synchronize()
        assert bool((out == SENTINEL).all())


# ---------------------------------------------------------------------------------------------------------------- _means / _pair
def fp16_ulp(x):
    return torch.pow(2.0, torch.floor(torch.log2(x.float().abs().clamp_min(2.0 ** -14))) - 10)


def means_bound_ok(om, mean64, tol):
    return bool(((om.double() - mean64).abs() <= tol + 2.0 ** -8 * mean64.abs()).all())


@gpu
@pytest.mark.parametrize("ntok", NTOK_MEANS)
@pytest.mark.parametrize("family", ["gauss", "spike"])
def test_vit_attention_means_edges(hip, family, ntok):
    """cfsar_vit_attention_means on every instance: the output bits of cfsar_vit_attention, the token means within the bound of
    test_vit_attention_means of the kernel's own rows, and -- new -- within tol + 2^-8 |mean| of the float64 reference's token means."""
    F_, heads = 2, 2
    D = heads * 64
    qkv, ref, tol = vit_case(family, F_, ntok, heads, torch.float16)
    _, qd = guarded(qkv)
    o0 = torch.empty(F_ * ntok, D, device="cuda", dtype=torch.float16)
    hip.vit_attention(qd, o0, F_, ntok, D, heads)
    obuf, o1 = out_buffer(F_ * ntok, D, torch.float16)
    mbuf, om = out_buffer(F_, D, torch.bfloat16)
    hip.vit_attention_means(qd, o1, om, F_, ntok, D, heads)
    torch.cuda.synchronize()
    what = "vit_attention_means f16 %s ntok=%d" % (family, ntok)
    check_untouched(obuf, F_ * ntok, what)
    check_untouched(mbuf, F_, what + " (omean)")
    assert torch.equal(o0, o1)
    own = o1.float().view(F_, ntok, D).mean(1)
    assert maxdiff(om.float(), own) < 2.0 ** -8 * max(0.05, float(own.abs().max())) + 2e-4, maxdiff(om.float(), own)
    mean64 = ref.view(F_, ntok, D).mean(1)
    err = float((om.cpu().double() - mean64).abs().max())
    print("%s: omean err %.3e tol %.3e + 2^-8 |mean| (max |mean| %.3e)" % (what, err, tol, float(mean64.abs().max())))
    assert means_bound_ok(om.cpu(), mean64, tol), (what, err, tol)


@gpu
@pytest.mark.parametrize("ntok", NTOK_MEANS)
@pytest.mark.parametrize("family", ["gauss", "spike"])
def test_vit_attention_pair_edges(hip, family, ntok):
    """cfsar_vit_attention_pair on every instance: o_hi and the means are the bits of cfsar_vit_attention_means (and so of cfsar_vit_attention),
    |o_lo| <= 1/2 ulp(o_hi), o_hi + o_lo closer to the float64 reference than o_hi (gauss; the spike family's spiked rows are exact v rows)."""
    F_, heads = 2, 2
    D = heads * 64
    qkv, ref, tol = vit_case(family, F_, ntok, heads, torch.float16)
    _, qd = guarded(qkv)
    o0 = torch.empty(F_ * ntok, D, device="cuda", dtype=torch.float16)
    hip.vit_attention(qd, o0, F_, ntok, D, heads)
    o1 = torch.empty(F_ * ntok, D, device="cuda", dtype=torch.float16)
    om1 = torch.empty(F_, D, device="cuda", dtype=torch.bfloat16)
    hip.vit_attention_means(qd, o1, om1, F_, ntok, D, heads)
    pbuf, op = out_buffer(F_ * ntok, 2 * D, torch.float16)
    mbuf, om2 = out_buffer(F_, D, torch.bfloat16)
    hip.vit_attention_pair(qd, op, om2, F_, ntok, D, heads)
    torch.cuda.synchronize()
    what = "vit_attention_pair f16 %s ntok=%d" % (family, ntok)
    check_untouched(pbuf, F_ * ntok, what)
    check_untouched(mbuf, F_, what + " (omean)")
    hi, lo = op[:, :D].contiguous(), op[:, D:].contiguous()
    assert torch.equal(hi, o1) and torch.equal(hi, o0) and torch.equal(om1, om2)
    assert bool((lo.float().abs() <= 0.5 * fp16_ulp(hi) * 1.001).all())
    mean64 = ref.view(F_, ntok, D).mean(1)
    assert means_bound_ok(om2.cpu(), mean64, tol)
    e_hi = float((hi.cpu().double() - ref).pow(2).mean().sqrt())
    e_pair = float((hi.cpu().double() + lo.cpu().double() - ref).pow(2).mean().sqrt())
    err = float((hi.cpu().double() - ref).abs().max())
    print("%s: err %.3e tol %.3e, rms o_hi %.3e, rms o_hi + o_lo %.3e" % (what, err, tol, e_hi, e_pair))
    assert err < vit_bound(family, tol, FIXED_VIT[torch.float16])
    if family == "gauss":
        assert e_pair < 0.9 * e_hi, (e_pair, e_hi)
    else:
        check_spiked_rows(hi.cpu().view(F_, ntok, D)[:, ntok - 1], qkv, F_, ntok, heads, what)


# ---------------------------------------------------------------------------------------------------------------- class-token form
def cls_case(family, F_, ntok, heads, dtype):
    """qkv with the spike on the class-token query, row 0 of the float64 reference of every frame, tol"""
    qkv, ref, tol = vit_case(family, F_, ntok, heads, dtype, 43, 0 if family == "spike" else None)
    return qkv, ref.view(F_, ntok, heads * 64)[:, 0, :], tol


def cls_split(qkv, F_, ntok, heads):
    """the separate-operand layout: q [F, D + 16], k and v [F ntok, D + 8], the extra columns NaN (rows stay 16-byte aligned)"""
    D = heads * 64
    nan = float("nan")
    x = qkv.reshape(F_, ntok, 3, D)
    q = torch.full((F_, D + 16), nan, dtype=qkv.dtype)
    q[:, :D] = x[:, 0, 0]
    k = torch.full((F_ * ntok, D + 8), nan, dtype=qkv.dtype)
    k[:, :D] = x[:, :, 1].reshape(F_ * ntok, D)
    v = torch.full((F_ * ntok, D + 8), nan, dtype=qkv.dtype)
    v[:, :D] = x[:, :, 2].reshape(F_ * ntok, D)
    return q, k, v


def run_cls_split(hip, q, k, v, out, F_, ntok, D, heads):
    """cfsar_vit_attention_cls with separate q / k / v and leading dimensions larger than D (the Python wrapper serves [k | v] only)"""
    ptr = [hip._dev(t, None, "operand") for t in (q, k, v, out)]
    assert k.shape[1] == v.shape[1]
    hip._check(hip.lib().cfsar_vit_attention_cls(ptr[0], q.shape[1], ptr[1], ptr[2], k.shape[1], ptr[3], hip._code(q.dtype),
                                                 F_, ntok, D, heads, hip._stream()), "cfsar_vit_attention_cls")


@gpu
@pytest.mark.parametrize("ntok", NTOK_CLS)
@pytest.mark.parametrize("family", ["gauss", "spike", "deep"])
@pytest.mark.parametrize("dtype", ["f32", "bf16", "f16"])
def test_vit_attention_cls_edges(hip, dtype, family, ntok):
    """cfsar_vit_attention_cls == row 0 of the float64 reference: around its 8- / 4-rows-per-instruction chunks, up to its limit of 320 tokens,
    with 1, 2, 3 and 4 items in the last workgroup, from the packed qkv matrix and from separate q / k / v with padded rows."""
    td = DT[dtype]
    for F_, heads in CLS_GRIDS:
        D = heads * 64
        qkv, ref, tol = cls_case(family, F_, ntok, heads, td)
        bound = vit_bound(family, tol, FIXED_CLS[td])
        for layout in ("packed", "split"):
            obuf, out = out_buffer(F_, D, td)
            if layout == "packed":
                _, qd = guarded(qkv)
                hip.vit_attention_cls(qd, out, F_, ntok, D, heads)
            else:
                q, k, v = cls_split(qkv, F_, ntok, heads)
                (_, qd), (_, kd), (_, vd) = guarded(q), guarded(k), guarded(v)
                run_cls_split(hip, qd, kd, vd, out, F_, ntok, D, heads)
            torch.cuda.synchronize()
            what = "vit_attention_cls %s %s ntok=%d F=%d heads=%d %s" % (dtype, family, ntok, F_, heads, layout)
            check_untouched(obuf, F_, what)
            got = out.cpu()
            err = float((got.double() - ref).abs().max())
            print("%s: err %.3e tol %.3e (asserted %.3e)" % (what, err, tol, bound))
            assert err < bound, (what, err, bound)
            if family == "spike":
                check_spiked_rows(got, qkv, F_, ntok, heads, what)


# ---------------------------------------------------------------------------------------------------------------- cfsar_seq_attention
def seq_family(family, lens, heads, hd, seed):
    """qkv [sum(lens), 3 heads hd] fp32 of sequences of the given lengths, rows [q | k | v]"""
    inner = heads * hd
    rows = sum(lens)
    x = _rand(rows, 3 * inner, seed=seed).reshape(rows, 3, heads, hd).clone()
    e = unit_vector(hd)
    c = spike_amplitude(hd ** -0.5)
    if family == "spike":
        r0 = 0
        for i, L in enumerate(lens):
            for h in range(heads):
                x[r0 + L - 1, 0, h] = c * e
                x[r0 + spike_key(i, h, heads, L), 1, h] = c * e
            r0 += L
    elif family == "deep":
        x[:, 0] += c * e
        x[:, 1] -= c * e
    elif family != "gauss":
        raise ValueError(family)
    return x.reshape(rows, 3 * inner)


def seq_reference(qkv, lens, heads, hd, emulate=False):
    """float64 reference per (sequence, head) -> (ref, max |q . k|, max |v|); emulate: the same in fp32 (the kernel's arithmetic)"""
    inner = heads * hd
    x = qkv.float() if emulate else qkv.double()
    scale = hd ** -0.5
    out, smax, r0 = [], 0.0, 0
    for L in lens:
        q, k, v = [t.reshape(L, heads, hd).transpose(0, 1) for t in x[r0:r0 + L].split(inner, dim=1)]
        s = q @ k.transpose(-1, -2)
        smax = max(smax, float(s.abs().max()))
        out.append((torch.softmax(s * scale, dim=-1) @ v).transpose(0, 1).reshape(L, inner))
        r0 += L
    return torch.cat(out).double(), smax, float(x[:, 2 * inner:].abs().max())


@functools.lru_cache(maxsize=None)
def seq_case(family, n_a, len_a, n_b, len_b, heads, hd):
    lens = (len_a,) * n_a + (len_b,) * n_b
    qkv = seq_family(family, lens, heads, hd, 47)
    ref, smax, vmax = seq_reference(qkv, lens, heads, hd)
    return qkv, lens, ref, tol_of(smax, vmax, torch.float32, hd ** -0.5)


def seq_lds_bytes(L, hd):
    """LDS of one workgroup of the kernel: q, k, v rows of hd + 1 floats and the [L][L + 1] probabilities"""
    return (3 * L * (hd + 1) + L * (L + 1)) * 4


def seq_cases():
    out = [(2, la, 3, lb, hd) for la, lb in SEQ_SHAPES for hd in SEQ_HD]
    return out + [(0, 8, 3, 9, 64), (2, 33, 0, 5, 8)]


def check_seq_spikes(got, qkv, lens, heads, hd, what):
    inner = heads * hd
    r0 = 0
    for i, L in enumerate(lens):
        for h in range(heads):
            want = qkv[r0 + spike_key(i, h, heads, L), 2 * inner + h * hd:2 * inner + (h + 1) * hd].double()
            have = got[r0 + L - 1, h * hd:(h + 1) * hd].double()
            assert bool(((have - want).abs() <= U[torch.float32] * want.abs() + 1e-9).all()), (what, i, h)
        r0 += L


@gpu
@pytest.mark.parametrize("n_a,len_a,n_b,len_b,hd", seq_cases())
@pytest.mark.parametrize("family", ["gauss", "spike", "deep"])
def test_seq_attention_edges(hip, family, n_a, len_a, n_b, len_b, hd):
    """cfsar_seq_attention (fp32, one thread per query) from one position to its limit of 128, head_dim 8 .. 128, with one of the two sequence
    groups empty.  At 128 positions the kernel's LDS (q, k, v and the probabilities of one head) passes 160 KiB from head_dim 63 on: those
    shapes are refused with a message, and that is what is asserted for them."""
    heads = 2
    qkv, lens, ref, tol = seq_case(family, n_a, len_a, n_b, len_b, heads, hd)
    inner = heads * hd
    rows = sum(lens)
    _, qd = guarded(qkv)
    obuf, out = out_buffer(rows, inner, torch.float32)
    what = "seq_attention %s n_a=%d len_a=%d n_b=%d len_b=%d hd=%d" % (family, n_a, len_a, n_b, len_b, hd)
    if seq_lds_bytes(max(len_a, len_b), hd) > 160 * 1024:
        with pytest.raises(RuntimeError, match="too large for LDS"):
            hip.seq_attention(qd, out, n_a, len_a, n_b, len_b, heads, hd, hd ** -0.5)
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all()) and bool((obuf[rows:] == SENTINEL).all())
        print("%s: refused (%d bytes of LDS)" % (what, seq_lds_bytes(max(len_a, len_b), hd)))
        return
    hip.seq_attention(qd, out, n_a, len_a, n_b, len_b, heads, hd, hd ** -0.5)
    torch.cuda.synchronize()
    check_untouched(obuf, rows, what)
    got = out.cpu()
    err = float((got.double() - ref).abs().max())
    print("%s: err %.3e tol %.3e" % (what, err, tol))
    assert err < tol, (what, err, tol)
    if family == "spike":
        check_seq_spikes(got, qkv, lens, heads, hd, what)


@gpu
def test_seq_attention_refusals(hip):
    heads = 2
    for la, lb, hd, msg in ((129, 8, 8, "max 128"), (8, 129, 8, "max 128"), (8, 9, 132, "max 128")):
        rows = 2 * la + 3 * lb
        qkv = _rand(rows, 3 * heads * hd, seed=47).cuda()
        out = torch.full((rows, heads * hd), SENTINEL, device="cuda")
        with pytest.raises(RuntimeError, match=msg):
            hip.seq_attention(qkv, out, 2, la, 3, lb, heads, hd, hd ** -0.5)
        torch.cuda.synchronize()
        assert bool((out == SENTINEL).all())


# ---------------------------------------------------------------------------------------------------------------- cfsar_attnpool_attend
def pool_family(family, Fn, T, heads, hd, seed):
    """q [Fn, C], kv [Fn T, 2 C] = [k | v], fp32"""
    C = heads * hd
    q = _rand(Fn, C, seed=seed).reshape(Fn, heads, hd).clone()
    kv = _rand(Fn * T, 2 * C, seed=seed + 1).reshape(Fn, T, 2, heads, hd).clone()
    e = unit_vector(hd)
    c = spike_amplitude(hd ** -0.5)
    if family == "spike":
        for f in range(Fn):
            for h in range(heads):
                q[f, h] = c * e
                kv[f, spike_key(f, h, heads, T), 0, h] = c * e
    elif family == "deep":
        q += c * e
        kv[:, :, 0] -= c * e
    elif family != "gauss":
        raise ValueError(family)
    return q.reshape(Fn, C), kv.reshape(Fn * T, 2 * C)


def pool_reference(q, kv, Fn, T, heads, hd, emulate=False):
    C = heads * hd
    cast = torch.Tensor.float if emulate else torch.Tensor.double
    k = cast(kv).reshape(Fn, T, 2, heads, hd)[:, :, 0].permute(0, 2, 1, 3)
    v = cast(kv).reshape(Fn, T, 2, heads, hd)[:, :, 1].permute(0, 2, 1, 3)
    s = cast(q).reshape(Fn, heads, 1, hd) @ k.transpose(-1, -2)
    ref = (torch.softmax(s * hd ** -0.5, dim=-1) @ v).reshape(Fn, C)
    return ref.double(), float(s.abs().max()), float(v.abs().max())


@functools.lru_cache(maxsize=None)
def pool_case(family, Fn, T, heads, hd):
    q, kv = pool_family(family, Fn, T, heads, hd, 53)
    ref, smax, vmax = pool_reference(q, kv, Fn, T, heads, hd)
    return q, kv, ref, tol_of(smax, vmax, torch.float32, hd ** -0.5)


@gpu
@pytest.mark.parametrize("T", POOL_T)
@pytest.mark.parametrize("hd", POOL_HD)
@pytest.mark.parametrize("family", ["gauss", "spike", "deep"])
def test_attnpool_attend_edges(hip, family, hd, T):
    """cfsar_attnpool_attend (fp32, one wave per (frame, head), 64 tokens per pass) around its 64-token passes and up to its limit of 512"""
    Fn, heads = 2, 2
    C = heads * hd
    q, kv, ref, tol = pool_case(family, Fn, T, heads, hd)
    (_, qd), (_, kd) = guarded(q), guarded(kv)
    obuf, out = out_buffer(Fn, C, torch.float32)
    hip.attnpool_attend(qd, kd, out, Fn, T, heads, hd, hd ** -0.5)
    torch.cuda.synchronize()
    what = "attnpool_attend %s T=%d hd=%d" % (family, T, hd)
    check_untouched(obuf, Fn, what)
    got = out.cpu()
    err = float((got.double() - ref).abs().max())
    print("%s: err %.3e tol %.3e" % (what, err, tol))
    assert err < tol, (what, err, tol)
    if family == "spike":
        v = kv.reshape(Fn, T, 2, heads, hd)[:, :, 1].double()
        for f in range(Fn):
            for h in range(heads):
                want = v[f, spike_key(f, h, heads, T), h]
                have = got[f, h * hd:(h + 1) * hd].double()
                assert bool(((have - want).abs() <= U[torch.float32] * want.abs() + 1e-9).all()), (what, f, h)


@gpu
def test_attnpool_attend_refusals(hip):
    Fn, heads = 2, 2
    for T, hd in ((513, 8), (5, 6)):
        C = heads * hd
        q, kv = _rand(Fn, C, seed=53).cuda(), _rand(Fn * T, 2 * C, seed=54).cuda()
        out = torch.full((Fn, C), SENTINEL, device="cuda")
        with pytest.raises(RuntimeError, match="T=%d" % T):
            hip.attnpool_attend(q, kv, out, Fn, T, heads, hd, hd ** -0.5)
        torch.cuda.synchronize()
        assert bool((out == SENTINEL).all())


# ---------------------------------------------------------------------------------------------------------------- the bound, on the CPU
def vit_cases_16bit():
    return [(fam, 2, n, 2) for fam in FAMILIES for n in NTOK_16BIT] + [("gauss", F_, n, h) for F_, h in ((1, 1), (3, 5)) for n in NTOK_GRID]


@pytest.mark.parametrize("dtype", ["bf16", "f16", "f32"])
def test_tol_holds_for_an_emulation_of_the_kernels_roundings(dtype):
    """No GPU: the kernels' roundings emulated in torch (vit_emulation) stay inside tol against float64 on every case of this file, so a GPU
    failure of the bound is the kernel's, not the formula's.  Also the token means of the emulated rows against the _means bound."""
    td = DT[dtype]
    worst = 0.0
    cases = vit_cases_16bit() if td != torch.float32 else [(fam, 2, n, 2) for fam in FAMILIES for n in NTOK_F32]
    for fam, F_, ntok, heads in cases:
        qkv, ref, tol = vit_case(fam, F_, ntok, heads, td)
        err = float((vit_emulation(qkv, F_, ntok, heads).double() - ref).abs().max())
        worst = max(worst, err / tol)
        assert err < tol, ("vit_attention", dtype, fam, F_, ntok, heads, err, tol)
    if td == torch.float16:
        for fam in ("gauss", "spike"):
            for ntok in NTOK_MEANS:
                qkv, ref, tol = vit_case(fam, 2, ntok, 2, td)
                q, k, v = qkv.float().reshape(2, ntok, 3, 2, 64).permute(2, 0, 3, 1, 4)
                s = q @ k.transpose(-1, -2)
                c = torch.tensor(0.125 * LOG2E, dtype=torch.float32)
                p = torch.exp2(s * c - s.max(dim=-1, keepdim=True).values * c).to(td).float()
                rows = ((p @ v) / p.sum(dim=-1, keepdim=True)).permute(0, 2, 1, 3).reshape(2, ntok, 128)     # unrounded fp32 rows
                om = rows.mean(1).bfloat16()
                assert means_bound_ok(om, ref.view(2, ntok, 128).mean(1), tol), ("vit_attention_means", fam, ntok)
    for fam in ("gauss", "spike", "deep"):
        for ntok in NTOK_CLS:
            for F_, heads in CLS_GRIDS:
                qkv, ref, tol = cls_case(fam, F_, ntok, heads, td)
                emu = vit_emulation(qkv, F_, ntok, heads, round_p=False).view(F_, ntok, heads * 64)[:, 0, :]
                err = float((emu.double() - ref).abs().max())
                worst = max(worst, err / tol)
                assert err < tol, ("vit_attention_cls", dtype, fam, F_, ntok, heads, err, tol)
    print("emulation %s: worst err / tol = %.3f" % (dtype, worst))


def test_tol_holds_for_fp32_arithmetic_on_the_tail_and_pool_shapes():
    """the same check for cfsar_seq_attention and cfsar_attnpool_attend: the operation in fp32 torch arithmetic against float64, inside tol"""
    worst = 0.0
    for fam in ("gauss", "spike", "deep"):
        for n_a, len_a, n_b, len_b, hd in seq_cases():
            qkv, lens, ref, tol = seq_case(fam, n_a, len_a, n_b, len_b, 2, hd)
            err = float((seq_reference(qkv, lens, 2, hd, emulate=True)[0] - ref).abs().max())
            worst = max(worst, err / tol)
            assert err < tol, ("seq_attention", fam, n_a, len_a, n_b, len_b, hd, err, tol)
        for T in POOL_T:
            for hd in POOL_HD:
                q, kv, ref, tol = pool_case(fam, 2, T, 2, hd)
                err = float((pool_reference(q, kv, 2, T, 2, hd, emulate=True)[0] - ref).abs().max())
                worst = max(worst, err / tol)
                assert err < tol, ("attnpool_attend", fam, T, hd, err, tol)
    print("fp32 emulation: worst err / tol = %.3f" % worst)
