"""GPU: the text gallery (clip_fsar_amd.text_gallery.TextGallery on libclipfsar_gallery_text.so) -- the EVAL_TEXT / COMBINE kernels against
a float64 restatement and against the episode kernels, gallery probabilities against ClipFsarEngine.forward(mode=...) on the same episode
and against the reference goldens, 300 classes (beyond the episode's 64) against the oracle, zero-shot registration, incremental adds,
batch independence, top-k, state and stale engines."""
from types import SimpleNamespace as NS

import pytest
import torch

import clip_fsar_amd.synth as synth
import clipfsar_oracle as orc
from _cases import load_golden, maxdiff

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
BOUND = 2e-5              # the gallery's bound (tests/test_gpu_gallery.py)
SCALE = 4.0               # the logit scale of the reference's N4 goldens (the heads' parameter starts at 1.0)


# ------------------------------------------------------------------ helpers
def _cfg(arch, precision, T, n_train=64, n_test=24, seed=18, **extra):
    head = NS(NAME="CNN_OTAM_CLIPFSAR", BACKBONE_NAME=arch, PRECISION=precision)
    if "TEXT_TOWER" in extra:
        head.TEXT_TOWER = extra.pop("TEXT_TOWER")
    return NS(VIDEO=NS(HEAD=head, BACKBONE=NS(META_ARCH="Identity")),
              TRAIN=NS(CLASS_NAME=["c%d" % i for i in range(n_train)], WAY=5, **extra),
              TEST=NS(CLASS_NAME=["t%d" % i for i in range(n_test)]), DATA=NS(NUM_INPUT_FRAMES=T),
              MODEL=NS(NAME="BaseVideoModel", EMA=NS(ENABLE=False)), BN=NS(FREEZE=False), NUM_GPUS=1, NUM_SHARDS=1, RANDOM_SEED=seed)


_HEADS = {}


def _head(arch, precision, T, scale=SCALE, **kw):
    key = (arch, precision, T, scale, tuple(sorted(kw.items())))
    if key not in _HEADS:
        if len(_HEADS) >= 2:
            _HEADS.clear()
            torch.cuda.empty_cache()
        from clip_fsar_amd.models.base.few_shot import CNN_OTAM_CLIPFSAR
        h = CNN_OTAM_CLIPFSAR(_cfg(arch, precision, T, **kw)).eval()
        with torch.no_grad():
            h.scale.fill_(scale)
        _HEADS[key] = h
    return _HEADS[key]


def _gallery(head, mode, merge_before=False, single_direct=False, coff=None):
    from clip_fsar_amd.text_gallery import TextGallery
    head.args.TRAIN.MERGE_BEFORE = merge_before
    head.args.TRAIN.SINGLE_DIRECT = single_direct
    head.args.TRAIN.TEXT_COFF = coff
    return TextGallery(head, DEV, mode=mode)


def _episode(arch, way, shot, T, episode=0, q=1, seed=18, n_test=24):
    a = synth.ARCHS[arch]
    ep = synth.make_episode(way=way, shot=shot, query_per_class=q, frames=T, res=a["res"], n_test_classes=n_test, episode=episode, seed=seed)
    return {k: torch.from_numpy(v).to(DEV) for k, v in ep.items()}


def _gallery_vs_episode(head, ep, way, T, mode, merge_before=False, single_direct=False, coff=None):
    """(episode output [Q, way], gallery output permuted into the episode's column order [Q, way])"""
    eng = head._get_engine(DEV)
    S = ep["support_set"].shape[0] // T
    g = _gallery(head, mode, merge_before, single_direct, coff)
    lg_ep, _ = eng.forward(ep["support_set"], ep["target_set"], ep["support_labels"], ep["real_support_labels"], way=way, T=T,
                           merge_before=merge_before, single_direct=single_direct, mode=mode, text_coff=g.text_coff)
    vids = ep["support_set"].reshape(S, T, *ep["support_set"].shape[1:])
    real = [int(v) for v in ep["real_support_labels"].cpu()]
    g.add_classes(vids, real)
    Q = ep["target_set"].shape[0] // T
    lg = g.classify(ep["target_set"].reshape(Q, T, *ep["target_set"].shape[1:]))
    sl = [float(v) for v in ep["support_labels"].cpu()]
    ranks = {v: i for i, v in enumerate(sorted(set(sl)))}
    col_of = {real[s]: ranks[sl[s]] for s in range(S)}
    perm = [g.class_ids.index(cid) for cid in sorted(col_of, key=lambda c: col_of[c])]
    torch.cuda.synchronize()
    return lg_ep[0].cpu(), lg[:, perm].cpu()


def _restated(emb, text, scale, vis=None, coff=0.9):
    """float64: scale * cos (no eps) -> softmax over the classes [-> p^coff * softmax((8 + v) / 8)^(1 - coff)]"""
    e, t = emb.double(), text.double()
    logits = scale * ((e @ t.T) / e.norm(dim=1, keepdim=True) / t.norm(dim=1)[None, :])
    p = torch.softmax(logits, 1)
    if vis is None:
        return logits, p
    soft = torch.softmax((8.0 + vis.double()) / 8.0, 1)
    return logits, p.pow(coff) * soft.pow(1.0 - coff)


# ------------------------------------------------------------------ 1: the kernels
KERNEL_SHAPES = [(37, 29, 512), (16, 300, 768), (5, 7, 1024), (64, 5000, 64),
                 (5, 7, 36), (70, 65, 100), (1, 1, 4)]                           # E % 32 != 0, E < 32: the K loop's last chunk


@pytest.mark.parametrize("NQ,C,E", KERNEL_SHAPES)
def test_text_kernels_vs_float64_and_episode_kernels(NQ, C, E):
    from clip_fsar_amd import gallery_hip as gh
    from clip_fsar_amd import gallery_text_hip as gt
    from clip_fsar_amd import hip
    g = torch.Generator().manual_seed(NQ * 13 + C)
    T = 4
    base = torch.randn(E, generator=g)
    feats = ((base + 1.5 * torch.randn(NQ, T, E, generator=g)) * (0.3 + 3 * torch.rand(NQ, 1, 1, generator=g))).float()   # spread norms
    text = ((base + 1.5 * torch.randn(C, E, generator=g)) * (0.3 + 3 * torch.rand(C, 1, generator=g))).float()
    vis = -(4.0 + 8.0 * torch.rand(NQ, C, generator=g))                                  # OTAM logits = -cum
    f, tx, v = feats.to(DEV), text.to(DEV), vis.to(DEV)
    emb, en, tn = torch.empty(NQ, E, device=DEV), torch.empty(NQ, device=DEV), torch.empty(C, device=DEV)
    gt.frame_mean(f, emb)
    gh.row_norms(emb, en)
    gh.row_norms(tx, tn)
    part = torch.empty(gt.workspace_floats(NQ, C), device=DEV)
    torch.cuda.synchronize()
    e_mean = maxdiff(emb.cpu(), feats.mean(1))
    assert e_mean <= 1e-5 * float(feats.abs().max()), e_mean
    for scale in (1.0, SCALE):
        sc = torch.tensor([scale], device=DEV)
        lg = torch.empty(NQ, C, device=DEV)
        gt.text_logits(emb, en, tx, tn, sc, lg, part)
        probs = torch.empty(NQ, C, device=DEV)
        gt.text_softmax(lg, part, probs)
        ref_l, ref_p = _restated(feats.double().mean(1), text, scale)
        torch.cuda.synchronize()
        e_l = float((lg.cpu().double() - ref_l).abs().max())
        e_p = float((probs.cpu().double() - ref_p).abs().max())
        e_sum = float((probs.cpu().double().sum(1) - 1).abs().max())
        print("NQ %d C %d E %d scale %g: |dlogits| %.2e |dprobs| %.2e |row sum - 1| %.2e" % (NQ, C, E, scale, e_l, e_p, e_sum))
        assert e_l <= 1e-5 * scale, e_l
        assert e_p <= BOUND, e_p
        assert e_sum <= 1e-5, e_sum
        for coff in (0.9, 0.5):
            out = lg.clone()
            gt.text_combine(out, part, v, out, coff)                                   # in place
            _, ref_c = _restated(feats.double().mean(1), text, scale, vis, coff)
            torch.cuda.synchronize()
            e_c = float((out.cpu().double() - ref_c).abs().max())
            print("    coff %.1f: |dcombine| %.2e" % (coff, e_c))
            assert e_c <= BOUND, e_c
            if C <= 64:                                                                 # the episode kernels' limit
                fe = torch.cat([torch.zeros(C, T, E), feats]).to(DEV)                      # C one-shot supports (never read), then the queries
                lab = torch.arange(C, dtype=torch.float32, device=DEV)
                p_ep = torch.empty(1, NQ, C, device=DEV)
                hip.text_match_probs(fe, tx, lab, lab, sc, p_ep, 1, C, NQ, T, E, C)
                c_ep = torch.empty(NQ, C, device=DEV)
                hip.combine_logits(p_ep, v, c_ep, NQ, C, coff)
                torch.cuda.synchronize()
                e_pe, e_ce = maxdiff(probs.cpu(), p_ep[0].cpu()), maxdiff(out.cpu(), c_ep.cpu())
                print("    vs episode kernels: |dprobs| %.2e |dcombine| %.2e" % (e_pe, e_ce))
                assert e_pe <= BOUND and e_ce <= BOUND, (e_pe, e_ce)


# ------------------------------------------------------------------ 2: gallery = episode
EPISODE_CASES = [("ViT-test/16", "fp32", "eval_text", 1, False, False, None), ("ViT-test/16", "fp32", "eval_text", 3, False, False, None),
                 ("ViT-test/16", "bf16", "eval_text", 5, False, False, None), ("ViT-B/16", "fp32", "eval_text", 3, False, False, None),
                 ("ViT-test/16", "fp32", "combine", 1, False, False, None), ("ViT-test/16", "fp32", "combine", 5, True, False, None),
                 ("ViT-test/16", "fp32", "combine", 3, False, True, None), ("ViT-test/16", "fp32", "combine", 3, False, False, 0.5),
                 ("ViT-test/16", "bf16", "combine", 5, True, False, 0.5), ("ViT-test/16", "bf16", "combine", 1, False, True, None),
                 ("ViT-B/16", "fp32", "combine", 1, False, False, None), ("ViT-B/16", "fp32", "combine", 5, True, False, 0.5)]


@pytest.mark.parametrize("arch,precision,mode,shot,merge_before,single_direct,coff", EPISODE_CASES)
def test_gallery_equals_episode(arch, precision, mode, shot, merge_before, single_direct, coff):
    T = 8
    head = _head(arch, precision, T)
    ep = _episode(arch, 5, shot, T, episode=shot + 3 * merge_before, q=2)
    with torch.no_grad():
        lg_ep, lg = _gallery_vs_episode(head, ep, 5, T, mode, merge_before, single_direct, coff)
    d = maxdiff(lg, lg_ep)
    print("%s %s %s %d-shot mb=%d sd=%d coff=%s: |gallery - episode| = %.2e" % (arch, precision, mode, shot, merge_before, single_direct,
                                                                              coff, d))
    assert d <= BOUND, d
    assert torch.equal(lg.argmax(1), lg_ep.argmax(1))


# ------------------------------------------------------------------ 3: the reference's own logits
@pytest.mark.parametrize("case", ["n4_evaltext_5w2s_T4", "n4_combine_5w1s_T8", "n4_combine_5w3s_T4_mb_c05"])
def test_gallery_against_reference_goldens(case):
    g = load_golden(case)
    m = g["meta"]
    head = _head(m["arch"], "fp32", m["T"], scale=m["scale"], n_train=m["n_train"], n_test=m["n_test"], seed=m["seed"])
    a = synth.ARCHS[m["arch"]]
    ep = synth.make_episode(m["way"], m["shot"], m["q"], m["T"], a["res"], m["n_test"], m["episode"], m["seed"])
    ep = {k: torch.from_numpy(v).to(DEV) for k, v in ep.items()}
    with torch.no_grad():
        lg_ep, lg = _gallery_vs_episode(head, ep, m["way"], m["T"], m["mode"], m.get("merge_before", False), False, m.get("text_coff"))
    d_ref = maxdiff(lg, torch.from_numpy(g["logits"]))
    print("%s: |gallery - reference| = %.2e, |gallery - episode| = %.2e" % (case, d_ref, maxdiff(lg, lg_ep)))
    assert d_ref < 1e-4, d_ref
    assert maxdiff(lg, lg_ep) <= BOUND


# ------------------------------------------------------------------ 4: beyond the episode's 64 classes
@pytest.mark.parametrize("mode", ["eval_text", "combine"])
def test_300_classes_against_oracle(mode):
    arch, T, C, NQ = "ViT-test/16", 8, 300, 4
    head = _head(arch, "fp32", T, n_test=C)
    a = synth.ARCHS[arch]
    E = a["embed"]
    sd = {k: v.detach().float() for k, v in head.state_dict().items()}
    te = head.text_features_test.float()
    g = torch.Generator().manual_seed(300)
    V = torch.randn(C, T, 3, a["res"], a["res"], generator=g) * 0.5 + 0.2 * torch.randn(C, 1, 1, 1, 1, generator=g)
    Qv = torch.randn(NQ, T, 3, a["res"], a["res"], generator=g) * 0.5
    ids = list(torch.randperm(C, generator=g).tolist())                       # one shot per class, registered in a shuffled order
    gal = _gallery(head, mode)
    with torch.no_grad():
        gal.add_classes(V.to(DEV), ids)
        out = gal.classify(Qv.to(DEV)).cpu()
        Fq = orc.vit_forward(Qv.reshape(-1, 3, a["res"], a["res"]), sd, a).reshape(NQ, T, E)
        vis = None
        if mode == "combine":
            Fs = orc.vit_forward(V.reshape(-1, 3, a["res"], a["res"]), sd, a).reshape(C, T, E)
            ctx = te[torch.tensor(ids)].reshape(C, 1, E)
            P = orc.context2_forward(torch.cat([Fs, ctx], 1), sd)[:, :T]
            Fq2 = orc.context2_forward(Fq, sd)
            sim = orc.cos_sim(Fq2.double().reshape(NQ * T, E), P.double().reshape(C * T, E))
            d = (1.0 - sim).reshape(NQ, T, C, T).permute(0, 2, 1, 3).contiguous()
            vis = -(orc.otam_cum_dist(d) + orc.otam_cum_dist(d.transpose(-1, -2)))
        _, ref = _restated(Fq.double().mean(1), te[torch.tensor(ids)], SCALE, vis, 0.9)
    dd = maxdiff(out, ref)
    print("%d classes, %s: |gallery - oracle| = %.2e (max prob %.3f)" % (C, mode, dd, float(ref.max())))
    assert gal.class_ids == ids
    assert dd < 1e-4, dd
    if mode == "eval_text":
        assert float((out.double().sum(1) - 1).abs().max()) < 1e-5


# ------------------------------------------------------------------ 5: zero-shot classes
def test_zero_shot_classes_from_text_alone():
    import os
    from clip_fsar_amd.models.base.few_shot import CNN_OTAM_CLIPFSAR
    arch, T = "ViT-test/16", 8
    # names whose BPE merges the committed subset holds (tests/test_text_n1.py)
    bpe = os.environ.get("CLIP_BPE_PATH") or os.path.join(os.path.dirname(__file__), "golden", "bpe_merges_subset.txt.gz")
    cfg = _cfg(arch, "fp32", T, TEXT_TOWER="synthetic")
    cfg.VIDEO.HEAD.BPE_PATH = bpe
    cfg.TRAIN.CLASS_NAME = ["air drumming", "bowling", "cheerleading", "zumba", "yoga"]
    cfg.TEST.CLASS_NAME = ["busking", "unboxing", "ice skating", "side kick", "tap dancing"]
    head = CNN_OTAM_CLIPFSAR(cfg).eval()
    with torch.no_grad():
        head.scale.fill_(SCALE)
    a = synth.ARCHS[arch]
    eng = head._get_engine(DEV)
    g = torch.Generator().manual_seed(7)
    row = torch.randn(a["embed"], generator=g)
    Q = (torch.randn(6, T, 3, a["res"], a["res"], generator=g) * 0.5).to(DEV)
    calls = []
    real_forward = eng.vit.forward
    eng.vit.forward = lambda *args, **kw: (calls.append(1), real_forward(*args, **kw))[1]
    try:
        with torch.no_grad():
            gal = _gallery(head, "eval_text")
            gal.add_text_classes([3, 0], text=None)
            gal.add_text_classes(["kite", "tap"], text={"kite": row, "tap": "tap dancing"})  # an explicit row; a name through the text tower
            gal.add_classes(torch.zeros(2, T, 3, a["res"], a["res"], device=DEV), [2, 2])   # EVAL_TEXT: ids only, the tower does not run
            assert not calls, "the tower ran at registration"
            assert gal.class_ids == [3, 0, "kite", "tap", 2]
            out = gal.classify(Q).cpu()
            assert len(calls) == 1                                                        # once per query chunk
            feats = torch.empty(6 * T, a["embed"], device=DEV)
            real_forward(Q.reshape(6 * T, 3, a["res"], a["res"]), feats)
            torch.cuda.synchronize()
    finally:
        eng.vit.forward = real_forward
    te = head.text_features_test.float()
    assert maxdiff(gal._text[2].cpu(), row) == 0
    assert maxdiff(gal._text[3].cpu(), te[4]) < 1e-4                      # "tap dancing" encoded alone = TEST.CLASS_NAME[4]'s row
    _, ref = _restated(feats.cpu().double().reshape(6, T, -1).mean(1), gal._text.cpu(), SCALE)
    d = maxdiff(out, ref)
    print("zero-shot: |gallery - restatement| = %.2e" % d)
    assert d <= BOUND, d
    with torch.no_grad():
        comb = _gallery(head, "combine")
        with pytest.raises(ValueError, match="COMBINE"):
            comb.add_text_classes([1])
        with pytest.raises(ValueError, match="already registered"):
            gal.add_text_classes([0])
        with pytest.raises(ValueError, match="repeat"):
            gal.add_text_classes([1, 1])


# ------------------------------------------------------------------ 6: incremental adds, batch independence, top-k, stable ranking
@pytest.mark.parametrize("mode", ["eval_text", "combine"])
def test_incremental_batch_topk_and_ranking(mode):
    arch, T = "ViT-test/16", 8
    head = _head(arch, "fp32", T)
    a = synth.ARCHS[arch]
    g = torch.Generator().manual_seed(11)
    V = (torch.randn(12, T, 3, a["res"], a["res"], generator=g) * 0.5).to(DEV)
    ids = [0, 0, 1, 2, 2, 2, 5, 5, 7, 9, 9, 9]
    Q = (torch.randn(100, T, 3, a["res"], a["res"], generator=g) * 0.5).to(DEV)
    with torch.no_grad():
        one = _gallery(head, mode)
        one.add_classes(V, ids)
        inc = _gallery(head, mode)
        inc.add_classes(V[:6], ids[:6])
        small = inc.classify(Q)
        inc.add_classes(V[6:], ids[6:])
        assert inc.class_ids == one.class_ids == [0, 1, 2, 5, 7, 9]
        for k in ("_text", "_tn", "_P", "_pn"):
            assert torch.equal(getattr(inc, k), getattr(one, k)), k
        lb = one.classify(Q)
        assert torch.equal(inc.classify(Q), lb)
        for i in (0, 57, 99):
            l1 = one.classify(Q[i:i + 1])
            assert int(l1.argmax()) == int(lb[i].argmax())
            assert maxdiff(l1[0].cpu(), lb[i].cpu()) <= BOUND, i
        vals, idx = one.topk(Q, k=4)
        sv, si = torch.sort(lb, dim=1, descending=True, stable=True)
        assert torch.equal(vals, sv[:, :4]) and torch.equal(idx.long(), si[:, :4])
    # the order among the first 3 classes is kept after 3 more are added, wherever the values are > 0
    old, new = small.cpu(), lb[:, :3].cpu()
    order = torch.sort(old, dim=1, descending=True, stable=True).indices
    new_sorted = torch.gather(new, 1, order)
    pos = torch.gather(new > 0, 1, order)
    viol = ((new_sorted[:, 1:] > new_sorted[:, :-1]) & pos[:, 1:] & pos[:, :-1]).sum()
    assert int(viol) == 0


# ------------------------------------------------------------------ 7: state dict, stale engines
def test_state_dict_and_stale_engine():
    arch, T = "ViT-test/16", 8
    head = _head(arch, "fp32", T, seed=21)
    a = synth.ARCHS[arch]
    g = torch.Generator().manual_seed(2)
    V = (torch.randn(6, T, 3, a["res"], a["res"], generator=g) * 0.5).to(DEV)
    Q = (torch.randn(4, T, 3, a["res"], a["res"], generator=g) * 0.5).to(DEV)
    with torch.no_grad():
        for mode in ("eval_text", "combine"):
            gal = _gallery(head, mode)
            gal.add_classes(V[:5], [4, 4, 8, 8, "new"], text={"new": torch.randn(a["embed"], generator=g)})
            lg = gal.classify(Q)
            sd = gal.state_dict()
            other = _gallery(head, mode)
            other.load_state_dict(sd)
            assert torch.equal(other.classify(Q), lg)
            for bad in (dict(sd["fingerprint"], mode="combine" if mode == "eval_text" else "eval_text"),
                        dict(sd["fingerprint"], text_coff=0.5)):
                with pytest.raises(ValueError, match="fingerprint"):
                    other.load_state_dict(dict(sd, fingerprint=bad))
        head.load_state_dict(head.state_dict())               # bumps the parameters' versions: the head rebuilds its engine
        with pytest.raises(RuntimeError, match="changed"):
            gal.classify(Q)
        with pytest.raises(RuntimeError, match="changed"):
            other.add_classes(V[5:], [1])
        other.load_state_dict(sd)
        assert torch.equal(other.classify(Q), lg)
