"""GPU, end to end: HipViT's option fold_last_kv (the bf16 mode's last block without its K | V projection, libclipfsar_lastblock.so)
against the same tower with the option off, on the golden cases, and an episode's bits alone and inside a batch."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import clip_fsar_amd.synth as synth  # noqa: E402
from _cases import bound, case_inputs, load_golden, maxdiff, run_engine  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.mark.parametrize("arch", ["ViT-test/16", "ViT-test197/16", "ViT-test257/14"])
def test_option_on_equals_option_off_within_the_pruning_bound(arch):
    """the bound of test_last_block_class_token_pruning_equals_full_block for bf16: 3e-2 * max(1, |features|max)"""
    from clip_fsar_amd.engine import HipViT
    a = synth.ARCHS[arch]
    sd = {k: torch.from_numpy(v) for k, v in synth.vit_state_dict(arch, 5).items()}
    ep = synth.make_episode(frames=4, res=a["res"], seed=5, episode=0)
    frames = torch.from_numpy(ep["support_set"][:5]).cuda()
    on, off = HipViT(a, sd, precision="bf16"), HipViT(a, sd, precision="bf16", options={"fold_last_kv": False})
    assert on.fold_last_kv and not off.fold_last_kv and on.prune_last and "wk_t" in on.blocks[-1] and "wk_t" not in off.blocks[-1]
    f_on, f_off = on.forward(frames).clone(), off.forward(frames).clone()
    full = off.forward(frames, taps={}).clone()
    torch.cuda.synchronize()
    assert torch.isfinite(f_on).all()
    assert maxdiff(f_on, f_off) < 3e-2 * max(1.0, float(full.abs().max())), maxdiff(f_on, f_off)
    assert maxdiff(f_on, full) < 3e-2 * max(1.0, float(full.abs().max())), maxdiff(f_on, full)
    assert not torch.equal(f_on, f_off)                            # the option is live
    # the other precisions do not take the option
    for precision in ("fp16", "fp16_strict", "fp32"):
        assert not HipViT(a, sd, precision=precision).fold_last_kv, precision


def test_small_golden_inside_its_bf16_bound_with_the_option_on_and_off():
    name = "t197_5w1s_T2"
    g = load_golden(name)
    m = g["meta"]
    a, sd, tt, te, ep = case_inputs(m)
    l_on, _ = run_engine(m, a, sd, tt, te, [ep], "bf16", vit_options={"fold_last_kv": True})
    l_off, _ = run_engine(m, a, sd, tt, te, [ep], "bf16", vit_options={"fold_last_kv": False})
    print("fold_last_kv on %.3e off %.3e bound %.3e" % (maxdiff(l_on[0], g["logits"]), maxdiff(l_off[0], g["logits"]), bound(name, "bf16")))
    assert maxdiff(l_off[0], g["logits"]) < bound(name, "bf16")
    assert maxdiff(l_on[0], g["logits"]) < bound(name, "bf16")


def test_an_episode_alone_and_as_the_second_of_three_has_the_same_logits():
    g = load_golden("t197_5w1s_T2")
    m = g["meta"]
    a, sd, tt, te, ep0 = case_inputs(m)
    eps = [case_inputs(m, episode=m["episode"] + 1)[4], ep0, case_inputs(m, episode=m["episode"] + 2)[4]]
    l3, c3 = run_engine(m, a, sd, tt, te, eps, "bf16", vit_options={"fold_last_kv": True})
    l1, c1 = run_engine(m, a, sd, tt, te, [ep0], "bf16", vit_options={"fold_last_kv": True})
    assert torch.equal(l3[1], l1[0]) and torch.equal(c3[1], c1[0]), (maxdiff(l3[1], l1[0]), maxdiff(c3[1], c1[0]))
