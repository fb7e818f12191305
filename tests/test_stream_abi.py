"""CPU: the window-stream library (libclipfsar_stream.so, include/clipfsar_stream.h) validates arguments without a GPU; window_plan emits every
window once, in order, with the push that delivers its last frame; WindowStream's constructor errors on a stub head.  Its exports, kernels
and place in the build are checked with every library's in tests/test_build_recipe.py."""
import ctypes
import os
import random
import re
from types import SimpleNamespace as NS

import pytest

from _abi import check_exports, lib_row

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "clipfsar_stream.h")
I64 = ctypes.c_int64


@pytest.fixture(scope="module")
def slib():
    import __graft_entry__ as ge
    ge.build()                                    # builds every library (no-op when up to date)
    from clip_fsar_amd import stream_hip
    return stream_hip.lib()


def test_header_exported_exactly_and_arity_matches(slib):
    check_exports(lib_row("stream"))                 # the checks every library gets; below, what is particular to this one
    from clip_fsar_amd import stream_hip as sh
    text = open(HEADER).read()
    assert int(re.search(r"#define CFSS_MAX_T (\d+)", text).group(1)) == sh.MAX_T == 32


def test_argument_validation_without_gpu(slib):
    p = ctypes.c_void_p(4096)                     # never dereferenced: every call below fails validation before any device work
    L = slib
    err = L.cfss_last_error
    # ring_put(feats, ring, B, n, E, cap, first_frame, stream)
    assert L.cfss_ring_put(None, p, 2, 4, 64, 8, I64(0), None) != 0 and b"null" in err()
    assert L.cfss_ring_put(p, None, 2, 4, 64, 8, I64(0), None) != 0 and b"null" in err()
    for B, n, E, cap in ((0, 4, 64, 8), (2, 0, 64, 8), (2, 4, 0, 8), (2, 4, 64, 0), (-1, 4, 64, 8)):
        assert L.cfss_ring_put(p, p, B, n, E, cap, I64(0), None) != 0 and b"bad shape" in err(), (B, n, E, cap)
    assert L.cfss_ring_put(p, p, 2, 9, 64, 8, I64(0), None) != 0 and b"do not fit" in err()          # n > cap
    assert L.cfss_ring_put(p, p, 2, 4, 64, 8, I64(-1), None) != 0 and b"negative" in err()
    assert L.cfss_ring_put(p, p, 1 << 20, 4, 4096, 1 << 10, I64(0), None) != 0 and b"too large" in err()
    # window_sequences(ring, X, B, nW, T, E, cap, stride, rate, first_window, frames_pushed, stream)
    ws = L.cfss_window_sequences
    assert ws(None, p, 2, 1, 8, 64, 16, 1, 1, I64(0), I64(8), None) != 0 and b"null" in err()
    assert ws(p, None, 2, 1, 8, 64, 16, 1, 1, I64(0), I64(8), None) != 0 and b"null" in err()
    for B, nW, E, cap in ((0, 1, 64, 16), (2, 0, 64, 16), (2, 1, 0, 16), (2, 1, 64, 0)):
        assert ws(p, p, B, nW, 8, E, cap, 1, 1, I64(0), I64(8), None) != 0 and b"bad shape" in err(), (B, nW, E, cap)
    for T in (0, 33, -1):
        assert ws(p, p, 2, 1, T, 64, 64, 1, 1, I64(0), I64(64), None) != 0 and b"T=" in err(), T
    for stride in (0, -3):
        assert ws(p, p, 2, 1, 8, 64, 16, stride, 1, I64(0), I64(8), None) != 0 and b"stride" in err()
    for rate in (0, -1):
        assert ws(p, p, 2, 1, 8, 64, 16, 1, rate, I64(0), I64(8), None) != 0 and b"rate" in err()
    assert ws(p, p, 2, 1, 8, 64, 16, 1, 1, I64(-1), I64(8), None) != 0 and b"negative" in err()
    # window 0 of T = 8 needs frames 0 .. 7: 7 pushed is one short, as is window 1 with 8 pushed and frame 14 at rate 2
    assert ws(p, p, 2, 1, 8, 64, 16, 1, 1, I64(0), I64(7), None) != 0 and b"not pushed yet" in err()
    assert ws(p, p, 2, 2, 8, 64, 16, 1, 1, I64(0), I64(8), None) != 0 and b"not pushed yet" in err()
    assert ws(p, p, 2, 1, 8, 64, 16, 1, 2, I64(0), I64(14), None) != 0 and b"not pushed yet" in err()
    # cap 16, 40 pushed: the ring holds frames 24 .. 39, so window 23 (frames 23 .. 30) lost its first frame
    assert ws(p, p, 2, 1, 8, 64, 16, 1, 1, I64(23), I64(40), None) != 0 and b"already overwritten" in err()
    assert ws(p, p, 2, 3, 8, 64, 16, 4, 1, I64(5), I64(40), None) != 0 and b"already overwritten" in err()
    assert ws(p, p, 2, 1, 8, 64, 16, 3, 1, I64(2 ** 62), I64(8), None) != 0 and b"too large" in err()
    # smooth_logits(logits, state, out, B, nW, C, alpha, windows_seen, stream)
    sm = L.cfss_smooth_logits
    for args in ((None, p, p), (p, None, p), (p, p, None)):
        assert sm(*args, 2, 3, 5, 0.5, I64(0), None) != 0 and b"null" in err()
    for B, nW, C in ((0, 3, 5), (2, 0, 5), (2, 3, 0)):
        assert sm(p, p, p, B, nW, C, 0.5, I64(0), None) != 0 and b"bad shape" in err()
    for alpha in (1.0, 1.5, -0.1, float("nan"), float("inf")):
        assert sm(p, p, p, 2, 3, 5, alpha, I64(0), None) != 0 and b"alpha" in err(), alpha
    assert sm(p, p, p, 2, 3, 5, 0.5, I64(-1), None) != 0 and b"negative" in err()


def test_python_wrappers_reject_cpu_tensors(slib):
    import torch
    from clip_fsar_amd import stream_hip as sh
    with pytest.raises(RuntimeError, match="HIP device tensor"):
        sh.ring_put(torch.zeros(2, 4, 8), torch.zeros(2, 9, 8), 0)
    with pytest.raises(RuntimeError, match="shape"):
        sh.ring_put(torch.zeros(2, 4, 8), torch.zeros(3, 9, 8), 0)
    with pytest.raises(RuntimeError, match="shape"):
        sh.window_sequences(torch.zeros(2, 9, 8), torch.zeros(3, 4, 8), 2, 4, 1, 1, 0, 5)
    with pytest.raises(RuntimeError, match="shape"):
        sh.smooth_logits(torch.zeros(2, 3, 5), torch.zeros(2, 4), torch.zeros(2, 3, 5), 0.5, 0)


# ------------------------------------------------------------------ the host plan
def _brute(pushes, T, stride, rate):
    """per push: the windows k whose last frame k * stride + (T-1) * rate arrives with it"""
    total = sum(pushes)
    last = lambda k: k * stride + (T - 1) * rate
    out, t = [], 0
    for n in pushes:
        out.append([k for k in range(total + 1) if t <= last(k) < t + n])
        t += n
    return out


@pytest.mark.parametrize("T", [1, 5, 8, 16])
def test_window_plan_against_brute_force(T):
    from clip_fsar_amd.stream import window_plan
    rng = random.Random(T)
    for stride in range(1, 10):
        for rate in (1, 2, 3):
            for trial in range(4):
                pushes = [rng.choice((1, 1, 2, 3, 5, 8, 13, 40)) for _ in range(rng.randint(1, 30))]
                want = _brute(pushes, T, stride, rate)
                t, emitted = 0, []
                for n, ks in zip(pushes, want):
                    first, nW = window_plan(t, n, T, stride, rate)
                    assert first == len(emitted), (T, stride, rate, pushes)                    # the next window, also when nW == 0
                    got = list(range(first, first + nW))
                    assert got == ks, (T, stride, rate, pushes, t, n)
                    for k in got:                                                              # its last frame arrives with this push
                        assert t <= k * stride + (T - 1) * rate < t + n
                    emitted += got
                    t += n
                assert emitted == list(range(len(emitted)))                                    # once each, in order
                assert window_plan(0, t, T, stride, rate) == (0, len(emitted))                 # one big push = the pieces
    assert window_plan(0, 0, T, 1, 1) == (0, 0)
    for bad in ((-1, 1, T, 1, 1), (0, -1, T, 1, 1), (0, 1, 0, 1, 1), (0, 1, T, 0, 1), (0, 1, T, 1, 0)):
        with pytest.raises(ValueError):
            window_plan(*bad)


def test_ring_capacity_holds_every_window_a_push_completes():
    """after any push of n <= max_push frames the first frame of the first completed window is still in the ring of
    (T-1) * rate + max_push frames"""
    from clip_fsar_amd.stream import window_plan
    rng = random.Random(7)
    for T, stride, rate, max_push in ((8, 1, 1, 8), (8, 3, 2, 5), (16, 16, 1, 1), (5, 9, 3, 64), (1, 1, 1, 1)):
        cap, t = (T - 1) * rate + max_push, 0
        for _ in range(200):
            n = rng.randint(1, max_push)
            first, nW = window_plan(t, n, T, stride, rate)
            t += n
            if nW:
                assert first * stride >= t - cap and (first + nW - 1) * stride + (T - 1) * rate < t


# ------------------------------------------------------------------ constructor errors (no GPU: a stub head)
def _stub_head(T=4, **train):
    engine = NS(arch={"embed": 8})
    return NS(args=NS(TRAIN=NS(**train), DATA=NS(NUM_INPUT_FRAMES=T)), _get_engine=lambda dev: engine, _engine_key=("stub",),
              arch_name="stub", precision="fp32", depth=1)


def test_constructor_errors_on_a_stub_head():
    import torch
    from clip_fsar_amd.gallery import SupportGallery
    from clip_fsar_amd.stream import WindowStream
    from clip_fsar_amd.text_gallery import TextGallery
    g = SupportGallery(_stub_head(), "cpu")
    with pytest.raises(TypeError, match="SupportGallery or a TextGallery"):
        WindowStream(_stub_head())
    for kw in ({"n_streams": 0}, {"stride": 0}, {"rate": -1}, {"max_push": 0}, {"stride": 1.5}, {"n_streams": True}):
        with pytest.raises(ValueError, match=list(kw)[0]):
            WindowStream(g, **kw)
    for smooth in (1.0, -0.1, 2.0, float("nan")):
        with pytest.raises(ValueError, match="smooth"):
            WindowStream(g, smooth=smooth)
    with pytest.raises(ValueError, match="at most 32"):
        WindowStream(SupportGallery(_stub_head(T=33), "cpu"))
    s = WindowStream(TextGallery(_stub_head(COMBINE=True), "cpu"), n_streams=3, stride=2, rate=3, max_push=5, smooth=0.25)
    assert (s.B, s.T, s.E, s.cap) == (3, 4, 8, 3 * 3 + 5) and tuple(s._ring.shape) == (3, 14, 8)
    assert s.stats == {"frames": 0, "tower_frames": 0, "windows": 0}
    with pytest.raises(RuntimeError, match="no classes registered"):
        s.push(torch.zeros(3, 2, 3, 4, 4))
    g._ids.append(0)                              # a registered class: the push gets as far as its tensor checks
    s = WindowStream(g, n_streams=2)
    with pytest.raises(RuntimeError, match="HIP device tensor"):
        s.push(torch.zeros(2, 2, 3, 4, 4))
    with pytest.raises(RuntimeError, match="HIP device tensor"):
        s.push_features(torch.zeros(2, 2, 8))
    g.head._engine_key = ("rebuilt",)
    with pytest.raises(RuntimeError, match="changed"):
        s.push(torch.zeros(2, 2, 3, 4, 4))


def test_galleries_have_classify_features():
    import torch
    from clip_fsar_amd.gallery import SupportGallery
    from clip_fsar_amd.text_gallery import TextGallery
    for g in (SupportGallery(_stub_head(), "cpu"), TextGallery(_stub_head(EVAL_TEXT=True), "cpu")):
        with pytest.raises(RuntimeError, match="no classes registered"):
            g.classify_features(torch.zeros(1, 4, 8))
        g._ids.append(0)
        with pytest.raises(RuntimeError, match="HIP device tensor"):
            g.classify_features(torch.zeros(1, 4, 8))
