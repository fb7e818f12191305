"""GPU: the still-frame gate (clip_fsar_amd.pool.StreamPool(still=StillGate(...)) on libclipfsar_still.so) -- cfsk_changed through its
binding against clip_fsar_amd.still.reference_changed bit for bit at every frame length that takes another path (one piece, no multiple
of 4, one chunk, a chunk and a tail, a 224 x 224 frame, frames past element 2^31), aligned and one float off, with planted NaN, inf and
signed zeros; cfsk_pack and cfsk_expand against torch indexing between sentinels; then the pool on the test tower over streams with
repeats: the tower sees exactly the frames plan_still keeps, every output equals a twin pool fed the recorded tower rows, and lies
within the gallery's batch bound of a twin that ran the tower on every frame; tolerances; and one pool with every other option on."""
import pytest
import torch

from test_gpu_stream import BOUND, DEV, _filled, _frames, _head

pytestmark = pytest.mark.gpu

F_SENTINEL, I_SENTINEL = -12345.0, -77
INF, NAN = float("inf"), float("nan")
ARCH, T = "ViT-test/16", 8


def _padded(t, pad=64):
    """t inside a larger buffer with `pad` sentinels on either side -> (buffer, the view holding t).  pad = 64: the view is 16-byte
    aligned as the buffer is; pad = 65: one float off"""
    sentinel = I_SENTINEL if t.dtype == torch.int32 else F_SENTINEL
    buf = torch.full((t.numel() + 2 * pad,), sentinel, dtype=t.dtype, device=DEV)
    view = buf[pad:pad + t.numel()].view(t.shape)
    view.copy_(t)
    return buf, view


def _intact(buf, pad=64):
    sentinel = I_SENTINEL if buf.dtype == torch.int32 else F_SENTINEL
    return bool((buf[:pad] == sentinel).all()) and bool((buf[-pad:] == sentinel).all())


def _bits(t):
    return t.contiguous().view(torch.int32)


def _uploader(max_streams):
    from clip_fsar_amd import pool_hip as ph
    from clip_fsar_amd import still_hip as sk
    return ph.TableUploader(DEV, max_streams, cols=sk.TABLE_COLS)


def _sixtyfourths(shape, g, span=64):
    """multiples of 1/64 in [-1, 1]: every difference of two of them is exact in fp32"""
    return torch.randint(-span, span + 1, shape, generator=g).float() / 64


# ------------------------------------------------------------------ 1: the change counts
#        slot f0 n last_pos: three sessions, the middle one without a predecessor; slots 1 and 4 of the store are nobody's
ROWS = [[2, 0, 3, 5], [0, 3, 1, -1], [3, 4, 4, 0]]
MS, NF = 5, 8


def _changed_world(L, seed):
    """frames [NF, L] and prev [MS, L]: every frame its predecessor with some elements moved by 1/64 .. 8/64 (frame 2 an exact repeat),
    then NaN, inf and signed zeros planted where L has room"""
    g = torch.Generator().manual_seed(seed)
    prev = _sixtyfourths((MS, L), g)
    prev[0] = NAN                                  # the session without a predecessor: its row of the store is never read
    frames = torch.empty(NF, L)
    for slot, f0, n, last_pos in ROWS:
        y = prev[slot] if last_pos >= 0 else _sixtyfourths((L,), g)
        for i in range(f0, f0 + n):
            step = torch.randint(1, 9, (L,), generator=g).float() / 64 * (torch.rand(L, generator=g) < 0.3)
            frames[i] = y + (0 if i == 2 else step)
            y = frames[i]
    if L >= 75:
        at = lambda k: (k * 37 + 5) % L
        frames[0, at(0)], prev[2, at(0)] = NAN, NAN              # NaN against NaN: changed
        frames[1, at(1)] = NAN                                   # a NaN arriving, and (frame 2 against it) a NaN leaving
        frames[4, at(2)], prev[3, at(2)] = INF, INF              # inf - inf
        frames[5, at(3)], frames[4, at(3)] = -INF, INF
        frames[6, at(4)], frames[5, at(4)] = 0.0, -0.0           # signed zeros: not changed
        frames[6, at(5)], frames[5, at(5)] = -0.0, 0.0
        frames[7, at(6)], frames[6, at(6)] = INF, INF
    return frames, prev


def _run_changed(frames, prev, rows, tol, pad=64, max_streams=MS):
    from clip_fsar_amd import still_hip as sk
    n, L = frames.shape
    f_buf, f_d = _padded(frames, pad)
    p_buf, p_d = _padded(prev, pad)
    c_buf, c_d = _padded(torch.full((n,), 99, dtype=torch.int32))
    w_buf, w_d = _padded(torch.full((sk.workspace_ints(n, L),), 55, dtype=torch.int32))
    up = _uploader(max_streams)
    runs = []
    for again in range(2):                         # two runs: identical bytes
        c_d.fill_(99)
        sk.changed(f_d, p_d, c_d, w_d, up.upload(rows), tol)
        runs.append((c_d.clone(), w_d.clone()))
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    for buf, p in ((f_buf, pad), (p_buf, pad), (c_buf, 64), (w_buf, 64)):
        assert _intact(buf, p)
    assert torch.equal(_bits(f_d.cpu()), _bits(frames)) and torch.equal(_bits(p_d.cpu()), _bits(prev))      # the inputs are only read
    return c_d.cpu()


@pytest.mark.parametrize("pad", [64, 65])          # 65: both bases one float off 16 bytes -- the 4-byte form at L % 4 == 0 too
@pytest.mark.parametrize("L", [1, 3, 75, 256, 1028, 12288])
def test_changed_is_reference_changed(L, pad):
    from clip_fsar_amd.still import reference_changed
    frames, prev = _changed_world(L, 100 + L)
    seen = set()
    for tol in (0.0, 3 / 64, 0.05):                # 0.05: no multiple of 1/64, rounded to fp32 on the way in
        got = _run_changed(frames, prev, ROWS, tol, pad)
        want = reference_changed(frames, prev, ROWS, tol)
        assert got.dtype == torch.int32 and torch.equal(got, want), (tol, got.tolist(), want.tolist())
        assert got[3].item() == -1 and got[2].item() == (0 if L < 75 else 1)     # no predecessor; the exact repeat (but for the NaN that left)
        seen |= set(got.tolist())
    assert len(seen) > 3 or L < 75


def test_changed_on_a_224_frame_and_a_single_session():
    from clip_fsar_amd.still import reference_changed
    L = 3 * 224 * 224                              # 150 528: 18 whole chunks and a tail of 3 072 elements
    g = torch.Generator().manual_seed(9)
    prev = _sixtyfourths((2, L), g)
    frames = prev[1].repeat(4, 1)
    frames[0, ::5001] += 1 / 64                    # 31 elements, a few in every region of the frame
    frames[1] = frames[0]
    frames[2] = frames[1] + (torch.rand(L, generator=g) < 0.5) * (2 / 64)
    frames[3] = frames[2]
    frames[3, L - 1] = NAN                         # the last element of the tail
    rows = [[1, 0, 4, 0]]
    for tol in (0.0, 1 / 64, 2 / 64):
        got = _run_changed(frames, prev, rows, tol, max_streams=2)
        assert torch.equal(got, reference_changed(frames, prev, rows, tol)), tol
    assert got.tolist() == [0, 0, 0, 1]
    assert _run_changed(frames, prev, rows, 0.0, max_streams=2)[:2].tolist() == [31, 0]


def test_frames_past_element_two_to_the_31():
    """one session of 14 300 frames of 224 x 224: the last frames lie beyond element 2^31 of the packed frames.  All zeros but for
    planted elements, so the counts, the packed rows and the store are known without a reference over 8 GiB."""
    from clip_fsar_amd import still_hip as sk
    L, n = 3 * 224 * 224, 14300
    assert (n - 3) * L > 1 << 31
    frames = torch.zeros(n, L, device=DEV)
    frames[n - 3, 7:12] = 1.0                      # 5 elements arrive in frame n - 3 and leave in frame n - 2
    frames[n - 1, L - 3:] = 2.0                    # 3 arrive in the last frame
    frames[1, 100] = 3.0                           # and, below 2^31, 1 in frame 1
    prev = torch.full((1, L), -1.0, device=DEV)
    counts = torch.full((n,), 99, dtype=torch.int32, device=DEV)
    work = torch.empty(sk.workspace_ints(n, L), dtype=torch.int32, device=DEV)
    table = _uploader(1).upload([[0, 0, n, -1]])
    sk.changed(frames, prev, counts, work, table, 0.0)
    want = torch.zeros(n, dtype=torch.int32)
    want[0], want[1], want[2], want[n - 3], want[n - 2], want[n - 1] = -1, 1, 1, 5, 5, 3
    assert torch.equal(counts.cpu(), want)
    kept = [1, n - 3, n - 1]
    packed = torch.full((3, L), -5.0, device=DEV)
    sk.pack(frames, packed, prev, sk.ListUploader(DEV).upload(kept), table)
    assert torch.equal(packed, frames[kept]) and torch.equal(prev[0], frames[n - 1])
    assert packed[1].sum().item() == 5.0 and prev.sum().item() == 6.0


# ------------------------------------------------------------------ 2: pack and expand
@pytest.mark.parametrize("pad", [64, 65])
@pytest.mark.parametrize("L", [3, 256, 12288])
def test_pack_against_torch_indexing(L, pad):
    from clip_fsar_amd import still_hip as sk
    g = torch.Generator().manual_seed(L)
    frames = torch.randn(NF, L, generator=g)
    prev0 = torch.randn(MS, L, generator=g)
    up, lists = _uploader(MS), sk.ListUploader(DEV)
    for kept in ([1, 2, 6], [0], [7], list(range(1, NF)), [], list(range(NF))):
        NK = len(kept)
        f_buf, f_d = _padded(frames, pad)
        p_buf, p_d = _padded(prev0, pad)
        k_buf, k_d = _padded(torch.full((max(NK, 1), L), 7.0), pad)
        packing = 0 < NK < NF
        sk.pack(f_d, k_d[:NK] if packing else None, p_d, lists.upload(kept) if packing else sk.List(None, None, NK), up.upload(ROWS))
        want = prev0.clone()
        for slot, f0, n, _ in ROWS:
            want[slot] = frames[f0 + n - 1]        # slots 1 and 4 are in no row: untouched
        assert torch.equal(_bits(p_d.cpu()), _bits(want)), kept
        if packing:
            assert torch.equal(_bits(k_d.cpu()), _bits(frames[kept])), kept
        else:
            assert bool((k_d == 7.0).all())        # nothing is packed when no frame or every frame is kept
        assert _intact(f_buf, pad) and _intact(p_buf, pad) and _intact(k_buf, pad)
        assert torch.equal(_bits(f_d.cpu()), _bits(frames))


@pytest.mark.parametrize("pad", [64, 65])
@pytest.mark.parametrize("E", [4, 64, 66, 512])
def test_expand_against_torch_indexing(E, pad):
    from clip_fsar_amd import still_hip as sk
    g = torch.Generator().manual_seed(E)
    cap = 11
    ring = torch.randn(MS, cap, E, generator=g)
    up, lists = _uploader(MS), sk.ListUploader(DEV)
    #         session 0 (last_pos 5)  1 (none)  2 (last_pos 0)
    for src in ([-1, 0, 0, 1, -1, -1, 2, 2],       # skipped frames before a session's first kept one read the ring
                [-1, -1, -1, 0, -1, -1, -1, -1],   # only the session without a predecessor keeps a frame
                [0, 1, 2, 3, 4, 5, 6, 7],          # NK = N
                [0, 0, 0, 1, 1, 1, 1, 1]):
        NK = max(src) + 1
        kept_feats = torch.randn(NK, E, generator=g)
        r_buf, r_d = _padded(ring, pad)
        k_buf, k_d = _padded(kept_feats, pad)
        o_buf, o_d = _padded(torch.full((NF, E), 7.0), pad)
        sk.expand(k_d, r_d, o_d, lists.upload(src), up.upload(ROWS))
        want = torch.empty(NF, E)
        for slot, f0, n, last_pos in ROWS:
            for i in range(f0, f0 + n):
                want[i] = kept_feats[src[i]] if src[i] >= 0 else ring[slot, last_pos]
        assert torch.equal(_bits(o_d.cpu()), _bits(want)), src
        assert _intact(r_buf, pad) and _intact(k_buf, pad) and _intact(o_buf, pad)
        assert torch.equal(_bits(r_d.cpu()), _bits(ring)) and torch.equal(_bits(k_d.cpu()), _bits(kept_feats))
    # NK = 0: every frame reads the ring, and there are no kept rows to pass
    rows = [[2, 0, 3, 5], [3, 3, 5, 0]]
    o_buf, o_d = _padded(torch.full((NF, E), 7.0), pad)
    r_buf, r_d = _padded(ring, pad)
    sk.expand(None, r_d, o_d, lists.upload([-1] * NF), up.upload(rows))
    assert torch.equal(o_d.cpu(), torch.cat([ring[2, 5].expand(3, E), ring[3, 0].expand(5, E)])) and _intact(o_buf, pad)
    with pytest.raises(RuntimeError, match=r"cfsk_expand: src\[3\]=-1 in row 1"):
        sk.expand(None, r_d, o_d, lists.upload([-1] * NF), up.upload(ROWS))


# ------------------------------------------------------------------ 3: the pool
class _Model:
    """The test's own bookkeeping of a gated pool: per session the newest frame of its last pixel push, whether it counts as a
    predecessor, the run of skipped frames and the tower row of its newest frame -- and from them, per push, the keep pattern
    (plan_still over reference_changed on the CPU) and the features the pool must hand to _run."""

    def __init__(self, gate, L, E):
        self.gate, self.L, self.E, self.s = gate, L, E, {}

    def open(self, h):
        self.s[h] = dict(prev=None, run=0, feat=None, tower=0, still=0)

    reset = open

    def plan(self, frames, handles, counts):
        from clip_fsar_amd.still import plan_still, reference_changed
        flat = frames.reshape(frames.shape[0], -1).cpu()
        prev = torch.stack([self.s[h]["prev"] if self.s[h]["prev"] is not None else torch.full((self.L,), NAN) for h in handles])
        rows, f0 = [], 0
        for j, (h, n) in enumerate(zip(handles, counts)):
            rows.append((j, f0, n, 0 if self.s[h]["prev"] is not None else -1))
            f0 += n
        changed = reference_changed(flat, prev, rows, self.gate.tol)
        kept, src, runs = plan_still(changed.tolist(), rows, [self.s[h]["run"] for h in handles], self.gate.limit(self.L), self.gate.max_run)
        return flat, rows, kept, src, runs

    def expand(self, plan, handles, tower_rows):
        """the push's [N, E] features from the rows the tower returned for its kept frames; commits the push"""
        flat, rows, kept, src, runs = plan
        feats = torch.empty(flat.shape[0], self.E, device=DEV)
        pattern = {}
        for (j, f0, n, _), h, run in zip(rows, handles, runs):
            st = self.s[h]
            for i in range(f0, f0 + n):
                feats[i] = tower_rows[src[i]] if src[i] >= 0 else st["feat"]
            mine = tuple(i in kept for i in range(f0, f0 + n))
            pattern[h] = mine
            st.update(prev=flat[f0 + n - 1].clone(), run=run, feat=feats[f0 + n - 1].clone(), tower=st["tower"] + sum(mine),
                      still=st["still"] + n - sum(mine))
        return feats, pattern

    def features_pushed(self, h, feats):
        self.s[h].update(prev=None, run=0, feat=feats[-1].clone())


def _same_outputs(x, y):
    assert x.sessions == y.sessions and x.first_window == y.first_window and x.offsets == y.offsets and type(x) is type(y)
    for name in ("logits", "smoothed", "deviation", "tempo"):
        u, v = getattr(x, name, None), getattr(y, name, None)
        assert (u is None) == (v is None) and (u is None or torch.equal(_bits(u), _bits(v))), name


class _Trio:
    """the gated pool, its twin fed the recorded tower rows through push_features_packed, and (full=True) a twin that runs the tower on
    every frame -- driven together; `seen` records every tower call of the gated pool: (frames in, rows out)"""

    def __init__(self, gal, gate, monkeypatch, full=True, **kw):
        from clip_fsar_amd.pool import StreamPool
        self.gated = StreamPool(gal, still=gate, **kw)
        self.twin = StreamPool(gal, **kw)
        self.full = StreamPool(gal, **kw) if full else None
        self.pools = [p for p in (self.gated, self.twin, self.full) if p is not None]
        self.eng = gal._fresh_engine()
        self.model = _Model(gate, 3 * 64 * 64, gal.E)
        self.seen, self.recording = [], False
        real = self.eng.vit.forward

        def forward(x, out, *a, **k):
            r = real(x, out, *a, **k)
            if self.recording:
                self.seen.append((x.shape[0], out.clone()))
            return r
        monkeypatch.setattr(self.eng.vit, "forward", forward)
        self.worst = 0.0

    def open(self):
        hs = [p.open() for p in self.pools]
        assert len(set(hs)) == 1
        self.model.open(hs[0])
        return hs[0]

    def reset(self, h):
        for p in self.pools:
            p.reset(h)
        self.model.reset(h)

    def close(self, h):
        for p in self.pools:
            p.close(h)

    def push(self, per_session):
        """one pixel push of all three pools -> (the gated pool's output, the keep pattern)"""
        handles, counts = list(per_session), [f.shape[0] for f in per_session.values()]
        frames = torch.cat(list(per_session.values()))
        plan = self.model.plan(frames, handles, counts)
        kept = plan[2]
        self.seen, self.recording = [], True
        out = self.gated.push_packed(frames, handles, counts)
        self.recording = False
        # (a) the tower saw exactly the kept frames, in calls of at most max_frames
        sizes = [n for n, _ in self.seen]
        assert sum(sizes) == len(kept) and all(n <= self.eng.max_frames for n in sizes), (sizes, kept)
        tower_rows = torch.cat([o for _, o in self.seen]) if self.seen else None
        feats, pattern = self.model.expand(plan, handles, tower_rows)
        assert self.gated.last_kept() == pattern
        for h in handles:
            st = self.gated.stats(h)
            assert (st["tower_frames"], st["still_frames"]) == (self.model.s[h]["tower"], self.model.s[h]["still"]), h
        # (b) bit for bit the twin fed the expanded rows
        _same_outputs(out, self.twin.push_features_packed(feats, handles, counts))
        # (c) within the batch bound of the pool that ran the tower on every frame
        if self.full is not None:
            ref = self.full.push_packed(frames, handles, counts)
            assert ref.offsets == out.offsets
            if out.logits.numel():
                self.worst = max(self.worst, float((out.logits - ref.logits).abs().max()))
        return out, pattern

    def push_features(self, h, feats):
        outs = [p.push_features_packed(feats, [h], [feats.shape[0]]) for p in self.pools]
        self.model.features_pushed(h, feats)
        for o in outs[1:]:
            _same_outputs(outs[0], o)


def _with_repeats(frames, runs):
    """frames [n, ...] -> each frame i repeated runs[i % len(runs)] times in a row"""
    idx = [i for i in range(frames.shape[0]) for _ in range(runs[i % len(runs)])]
    return frames[idx]


def test_the_pool_skips_exactly_the_repeats(monkeypatch):
    from clip_fsar_amd.still import StillGate
    head = _head(ARCH, "fp32", T)
    with torch.no_grad():
        gal = _filled(head, ARCH, T)
        trio = _Trio(gal, StillGate(), monkeypatch, max_streams=3, stride=1, max_push=8)
        monkeypatch.setattr(trio.eng, "max_frames", 16)
        base = _frames(ARCH, 3, 24, seed=31)
        A = _with_repeats(base[0], (1, 2, 3, 4, 5))            # runs of 1 to 5: 0 1 1 2 2 2 3 3 3 3 4 4 4 4 4 5 6 6 ..
        B, C = _with_repeats(base[1], (2, 1)), _with_repeats(base[2], (1, 3))
        a, b = trio.open(), trio.open()
        out, pat = trio.push({a: A[:5], b: B[:3]})
        assert pat == {a: (True, True, False, True, False), b: (True, False, True)}
        # a run over the push boundary (A[5] = A[4] = base frame 2), and a session whose whole push repeats its last frame
        out, pat = trio.push({a: A[5:11], b: B[2:3].repeat(3, 1, 1, 1)})
        assert pat == {a: (False, True, False, False, False, True), b: (False, False, False)}
        assert trio.gated.stats(b) == {"frames": 6, "tower_frames": 2, "windows": 0, "still_frames": 4}
        # a push in which nothing goes through the tower at all: NK = 0; a's first windows complete in it
        out, pat = trio.push({a: A[10:11].repeat(2, 1, 1, 1), b: B[2:3]})
        assert pat == {a: (False, False), b: (False,)} and trio.seen == []
        assert out.logits.shape[0] == out.offsets[-1] == 2 and trio.gated.stats(a)["windows"] == 6
        # one push of several rounds (27 frames of a against max_push = 8); c joins with its first frame
        c = trio.open()
        out, pat = trio.push({a: A[11:38], c: C[:1]})
        assert len(pat[a]) == 27 and pat[a][0] is False and 5 < sum(pat[a]) < 16 and pat[c] == (True,)
        assert [n for n, _ in trio.seen] == [sum(pat[a]) + 1]      # one tower call, sized by the kept frames
        # reset: b's next frame equals the one in the store and must go through the tower all the same
        trio.reset(b)
        out, pat = trio.push({b: B[2:5]})
        assert pat[b][0] is True and pat == {b: (True, True, False)}
        # a reused slot: d's first frame equals the previous owner's last
        slot = trio.gated._sessions[c].slot
        trio.close(c)
        d = trio.open()
        assert trio.gated._sessions[d].slot == slot
        out, pat = trio.push({d: C[:4]})
        assert pat == {d: (True, True, False, False)}
        # a feature push in between: a's newest frame is no longer the one in the store
        trio.push_features(a, torch.randn(3, gal.E, generator=torch.Generator().manual_seed(5)).to(DEV))
        out, pat = trio.push({a: A[37:40], d: C[3:6]})
        assert pat == {a: (True, False, False), d: (False, True, True)}
        # ... and afterwards its repeats are skipped again
        out, pat = trio.push({a: A[39:40].repeat(2, 1, 1, 1)})
        assert pat == {a: (False, False)}
        total = trio.gated.stats()
        assert total["tower_frames"] + total["still_frames"] == total["frames"] - 3 and total["still_frames"] > 20
        assert trio.twin.stats()["tower_frames"] == 0 and trio.full.stats()["tower_frames"] == total["frames"] - 3
        assert trio.worst <= BOUND, trio.worst
        # another geometry is refused, naming both
        with pytest.raises(ValueError, match=r"frames of 32 x 32 pushed into a pool whose still= store was made for 64 x 64"):
            trio.gated.push_packed(torch.zeros(1, 3, 32, 32, device=DEV), [a], [1])


# ------------------------------------------------------------------ 4: tolerances
def test_tolerances_noise_is_still_and_a_moved_patch_is_not(monkeypatch):
    """frame values are multiples of 1/64, so every difference is exact: noise of at most 2/64 per step under pixel_tol = 3/64 is
    still, a 24 x 24 patch (1 728 elements > limit = floor(0.1 * 12 288) = 1 228) off by 8/64 is a move, a 16 x 16 patch (768) is not;
    max_run = 3 forces every fourth frame of a still run through the tower"""
    from clip_fsar_amd.still import StillGate
    head = _head(ARCH, "fp32", T)
    gate = StillGate(pixel_tol=3 / 64, changed=0.1, max_run=3)
    assert gate.limit(3 * 64 * 64) == 1228
    g = torch.Generator().manual_seed(77)
    n = 26
    frames = torch.empty(n, 3, 64, 64)
    frames[0] = _sixtyfourths((3, 64, 64), g)
    moved, small = {5, 6, 15}, {10, 20}
    for i in range(1, n):
        frames[i] = frames[i - 1] + torch.randint(-2, 3, (3, 64, 64), generator=g).float() / 64
        if i in moved:
            frames[i, :, 8:32, 30:54] += (8 / 64) * (1 if i % 2 else -1)
        if i in small:
            frames[i, :, 40:56, 4:20] += 8 / 64
    assert bool((frames * 64 == (frames * 64).round()).all()) and float(frames.abs().max()) < 4
    frames = frames.to(DEV)
    with torch.no_grad():
        gal = _filled(head, ARCH, T)
        trio = _Trio(gal, gate, monkeypatch, full=False, max_streams=2, stride=2, max_push=8)
        h = trio.open()
        pattern = ()
        for f0, f1 in ((0, 4), (4, 11), (11, 12), (12, 20), (20, 26)):
            pattern += trio.push({h: frames[f0:f1]})[1][h]            # equal to plan_still over reference_changed, asserted in push()
    #          0     1      2      3      4     5     6     7      8      9      10    11     12     13     14    15    16 ..
    want = [True, False, False, False, True, True, True, False, False, False, True, False, False, False, True, True, False, False,
            False, True, False, False, False, True, False, False]
    assert list(pattern) == want
    assert trio.gated.stats(h) == {"frames": 26, "tower_frames": sum(want), "windows": 10, "still_frames": 26 - sum(want)}


# ------------------------------------------------------------------ 5: composition
def test_every_other_option_inherits_the_gate(monkeypatch):
    from test_gpu_live import IDS, _pair, _videos
    from clip_fsar_amd.baseline import Baseline
    from clip_fsar_amd.events import EventRule
    from clip_fsar_amd.evidence import Evidence
    from clip_fsar_amd.still import StillGate
    with torch.no_grad():
        head, live, _ = _pair()
        live.add_classes(_videos(12, 51), IDS)
        kw = dict(max_streams=3, stride=1, max_push=8, smooth=0.5, smooth_by="class", rates=(1, 2),
                  baseline=Baseline(rate=1 / 4, warm_rate=0.5, warmup=2, gate=3.0), events=EventRule(0.5, 0.0, 1, 1),
                  evidence=Evidence(64, ("onset", "offset")))
        trio = _Trio(live, StillGate(), monkeypatch, full=False, **kw)
        base = _frames(ARCH, 2, 30, seed=41)
        A, B = _with_repeats(base[0], (1, 3, 2)), _with_repeats(base[1], (2, 1, 4))
        a, b = trio.open(), trio.open()
        t, windows = 0, 0
        for na, nb in ((5, 3), (7, 8), (20, 2), (6, 6), (3, 9), (8, 8)):           # (20, 2): three rounds
            out, pat = trio.push({a: A[t:t + na], b: B[t:t + nb]} if nb else {a: A[t:t + na]})
            assert type(out).__name__ == "DeviationTempoPackedOutput" and out.tempo is not None and out.smoothed is not None
            windows += out.logits.shape[0]
            t += max(na, nb)
        mine, theirs = trio.gated.take_events(), trio.twin.take_events()
        assert [tuple(e) for e in mine] == [tuple(e) for e in theirs] and windows > 40
        assert len(mine) > 0 and any(e.evidence is not None for e in mine)
        for e, f in zip(mine, theirs):
            if e.evidence is not None and trio.gated.held(e):
                assert torch.equal(trio.gated.evidence_features(e), trio.twin.evidence_features(f))
        st = trio.gated.stats()
        assert st["still_frames"] > 20 and st["tower_frames"] + st["still_frames"] == st["frames"]
        assert trio.twin.stats()["events"] == st["events"] and "still_frames" not in trio.twin.stats()
