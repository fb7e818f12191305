"""GPU: the launch trace of clip_fsar_amd.pool.StreamPool -- every call a push, take_events(), topk, leaders, active and baseline make into
the twelve binding modules pool.py imports and into the gallery's classify_features, classify_features_grouped and topk_of_groups, in
order, with the shape and dtype of every tensor argument and the value of every int, float, bool, None and tuple -- against
tests/golden/pool_launch_trace.json, over five configurations of a pool of four streams with three sessions and test_gpu_contest's seven
pushes (pushes beyond max_push, pushes that complete no window).

The golden pins what the pool asks of the device, not what the device answers: it was recorded by this module's recorder
(`python tests/test_gpu_pool_trace.py OUT.json`) from the pool.py of the commit BEFORE the pool's keyed cell stores, judged tail and
output types were folded into shared helpers, and is never to be recorded again from a later pool.py: a difference in any entry is a
change of the device work, and the pool is wrong, not the golden.  Two things that fold changed lie outside the trace, because neither is
a binding call:
  * a shortlist push with an event rule asked for the detector's cells twice; the second request only repeated the torch fills that
    zero the marks of forgotten slots, over a set the first had emptied.  It asks once now.
  * a grouped push (a session with a class list) moved its sessions' frame counters and the pool's totals before smoothing, the baseline
    and the detector; every push moves them after the detector now.  The evidence capture takes the sessions' frames after the push
    either way."""
import contextlib
import inspect
import json
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pool_launch_trace.json")
BINDINGS = ("pool_hip", "class_smooth_hip", "events_hip", "baseline_hip", "contest_hip", "evidence_hip", "tempo_hip", "pool_select_hip",
            "still_hip", "enroll_hip", "groups_hip", "gallery_hip")
GALLERY_CALLS = ("classify_features", "classify_features_grouped", "topk_of_groups")
CONFIGS = ("plain", "grouped", "shortlist", "rates", "still")
DTYPES = {torch.float32: "f32", torch.int32: "i32", torch.int64: "i64", torch.bool: "b", torch.uint8: "u8"}


def _told(v):
    """what the trace keeps of one argument"""
    if isinstance(v, torch.Tensor):
        return [DTYPES.get(v.dtype, str(v.dtype)), list(v.shape)]
    if v is None or isinstance(v, (bool, int, float)):
        return v
    if isinstance(v, tuple):
        return {"tuple": [_told(x) for x in v]}
    return type(v).__name__


@contextlib.contextmanager
def _recording(gallery, trace):
    """every public function of the binding modules, and the gallery's three scoring calls, append (name, arguments) to `trace` on
    their way in; pool.py calls all of them through module and instance attributes, so nothing of the package changes"""
    import importlib
    undo = []

    def wrap(owner, attr, name, f):
        def recorded(*args, **kw):
            trace.append([name] + [_told(a) for a in args] + [[k, _told(v)] for k, v in sorted(kw.items())])
            return f(*args, **kw)
        setattr(owner, attr, recorded)

    try:
        for short in BINDINGS:
            mod = importlib.import_module("clip_fsar_amd." + short)
            for attr, f in sorted(vars(mod).items()):
                if inspect.isfunction(f) and not attr.startswith("_"):
                    undo.append((mod, attr, f))
                    wrap(mod, attr, "%s.%s" % (short, attr), f)
        for attr in GALLERY_CALLS:                 # on the instance, which the caller drops: nothing to undo
            wrap(gallery, attr, "gallery." + attr, getattr(gallery, attr))
        yield trace
    finally:
        for mod, attr, f in undo:
            setattr(mod, attr, f)


def _pool(config):
    """a gallery of its own and the configuration's pool over it"""
    from clip_fsar_amd.baseline import Baseline
    from clip_fsar_amd.contest import Contest
    from clip_fsar_amd.events import EventRule
    from clip_fsar_amd.evidence import Evidence
    from clip_fsar_amd.pool import StreamPool
    from clip_fsar_amd.shortlist import Shortlist
    from clip_fsar_amd.still import StillGate
    from test_gpu_contest import ALPHA
    from test_gpu_events import MAX_PUSH, STRIDE, _gallery
    live = _gallery("live")
    kw = dict(max_streams=4, stride=STRIDE, max_push=MAX_PUSH)
    # with a baseline the rule judges deviations: an onset at half a deviation above the pair's mean, an offset below the mean
    judged = dict(events=EventRule(0.5, 0.0, 1, 1), evidence=Evidence(capacity=8), baseline=Baseline(rate=0.25, warm_rate=0.5, warmup=2, gate=3.0))
    if config == "plain":
        kw.update(smooth=ALPHA)
    elif config == "grouped":
        kw.update(judged, smooth=ALPHA, smooth_by="class", contest=Contest(top=2))
    elif config == "shortlist":
        kw.update(judged, smooth=ALPHA, smooth_by="class", contest=Contest(top=2), shortlist=Shortlist(live, keep=3), shortlist_hold=1)
    elif config == "rates":
        kw.update(judged, rates=(1, 2))
    else:
        kw.update(still=StillGate())
    return live, StreamPool(live, **kw)


def drive(config, trace=None):
    """the configuration's pool through test_gpu_contest's CUTS -> (every push's outputs, every take_events() result); with `trace`:
    recorded"""
    from test_gpu_contest import CUTS
    from test_gpu_events import _feats
    from test_gpu_live import ARCH
    from test_gpu_stream import _frames
    outs, taken = [], []
    with torch.no_grad():
        live, pool = _pool(config)
        total = [sum(c[i] for c in CUTS) for i in range(3)]
        if config == "still":                      # pixel frames, every second one a repeat of its predecessor
            base = _frames(ARCH, 3, max(total), seed=31)
            streams = [base[i][[j // 2 for j in range(n)]] for i, n in enumerate(total)]
            push = pool.push
        else:
            streams = [_feats(n, live.E, 900 + i) for i, n in enumerate(total)]
            push = pool.push_features
        with _recording(live, [] if trace is None else trace) as trace:
            hs = [pool.open(), pool.open(classes=[9, 2]) if config == "grouped" else pool.open(), pool.open()]
            done = [0, 0, 0]
            for k, counts in enumerate(CUTS):
                out = push({hs[i]: streams[i][done[i]:done[i] + n] for i, n in enumerate(counts) if n})
                done = [d + n for d, n in zip(done, counts)]
                outs.append(out)
                if config == "still":
                    trace.append(["last_kept"] + [[h, list(kept)] for h, kept in sorted(pool.last_kept().items())])
                if pool._events is not None and k in (1, len(CUTS) - 1):
                    taken.append(pool.take_events())
            assert done == total and list(out) == hs
            for h in hs:
                pool.topk(out[h], k=2)
                if pool._contest_rule is not None:
                    pool.leaders(out[h])
                if pool._events is not None:
                    pool.active(h)
                if pool._baseline is not None:
                    pool.baseline(h)
    return outs, taken


def record():
    """{configuration: its trace}, as JSON holds it"""
    traces = {}
    for config in CONFIGS:
        traces[config] = []
        drive(config, traces[config])
    return json.loads(json.dumps(traces))


@pytest.mark.parametrize("config", CONFIGS)
def test_the_launch_trace_is_the_goldens(config):
    with open(GOLDEN) as f:
        want = json.load(f)[config]
    got = []
    outs, taken = drive(config, got)
    got = json.loads(json.dumps(got))
    assert len(want) > 50 and sum(o[h].logits.shape[0] for o in outs for h in o) > 30          # the run is not vacuous
    assert config in ("plain", "still") or sum(len(t) for t in taken) > 0
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            print("entry %d differs:\n  got    %r\n  golden %r" % (i, g, w))
        assert g == w, i
    assert len(got) == len(want)


if __name__ == "__main__":                          # the recorder on its own: writes the trace of the pool.py it finds
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle")]
    with open(sys.argv[1], "w") as f:
        json.dump(record(), f, separators=(",", ":"))
