"""HIP-event timing shared by the gallery timing tools."""
import statistics

import torch


def _time_ms(fn, reps):
    """median over reps timed calls of fn() (ms between HIP events), after one warm-up call"""
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        ts.append(s.elapsed_time(e))
    return statistics.median(ts)
