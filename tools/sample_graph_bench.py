"""What `tools/gpt_sample_bench.py --graph` and `tools/rq_sample_bench.py --graph` share: one position of a prior's sampling loop captured into a HIP
graph the way `sample(graph=True)` captures it (prior.py `_sample_graphed`: the cursor forms of the launches, enh_cursor_advance at the end, one side
stream), and the measurement around it: windows of consecutive positions, eager and graph alternating in one process after a warm-up of both, every
window timed with a host clock around work that ends in a device synchronise (the loop is host-bound: device events would miss the enqueue), the
codes and logits of the two paths compared bit for bit at the positions timed."""
import ctypes
import statistics
import time

import torch

from enhancing import _C


def capture_position(later, dev):
    """(graph, cursor, seconds of capture + instantiate, kernel nodes or None): `later(cursor)` are the launches of one position in their cursor
    forms; called with the side stream current"""
    cursor = torch.ones(1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    try:
        g, kept = torch.cuda.CUDAGraph(keep_graph=True), True
    except TypeError:
        g, kept = torch.cuda.CUDAGraph(), False
    with torch.cuda.graph(g, stream=torch.cuda.current_stream()):
        later(cursor)
        _C.cursor_advance(cursor)
    if kept:
        g.instantiate()
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    nodes = None
    if kept:
        try:
            n = ctypes.c_size_t(0)
            if ctypes.CDLL("libamdhip64.so").hipGraphGetNodes(ctypes.c_void_p(g.raw_cuda_graph()), None, ctypes.byref(n)) == 0:
                nodes = n.value
        except (OSError, AttributeError, RuntimeError):
            pass
    return g, cursor, seconds, nodes


def window(fn, first, count):
    """ms per position of fn(t) over the positions first .. first + count - 1, host clock, ending in a device synchronise"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for t in range(first, first + count):
        fn(t)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / count


def eager_against_graph(eager, graph, cursor, first, count, reps=5):
    """((mean, min, max) ms per position of the eager loop, the same of the replays): `reps` rounds of one window each, alternating, after a warm-up
    window of both.  eager(t) runs position t; a graph window sets the cursor to `first` and replays `count` times."""
    def replays(t):
        if t == first:
            cursor.fill_(first)
        graph.replay()
    window(eager, first, count)
    window(replays, first, count)
    te, tg = [], []
    for _ in range(reps):
        te.append(window(eager, first, count))
        tg.append(window(replays, first, count))
    st = lambda v: (statistics.mean(v), min(v), max(v))
    return st(te), st(tg)


def same_bits(a, b) -> bool:
    return torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)


def fmt(v) -> str:
    return f"{v[0]:.3f} [{v[1]:.3f} .. {v[2]:.3f}]"
