#!/usr/bin/env python
"""Encoding a frame once: what ``cache_features=True`` saves per step.

    python scripts/bench_feature_cache.py [--calls 200] [--repeats 3] [--frames 100]

1. Op time: ``ops.feature_ring_step`` (csrc/feat_ring.hip) at the trackers'
   benchmark shape (512x640 frames: 64x80 feature maps, RAFT-small's 128
   feature and 160 context channels, bf16 and fp32) for K = 1 and K = 5 slots,
   against its ATen composite (``reference.feature_ring_step``) on the same
   device tensors.  Each form is captured in its own hipGraph, as the tracker
   runs it, and the replays are timed with device events.
2. Tracker time: ms per frame, RAFT-small, 512x640, 32 points, 12 iterations,
   bf16 and fp32, frames already on the device, every configuration with
   ``cache_features`` off and on, all of them alternating inside every repeat:
     tracker_fb      SequenceTracker(fb_check=True)
     multi_1         MultiFlowTracker(deltas=(1,))
     multi_1_anchor  MultiFlowTracker(deltas=(1, None))
     multi_5         MultiFlowTracker(deltas=(1, 2, 4, 8, None))
   The yardstick of a cached tracker is the uncached one of the same process;
   ``spread_ms`` is the max minus the min of the uncached repeats, and
   ``slower_than_spread`` says whether the cached tracker's best repeat is
   slower than the uncached one's by more than that.

Every repeat is printed; one JSON line per measurement.  Needs a GPU: there is
no CPU fall-back.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from raft_stir_amd import ops  # noqa: E402
from raft_stir_amd.config import make_args  # noqa: E402
from raft_stir_amd.export.multiflow import MultiFlowTracker, ring_index_row, ring_index_table  # noqa: E402
from raft_stir_amd.export.pointtrack import SequenceTracker  # noqa: E402
from raft_stir_amd.models import RAFT  # noqa: E402
from raft_stir_amd.ops import reference  # noqa: E402

ALPHA = (0.01, 0.5)
CONFIGS = {"tracker_fb": None, "multi_1": (1,), "multi_1_anchor": (1, None), "multi_5": (1, 2, 4, 8, None)}


def device_ms(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def graphed(fn, dev):
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        for _ in range(3):
            fn()
    torch.cuda.current_stream(dev).wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    g.replay()
    return g


def bench_op(dev, calls, repeats):
    h, w, C, Cc = 64, 80, 128, 160
    for dtype, name in ((torch.bfloat16, "bf16"), (torch.float32, "fp32")):
        for deltas in ((1,), (1, 2, 4, 8, None)):
            K = len(deltas)
            L = max(d for d in deltas if d is not None)
            R = L + 2
            g = torch.Generator().manual_seed(K)
            mk = lambda *s: torch.randn(*s, generator=g).to(dev, dtype)  # noqa: E731
            t = [mk(R, h, w, C), mk(R, h, w, Cc), mk(1, h, w, C), mk(1, h, w, Cc)]
            out = [torch.zeros(3 * K, h, w, C, device=dev, dtype=dtype),
                   torch.zeros(2 * K, h, w, Cc, device=dev, dtype=dtype)]
            idx = torch.tensor(ring_index_table(deltas)[ring_index_row(3 * L, L)], dtype=torch.int32, device=dev)
            hip = lambda: ops.feature_ring_step(*t, idx, *out)  # noqa: E731
            aten = lambda: reference.feature_ring_step(*t, idx, *out)  # noqa: E731
            g_hip, g_aten = graphed(hip, dev), graphed(aten, dev)
            us = {"op_graph_us": [], "aten_graph_us": []}
            for _ in range(repeats):
                us["op_graph_us"].append(device_ms(g_hip.replay, calls) * 1e3)
                us["aten_graph_us"].append(device_ms(g_aten.replay, calls) * 1e3)
            moved = (3 * K + 1) * h * w * C + (2 * K + 1) * h * w * Cc  # elements written; as many are read
            best = min(us["op_graph_us"])
            print(json.dumps({"bench": "feature_ring_step", "precision": name, "K": K, "R": R,
                              "shape": [h, w, C, Cc], "calls": calls,
                              **{k: [round(x, 2) for x in v] for k, v in us.items()},
                              "aten_over_op_graph": round(min(us["aten_graph_us"]) / best, 2),
                              "op_gb_per_s": round(2 * moved * t[0].element_size() / best / 1e3, 1)}), flush=True)


def bench_tracker(dev, frames_n, repeats, mixed):
    torch.manual_seed(0)
    model = RAFT(make_args(small=True, mixed_precision=mixed)).to(dev).to(memory_format=torch.channels_last).eval()
    g = torch.Generator().manual_seed(1)
    pool = [(torch.rand(1, 3, 512, 640, generator=g) * 255).to(dev) for _ in range(8)]
    points = (torch.rand(1, 32, 2, generator=g) * 500).to(dev)

    def make(deltas, cache):
        if deltas is None:
            return SequenceTracker(model, iters=12, fb_check=True, fb_alpha=ALPHA, cache_features=cache)
        return MultiFlowTracker(model, iters=12, deltas=deltas, fb_alpha=ALPHA, cache_features=cache)

    def timed(trk):
        def go():
            trk.reset()
            trk.step(pool[0], points)
            for t in range(1, 10):  # past the longest span: every slot active
                trk.step(pool[t % len(pool)])
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for t in range(10, 10 + frames_n):
                trk.step(pool[t % len(pool)])
            b.record()
            b.synchronize()
            return a.elapsed_time(b) / frames_n
        return go

    variants = {(k, cache): timed(make(d, cache)) for k, d in CONFIGS.items() for cache in (False, True)}
    for fn in variants.values():  # capture + warm-up
        fn()
    ms = {k: [] for k in variants}
    for _ in range(repeats):
        for k, fn in variants.items():
            ms[k].append(round(fn(), 4))
    for name in CONFIGS:
        off, on = ms[(name, False)], ms[(name, True)]
        spread = max(off) - min(off)
        print(json.dumps({"bench": "feature_cache_tracker", "config": name, "model": "raft-small",
                          "precision": "bf16" if mixed else "fp32", "size": [512, 640], "points": 32, "iters": 12,
                          "frames": frames_n, "uncached_ms": off, "cached_ms": on, "spread_ms": round(spread, 4),
                          "saving_ms": round(min(off) - min(on), 4),
                          "cached_over_uncached": round(min(on) / min(off), 3),
                          "slower_than_spread": bool(min(on) - min(off) > spread)}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=200, help="timed op replays per repeat (at least 200)")
    ap.add_argument("--repeats", type=int, default=3, help="repeats per configuration (at least 3)")
    ap.add_argument("--frames", type=int, default=100, help="timed frames per tracker repeat")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_feature_cache needs a GPU")
    dev = torch.device("cuda", 0)
    ops._ext.load(raise_on_error=True)
    with torch.no_grad():
        bench_op(dev, max(200, a.calls), max(3, a.repeats))
    for mixed in (True, False):
        bench_tracker(dev, a.frames, max(3, a.repeats), mixed)


if __name__ == "__main__":
    main()
