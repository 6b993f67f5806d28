#!/usr/bin/env python
"""Warm start on the device: what it costs and what it replaces.

    python scripts/bench_warm_start.py [--calls 200] [--repeats 3] [--frames 100]

1. Op time: ``ops.forward_interpolate`` (csrc/forward_interp.hip), device
   events around ``--calls`` back-to-back calls, at the 1/8 fields of Sintel
   (1x2x55x128) and STIR (1x2x64x80), on ``smooth(amp=6, noise=0.5)`` flows.
   Next to it the host path it replaces on the same input:
   ``utils.geometry.forward_interpolate(flow).to(dev)``, host clock, with its
   device-to-host copy, KD-tree, host-to-device copy and synchronise.
2. Tracker time: ms per frame of ``SequenceTracker`` with warm start on and
   off against ``PointTrackServer`` per pair; RAFT-small, 512x640, 32 points,
   12 iterations, bf16 and fp32, frames already on the device, the variants
   alternating inside every repeat.

Every repeat is printed, so the spread is visible; one JSON line per
measurement.  Needs a GPU: there is no CPU fall-back.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from raft_stir_amd import ops  # noqa: E402
from raft_stir_amd.config import make_args  # noqa: E402
from raft_stir_amd.export.pointtrack import PointTrackServer, SequenceTracker  # noqa: E402
from raft_stir_amd.models import RAFT  # noqa: E402
from raft_stir_amd.utils.geometry import forward_interpolate as host_forward_interpolate  # noqa: E402


def smooth(H, W, seed, amp, noise):
    g = torch.Generator().manual_seed(seed)
    lo = torch.randn(1, 2, max(2, H // 8), max(2, W // 8), generator=g) * amp
    f = F.interpolate(lo, size=(H, W), mode="bilinear", align_corners=True)[0]
    return f + noise * torch.randn(2, H, W, generator=g)


def device_ms(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def host_ms(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


def bench_op(dev, calls, repeats):
    out = {}
    for name, (H, W) in (("sintel_55x128", (55, 128)), ("stir_64x80", (64, 80))):
        flow = smooth(H, W, 0, 6, 0.5)[None].to(dev)
        same = torch.equal(ops.forward_interpolate(flow)[0].cpu(), host_forward_interpolate(flow[0]))
        for _ in range(20):
            ops.forward_interpolate(flow)
        host_forward_interpolate(flow[0]).to(dev)
        op = [device_ms(lambda: ops.forward_interpolate(flow), calls) for _ in range(repeats)]
        host = [host_ms(lambda: host_forward_interpolate(flow[0])[None].to(dev), max(20, calls // 10))
                for _ in range(repeats)]
        rec = {"bench": "forward_interpolate", "shape": [1, 2, H, W], "calls": calls,
               "op_us": [round(v * 1e3, 2) for v in op], "host_path_us": [round(v * 1e3, 1) for v in host],
               "op_equals_host_path": same, "op_faster_than_host_path": max(op) < min(host)}
        print(json.dumps(rec), flush=True)
        out[name] = min(op)
        if not rec["op_faster_than_host_path"]:
            raise SystemExit(f"forward_interpolate is not faster than the host path at {name}")
    return out


def bench_tracker(dev, frames_n, repeats, mixed):
    torch.manual_seed(0)
    model = RAFT(make_args(small=True, mixed_precision=mixed)).to(dev).to(memory_format=torch.channels_last).eval()
    g = torch.Generator().manual_seed(1)
    pool = [(torch.rand(1, 3, 512, 640, generator=g) * 255).to(dev) for _ in range(8)]
    points = (torch.rand(1, 32, 2, generator=g) * 500).to(dev)
    warm = SequenceTracker(model, iters=12, warm_start=True)
    cold = SequenceTracker(model, iters=12, warm_start=False)
    server = PointTrackServer(model, iters=12)

    def run_tracker(trk):
        def go():
            trk.reset()
            trk.step(pool[0], points)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for t in range(1, frames_n + 1):
                trk.step(pool[t % len(pool)])
            b.record()
            b.synchronize()
            return a.elapsed_time(b) / frames_n
        return go

    def run_server():
        pts = points
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for t in range(1, frames_n + 1):
            pts = server(pts, pool[(t - 1) % len(pool)], pool[t % len(pool)])
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / frames_n

    variants = {"tracker_warm": run_tracker(warm), "tracker_cold": run_tracker(cold), "server_pair": run_server}
    for fn in variants.values():  # capture + warm-up
        fn()
    ms = {k: [] for k in variants}
    for _ in range(repeats):
        for k, fn in variants.items():
            ms[k].append(round(fn(), 4))
    rec = {"bench": "sequence_tracker", "model": "raft-small", "precision": "bf16" if mixed else "fp32",
           "size": [512, 640], "points": 32, "iters": 12, "frames": frames_n, "ms_per_frame": ms,
           "warm_start_cost_ms": round(min(ms["tracker_warm"]) - min(ms["tracker_cold"]), 4)}
    print(json.dumps(rec), flush=True)
    return min(ms["server_pair"])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=200, help="timed op calls per repeat (at least 200)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--frames", type=int, default=100, help="timed frames per tracker repeat")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_warm_start needs a GPU")
    dev = torch.device("cuda", 0)
    ops._ext.load(raise_on_error=True)
    op = bench_op(dev, max(200, a.calls), a.repeats)
    for mixed in (True, False):
        pair = bench_tracker(dev, a.frames, a.repeats, mixed)
        print(json.dumps({"bench": "op_share", "precision": "bf16" if mixed else "fp32",
                          "op_us_stir_64x80": round(op["stir_64x80"] * 1e3, 2), "graphed_pair_ms": pair,
                          "op_share_of_graphed_pair": round(op["stir_64x80"] / pair, 4)}), flush=True)


if __name__ == "__main__":
    main()
