#!/usr/bin/env python
"""Re-anchoring the dense tracker: what the composition of two track fields costs.

    python scripts/bench_reanchor.py [--calls 200] [--repeats 3] [--frames 40] [--only op|tracker]

1. Op time: ``ops.dense_compose`` (csrc/dense_compose.hip, one launch) at
   512x640 on two pairs of fields: ``smooth``, base and inner field both the
   pixel grid plus ``smooth(amp=6, noise=0.2)`` as in bench_dense_flow.py with
   10 % of the scores +inf, and ``scatter``, the same inner field under a base
   that sends every pixel to a random place of the frame (no two neighbouring
   threads gather from neighbouring cells).  The call writes into buffers of
   the caller's, is captured with ``runtime.graph.capture`` and its replays
   are timed with device events.  Next to it: the ATen oracle
   (``reference.dense_compose``) run eagerly on the same GPU tensors.  The byte
   floor is what the launch must move if every gathered plane were read once:
   three base planes and five inner planes read, 4+4+4+1+4+4 B/pixel written.
   ``ops.dense_query`` at N = 32 and N = H*W against ``reference.dense_query``
   on the GPU, the same way.
2. Tracker time: ``DenseMultiFlowTracker.track(frames)``, RAFT-small, bf16,
   512x640, 12 iterations, ``cache_features``, five deltas, frames on the
   device: a tracker that never re-anchors against one that re-anchors once,
   on the second frame (so every later frame pays the composition), the two
   alternating inside every repeat; and the cost of the re-anchor itself, the
   wall time of ``reanchor()`` with a device synchronisation on both sides.

Every tensor a captured graph reads or writes, every graph and every tracker
is kept in one list until ``main`` returns; nothing is deleted and the
allocator's cache is never emptied.  Every repeat is printed, one JSON line per
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
from raft_stir_amd.export.denseflow import DenseMultiFlowTracker  # noqa: E402
from raft_stir_amd.models import RAFT  # noqa: E402
from raft_stir_amd.ops import reference  # noqa: E402
from raft_stir_amd.runtime.graph import capture  # noqa: E402

H, W = 512, 640
INF = float("inf")


def smooth(H, W, seed, amp, noise):
    g = torch.Generator().manual_seed(seed)
    lo = torch.randn(1, 2, max(2, H // 8), max(2, W // 8), generator=g) * amp
    f = F.interpolate(lo, size=(H, W), mode="bilinear", align_corners=True)[0]
    return f + noise * torch.randn(2, H, W, generator=g)


def field(seed):
    """(pos, score): the grid plus a smooth displacement, 10 % of the pixels lost."""
    g = torch.Generator().manual_seed(seed)
    score = torch.rand(1, 1, H, W, generator=g)
    score[torch.rand(1, 1, H, W, generator=g) < 0.1] = INF
    return (reference.coords_grid(1, H, W) + smooth(H, W, seed, 6, 0.2)[None]).contiguous(), score


def cases():
    g = torch.Generator().manual_seed(3)
    pos, score = field(1)
    delta = torch.tensor([1, 2, 4, 8, 0], dtype=torch.int32)[torch.randint(0, 5, (1, 1, H, W), generator=g)]
    err = torch.rand(1, 1, H, W, generator=g)
    inner = (pos, score, delta.contiguous(), err)
    yield "smooth", field(0), inner
    scatter = torch.rand(1, 2, H, W, generator=g) * torch.tensor([W - 1.0, H - 1.0]).view(1, 2, 1, 1)
    yield "scatter", (scatter.contiguous(), field(0)[1]), inner


def device_us(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls * 1e3


def same(a, b):
    return bool(((a == b) | ((a != a) & (b != b))).all())


def bench_op(dev, calls, repeats, keep):
    N = H * W
    for name, base, inner in cases():
        args = [t.to(dev) for t in base + inner]
        out = (torch.empty(1, 2, H, W, device=dev), torch.empty(1, 1, H, W, device=dev),
               torch.empty(1, 1, H, W, dtype=torch.bool, device=dev),
               torch.empty(1, 1, H, W, dtype=torch.int32, device=dev), torch.empty(1, 1, H, W, device=dev))
        keep += [args, out]

        def hip():
            return ops.dense_compose(*args, out=out)

        def aten():
            return reference.dense_compose(*args)

        graph, _ = capture(dev, hip)
        keep.append(graph)
        graph.replay()
        ref = aten()
        keep.append(ref)
        row = {"bench": "dense_compose", "field": name, "shape": [H, W], "calls": calls,
               "hip_graph_us": [round(device_us(graph.replay, calls), 2) for _ in range(repeats)],
               "aten_gpu_eager_us": [round(device_us(aten, 20), 1) for _ in range(repeats)],
               "bit_equal_to_aten_gpu": all(same(a, b) for a, b in zip(out, ref)),
               "bit_equal_to_cpu_oracle": all(same(a.cpu(), b) for a, b in
                                              zip(out, reference.dense_compose(*(t.cpu() for t in args))))}
        floor_mb = (3 * 4 + 5 * 4 + 21) * N / 1e6
        best = min(row["hip_graph_us"])
        row.update(visible=round(out[2].float().mean().item(), 3), floor_MB=round(floor_mb, 2),
                   GBps_at_floor=round(floor_mb / 1e3 / (best / 1e6), 1),
                   aten_gpu_over_hip=round(min(row["aten_gpu_eager_us"]) / best, 1))
        print(json.dumps(row), flush=True)
    # the point form, on the inner field of the last case
    pos, score = args[2], args[3]
    g = torch.Generator().manual_seed(4)
    for n in (32, N):
        pts = (torch.rand(1, n, 2, generator=g) * torch.tensor([W + 1.0, H + 1.0]) - 1.0).to(dev)
        keep.append(pts)

        def hip_q(pts=pts):
            return ops.dense_query(pos, score, pts)

        def aten_q(pts=pts):
            return reference.dense_query(pos, score, pts)

        graph, got = capture(dev, hip_q)
        keep += [graph, got]
        graph.replay()
        ref = aten_q()
        keep.append(ref)
        row = {"bench": "dense_query", "shape": [H, W], "N": n, "calls": calls,
               "hip_graph_us": [round(device_us(graph.replay, calls), 2) for _ in range(repeats)],
               "hip_eager_us": [round(device_us(hip_q, calls), 2) for _ in range(repeats)],
               "aten_gpu_eager_us": [round(device_us(aten_q, 20), 1) for _ in range(repeats)],
               "bit_equal_to_aten_gpu": all(same(a, b) for a, b in zip(got, ref))}
        row["aten_gpu_over_hip_eager"] = round(min(row["aten_gpu_eager_us"]) / min(row["hip_eager_us"]), 1)
        print(json.dumps(row), flush=True)


def bench_tracker(dev, frames_n, repeats, keep):
    torch.manual_seed(0)
    model = RAFT(make_args(small=True, mixed_precision=True)).to(dev).to(memory_format=torch.channels_last).eval()
    g = torch.Generator().manual_seed(1)
    pool = [(torch.rand(1, 3, H, W, generator=g) * 255).to(dev) for _ in range(8)]
    frames = [pool[t % len(pool)] for t in range(frames_n)]
    trk = DenseMultiFlowTracker(model, iters=12, deltas=(1, 2, 4, 8, None), cache_features=True)
    keep += [model, pool, frames, trk]
    once = []  # the wall time of every reanchor() call

    def run(reanchor):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        trk.reset()
        for t in range(frames_n):
            trk.step(frames[t])
            if reanchor and t == 1:
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                trk.reanchor()
                torch.cuda.synchronize()
                once.append(round((time.perf_counter() - t1) * 1e3, 4))
        torch.cuda.synchronize()
        keep.append(trk.pos[:, :1, :1, :1].clone())
        return (time.perf_counter() - t0) * 1e3 / frames_n

    variants = {"plain": lambda: run(False), "reanchored": lambda: run(True)}
    for fn in variants.values():  # capture + warm-up
        fn()
    once.clear()
    ms = {k: [] for k in variants}
    for _ in range(repeats):
        for k, fn in variants.items():
            ms[k].append(round(fn(), 4))
    # the re-anchor itself is inside the re-anchored run's time: take it out of the per-frame difference
    per_frame = [(m * frames_n - o) / frames_n for m, o in zip(ms["reanchored"], once)]
    print(json.dumps({"bench": "reanchor_tracker", "model": "raft-small", "precision": "bf16", "size": [H, W],
                      "iters": 12, "deltas": 5, "frames": frames_n, "graphs": len(trk.graphs), "ms_per_frame": ms,
                      "reanchor_call_ms": once,
                      "added_us_per_frame": round((min(per_frame) - min(ms["plain"])) * 1e3 * frames_n
                                                  / (frames_n - 2), 1),
                      "plain_spread_us": round((max(ms["plain"]) - min(ms["plain"])) * 1e3, 1),
                      "reanchored_spread_us": round((max(per_frame) - min(per_frame)) * 1e3, 1)}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=200, help="timed op replays per repeat (at least 200)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--frames", type=int, default=40, help="frames per tracked sequence")
    ap.add_argument("--only", choices=("op", "tracker"), help="one of the two measurements")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_reanchor needs a GPU")
    dev = torch.device("cuda", 0)
    ops._ext.load(raise_on_error=True)
    keep = []  # everything a graph touches lives until main returns
    with torch.no_grad():
        if a.only != "tracker":
            bench_op(dev, max(200, a.calls), max(3, a.repeats), keep)
        if a.only != "op":
            bench_tracker(dev, a.frames, max(3, a.repeats), keep)
    torch.cuda.synchronize()
    return keep


if __name__ == "__main__":
    main()
