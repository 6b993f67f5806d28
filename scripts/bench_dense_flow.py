#!/usr/bin/env python
"""Dense every-pixel tracking: what following all pixels costs over 32 points.

    python scripts/bench_dense_flow.py [--calls 200] [--repeats 3] [--frames 100] [--only op|tracker]

1. Op time: ``ops.dense_multi_flow_step`` (csrc/dense_flow.hip) for K = 1 and
   5 slots on (K,2,512,640) fields (``smooth(amp=6, noise=0.2)`` forward fields
   and their disturbed negations), a ring of K + 2 rows whose positions are
   the pixel grid moved by a smooth field, against what the point form offers
   for the same job: ``ops.multi_flow_track_points`` at N = H*W = 327680 with
   the device-to-device copies around it that MultiFlowTracker issues per
   step, three per slot to assemble ``starts`` / ``start_score`` /
   ``start_visible`` from the per-frame state, the ``where`` that stores +inf
   for a lost point, and the three clones that keep the result as the new
   frame's state.  Each form is captured in its own hipGraph and the replays
   are timed with device events.
2. Tracker time: ms per frame, RAFT-small, 512x640, 12 iterations, bf16 and
   fp32, frames already on the device, the variants alternating inside every
   repeat: ``DenseMultiFlowTracker`` against ``MultiFlowTracker`` with 32
   points for ``deltas`` = (1,), (1, None) and (1, 2, 4, 8, None), with
   ``cache_features`` off and on.

Every repeat is printed, so the spread is visible; one JSON line per
measurement.  Needs a GPU: there is no CPU fall-back.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from raft_stir_amd import ops  # noqa: E402
from raft_stir_amd.config import make_args  # noqa: E402
from raft_stir_amd.export.denseflow import DenseMultiFlowTracker  # noqa: E402
from raft_stir_amd.export.multiflow import MultiFlowTracker  # noqa: E402
from raft_stir_amd.models import RAFT  # noqa: E402
from raft_stir_amd.ops import reference  # noqa: E402

ALPHA = (0.01, 0.5)
H, W = 512, 640
DELTAS = {"1": (1,), "1_anchor": (1, None), "5": (1, 2, 4, 8, None)}


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


def graphed(fn, dev):
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        for _ in range(3):
            fn()
    torch.cuda.current_stream(dev).wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = fn()
    g.replay()
    return g, out


def bench_op(dev, calls, repeats):
    N = H * W
    grid = reference.coords_grid(1, H, W)
    for K in (1, 5):
        R = K + 2
        fw = torch.stack([smooth(H, W, k, 6, 0.2) for k in range(K)])
        bw = torch.stack([-fw[k] + smooth(H, W, 100 + k, 0.4, 0.05) for k in range(K)]).to(dev)
        fw = fw.to(dev)
        g = torch.Generator().manual_seed(1)
        ring_pos = torch.cat([grid + smooth(H, W, 200 + r, 4, 0.0) for r in range(R)]).to(dev)
        ring_score = torch.rand(R, H, W, generator=g)
        ring_score[torch.rand(R, H, W, generator=g) < 0.1] = float("inf")
        ring_score = ring_score.to(dev)
        src = [K + 1] + list(range(K - 1))
        idx = torch.tensor(src + [K - 1], dtype=torch.int32, device=dev)
        act = torch.ones(K, dtype=torch.bool, device=dev)

        # the point form's per-frame state, as MultiFlowTracker keeps it, and its static inputs
        hist = [(ring_pos[r].reshape(2, N).t().contiguous()[None], ring_score[r].reshape(1, N).clone(),
                 ring_score[r].reshape(1, N) < float("inf")) for r in range(R)]
        starts, sscore = torch.zeros(K, N, 2, device=dev), torch.zeros(K, N, device=dev)
        svis = torch.ones(K, N, dtype=torch.bool, device=dev)
        inf = torch.full((1, N), float("inf"), device=dev)

        def dense():
            return ops.dense_multi_flow_step(fw, bw, ring_pos, ring_score, idx, act, *ALPHA)

        def points():
            for k, r in enumerate(src):
                p, s, v = hist[r]
                starts[k].copy_(p[0])
                sscore[k].copy_(s[0])
                svis[k].copy_(v[0])
            pts, score, vis, choice, err, cand = ops.multi_flow_track_points(fw, bw, starts, sscore, svis, act, *ALPHA)
            score = torch.where(vis, score, inf)
            return pts.clone(), score.clone(), vis.clone(), choice, err

        def points_op_only():
            return ops.multi_flow_track_points(fw, bw, starts, sscore, svis, act, *ALPHA)

        ring0 = ring_pos.clone(), ring_score.clone()
        g_points, o_points = graphed(points, dev)
        g_only, _ = graphed(points_op_only, dev)
        g_dense, o_dense = graphed(dense, dev)
        # the same step from the same state: the ring was written by the warm-up calls, so once more from a copy
        ring_pos.copy_(ring0[0])
        ring_score.copy_(ring0[1])
        g_dense.replay()
        agree = (o_dense[3].view(1, N) == o_points[3]).float().mean().item()
        same_pos = bool(((o_dense[0].view(2, N).t() == o_points[0][0]) | (o_points[0][0] != o_points[0][0])).all())
        t = {"dense_graph_us": [], "points_composite_graph_us": [], "points_op_only_graph_us": []}
        for _ in range(repeats):
            t["dense_graph_us"].append(device_ms(g_dense.replay, calls))
            t["points_composite_graph_us"].append(device_ms(g_points.replay, calls))
            t["points_op_only_graph_us"].append(device_ms(g_only.replay, calls))
        best = {k: min(v) for k, v in t.items()}
        # what the dense launch moves at the least, in fp32 planes: per slot the two flow fields (4) and the
        # state (3); the outputs (pos 2, score, choice, err 1 each, visible 1/4) and the ring row written (3)
        mb = (K * 7 + 8.25) * N * 4 / 1e6
        print(json.dumps({"bench": "dense_multi_flow_step", "K": K, "shape": [K, 2, H, W], "calls": calls,
                          **{k: [round(x * 1e3, 2) for x in v] for k, v in t.items()},
                          "composite_over_dense": round(best["points_composite_graph_us"] / best["dense_graph_us"], 2),
                          "op_only_over_dense": round(best["points_op_only_graph_us"] / best["dense_graph_us"], 2),
                          "dense_min_MB": round(mb, 1),
                          "dense_GBps_at_min_MB": round(mb / 1e3 / (best["dense_graph_us"] / 1e3), 1),
                          "visible_fraction": round(o_dense[2].float().mean().item(), 3),
                          "choice_agreement": round(agree, 4), "positions_bit_equal": same_pos}), flush=True)


def bench_tracker(dev, frames_n, repeats, mixed):
    torch.manual_seed(0)
    model = RAFT(make_args(small=True, mixed_precision=mixed)).to(dev).to(memory_format=torch.channels_last).eval()
    g = torch.Generator().manual_seed(1)
    pool = [(torch.rand(1, 3, H, W, generator=g) * 255).to(dev) for _ in range(8)]
    points = (torch.rand(1, 32, 2, generator=g) * 500).to(dev)
    trackers = {}
    for name, deltas in DELTAS.items():
        for cached in (False, True):
            kw = dict(iters=12, deltas=deltas, fb_alpha=ALPHA, cache_features=cached)
            tag = name + ("_cached" if cached else "")
            trackers["points32_" + tag] = (MultiFlowTracker(model, **kw), points)
            trackers["dense_" + tag] = (DenseMultiFlowTracker(model, **kw), None)

    def timed(trk, pts):
        def go():
            trk.reset()
            trk.step(pool[0]) if pts is None else trk.step(pool[0], pts)
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

    variants = {k: timed(*v) for k, v in trackers.items()}
    for fn in variants.values():  # capture + warm-up
        fn()
    ms = {k: [] for k in variants}
    for _ in range(repeats):
        for k, fn in variants.items():
            ms[k].append(round(fn(), 4))
    extra = {}
    for name in DELTAS:
        for tag in (name, name + "_cached"):
            p, d = ms["points32_" + tag], ms["dense_" + tag]
            extra[tag] = {"dense_minus_points32_us": round((min(d) - min(p)) * 1e3, 1),
                          "points32_spread_us": round((max(p) - min(p)) * 1e3, 1)}
    print(json.dumps({"bench": "dense_flow_tracker", "model": "raft-small", "precision": "bf16" if mixed else "fp32",
                      "size": [H, W], "iters": 12, "frames": frames_n, "ms_per_frame": ms, "difference": extra}),
          flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=200, help="timed op calls per repeat (at least 200)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--frames", type=int, default=100, help="timed frames per tracker repeat")
    ap.add_argument("--only", choices=("op", "tracker"), help="one of the two measurements")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_dense_flow needs a GPU")
    dev = torch.device("cuda", 0)
    ops._ext.load(raise_on_error=True)
    if a.only != "tracker":
        with torch.no_grad():
            bench_op(dev, max(200, a.calls), a.repeats)
    if a.only != "op":
        for mixed in (True, False):
            bench_tracker(dev, a.frames, a.repeats, mixed)


if __name__ == "__main__":
    main()
