#!/usr/bin/env python
"""Hole in-painting on the GPU: what filling the holes of a forward splat costs.

    python scripts/bench_splat_inpaint.py [--calls 200] [--repeats 3] [--frames 40] [--only op|tracker]
                                          [--in_place]

1. Op time: ``ops.splat_inpaint`` (csrc/splat_inpaint.hip: column, row, apply)
   at 512x640 on the footprint-2 splat of the ``smooth`` and ``contract``
   fields of bench_forward_splat.py, one carried channel, at max_dist 2, 8, 32
   and unlimited.  Each call is captured with ``runtime.graph.capture`` and its
   replays are timed with device events.  Next to it: the ATen oracle
   (``reference.splat_inpaint``) run eagerly on the same GPU tensors, and the
   route a user has without the op: the splat's outputs copied to the host and
   the oracle on the CPU.  The byte floor is what the three launches must move
   without the searches and the gathers: src_index read, col and donor written
   and read, dist2 written (24 B/cell), and src_index, inv_pos and out written
   (12 + 4C B/cell).  ``--in_place`` sets RS_INPAINT_STAGE=0 before the
   extension loads, so that the row pass reads col through L2 and not from
   LDS: run the script once with and once without it to compare the two.
2. Tracker time: ``DenseMultiFlowTracker.track(frames, labels, inpaint=8)``
   against ``inpaint=0`` on the same tracker, RAFT-small, bf16, 512x640, 12
   iterations, ``cache_features``, frames on the device, uint8 labels, the two
   variants alternating inside every repeat.

Every tensor a captured graph reads or writes, every graph and every tracker
is kept in one list until ``main`` returns.  Every repeat is printed, one JSON
line per measurement.  Needs a GPU: there is no CPU fall-back.
"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import torch  # noqa: E402

import bench_forward_splat as B  # noqa: E402
from raft_stir_amd import ops  # noqa: E402
from raft_stir_amd.config import make_args  # noqa: E402
from raft_stir_amd.export.denseflow import DenseMultiFlowTracker  # noqa: E402
from raft_stir_amd.models import RAFT  # noqa: E402
from raft_stir_amd.ops import reference  # noqa: E402
from raft_stir_amd.runtime.graph import capture  # noqa: E402

H, W = B.H, B.W
RADII = (2, 8, 32, None)


def bench_op(dev, calls, repeats, keep, row_pass):
    N = H * W
    values = torch.randn(1, 1, H, W, generator=torch.Generator().manual_seed(2))
    d_val = values.to(dev)
    keep.append(d_val)
    for name, pos, score in B.fields():
        d_pos = pos.to(dev)
        src, cov, inv, _ = ops.forward_splat(d_pos, score.to(dev), None, footprint=2)
        keep += [d_pos, src, cov, inv]
        for R in RADII:
            Rn = max(H, W) if R is None else R

            def hip(R=R):
                return ops.splat_inpaint(src, d_pos, inv, d_val, max_dist=R, fill=0.0)

            def aten(Rn=Rn):
                return reference.splat_inpaint(src, d_pos, inv, d_val, Rn, 0.0)

            def host(Rn=Rn):
                return reference.splat_inpaint(src.cpu(), d_pos.cpu(), inv.cpu(), values, Rn, 0.0)

            graph, out = capture(dev, hip)
            keep += [graph, out]
            graph.replay()
            row = {"bench": "splat_inpaint", "field": name, "shape": [H, W], "footprint": 2, "C": 1,
                   "max_dist": "inf" if R is None else R, "row_pass": row_pass, "calls": calls,
                   "hip_graph_us": [round(B.device_us(graph.replay, calls), 2) for _ in range(repeats)]}
            ref = aten()
            keep.append(ref)
            row["aten_gpu_eager_us"] = [round(B.device_us(aten, 20 if Rn <= 32 else 3), 1) for _ in range(repeats)]
            row["bit_equal_to_aten_gpu"] = all(B.same(a, b) for a, b in zip(out, ref))
            torch.cuda.synchronize()
            times = []
            for _ in range(repeats if Rn <= 32 else 1):
                t0 = time.perf_counter()
                cpu = host()
                times.append(round((time.perf_counter() - t0) * 1e3, 2))
            row["copies_and_cpu_oracle_ms"] = times
            row["bit_equal_to_cpu_oracle"] = all(B.same(a.cpu(), b) for a, b in zip(out, cpu))
            floor_mb = (24 + 12 + 4) * N / 1e6
            best = min(row["hip_graph_us"])
            holes = ~cov
            row.update(holes=int(holes.sum()), filled=int((holes & (out[0] >= 0)).sum()),
                       floor_MB=round(floor_mb, 2), GBps_at_floor=round(floor_mb / 1e3 / (best / 1e6), 1),
                       aten_gpu_over_hip=round(min(row["aten_gpu_eager_us"]) / best, 1),
                       cpu_path_over_hip=round(min(times) * 1e3 / best, 1))
            print(json.dumps(row), flush=True)


def bench_tracker(dev, frames_n, repeats, keep):
    torch.manual_seed(0)
    model = RAFT(make_args(small=True, mixed_precision=True)).to(dev).to(memory_format=torch.channels_last).eval()
    g = torch.Generator().manual_seed(1)
    pool = [(torch.rand(1, 3, H, W, generator=g) * 255).to(dev) for _ in range(8)]
    frames = [pool[t % len(pool)] for t in range(frames_n)]
    labels = torch.randint(0, 255, (H, W), generator=g, dtype=torch.uint8).to(dev)
    trk = DenseMultiFlowTracker(model, iters=12, deltas=(1, 2, 4, 8, None), cache_features=True)
    keep += [model, pool, frames, labels, trk]

    def timed(R):
        def go():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = trk.track(frames, labels, inpaint=R)
            torch.cuda.synchronize()
            keep.append(out[-1][:1])
            return (time.perf_counter() - t0) * 1e3 / frames_n
        return go

    variants = {"inpaint_0": timed(0), "inpaint_8": timed(8)}
    for fn in variants.values():  # capture + warm-up
        fn()
    ms = {k: [] for k in variants}
    for _ in range(repeats):
        for k, fn in variants.items():
            ms[k].append(round(fn(), 4))
    print(json.dumps({"bench": "splat_inpaint_tracker", "model": "raft-small", "precision": "bf16", "size": [H, W],
                      "iters": 12, "deltas": "5", "frames": frames_n, "graphs": len(trk.graphs), "ms_per_frame": ms,
                      "added_us_per_frame": round((min(ms["inpaint_8"]) - min(ms["inpaint_0"])) * 1e3, 1),
                      "inpaint_0_spread_us": round((max(ms["inpaint_0"]) - min(ms["inpaint_0"])) * 1e3, 1),
                      "inpaint_8_spread_us": round((max(ms["inpaint_8"]) - min(ms["inpaint_8"])) * 1e3, 1)}),
          flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=200, help="timed op replays per repeat (at least 200)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--frames", type=int, default=40, help="frames per tracked sequence")
    ap.add_argument("--only", choices=("op", "tracker"), help="one of the two measurements")
    ap.add_argument("--in_place", action="store_true", help="row pass without LDS staging (RS_INPAINT_STAGE=0)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_splat_inpaint needs a GPU")
    if a.in_place:
        os.environ["RS_INPAINT_STAGE"] = "0"  # read once, at the op's first launch
    dev = torch.device("cuda", 0)
    ops._ext.load(raise_on_error=True)
    keep = []  # everything a graph touches lives until main returns
    with torch.no_grad():
        if a.only != "tracker":
            bench_op(dev, max(200, a.calls), max(3, a.repeats), keep, "in_place" if a.in_place else "lds")
        if a.only != "op":
            bench_tracker(dev, a.frames, max(3, a.repeats), keep)
    torch.cuda.synchronize()
    return keep


if __name__ == "__main__":
    main()
