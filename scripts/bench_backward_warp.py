#!/usr/bin/env python
"""Backward warp of an image through the dense track field: what it costs.

    python scripts/bench_backward_warp.py [--calls 200] [--repeats 3] [--frames 40] [--only op|tracker]

1. Op time: ``ops.backward_warp`` (csrc/backward_warp.hip, one launch) at
   512x640, fp32 and uint8 images, planar and channels-last, C = 1, 3 and 4,
   on the two fields of bench_reanchor.py: ``smooth``, the pixel grid plus
   ``smooth(amp=6, noise=0.2)``, and ``scatter``, every cell reading a random
   place of the image (no two neighbouring threads read neighbouring pixels);
   10 % of the cells are not valid.  The call writes into buffers of the
   caller's, is captured with ``runtime.graph.capture`` and its replays are
   timed with device events.  Next to it: the ATen oracle
   (``reference.backward_warp``) run eagerly on the same GPU tensors, and, for
   fp32 and for orientation only (it is not bit-equal: another border rule, no
   validity), ``grid_sample(align_corners=True)`` plus the masking.  The byte
   floor is what the launch must move if every source pixel were read once:
   per pixel C elements of the source, 8 B of coords, 1 B of valid, C elements
   of the output and 1 B of ok.
2. Tracker time: RAFT-small, bf16, 512x640, 12 iterations, ``cache_features``,
   five deltas, frames on the device: a sequence of plain ``step`` calls
   against one of ``step`` + ``stabilize()``, the two alternating inside every
   repeat of one process.

Every tensor a captured graph reads or writes, every graph and every tracker
is kept in one list until ``main`` returns.  Every repeat is printed, one JSON
line per measurement.  Needs a GPU: there is no CPU fall-back.
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


def smooth(H, W, seed, amp, noise):
    g = torch.Generator().manual_seed(seed)
    lo = torch.randn(1, 2, max(2, H // 8), max(2, W // 8), generator=g) * amp
    f = F.interpolate(lo, size=(H, W), mode="bilinear", align_corners=True)[0]
    return f + noise * torch.randn(2, H, W, generator=g)


def fields():
    g = torch.Generator().manual_seed(3)
    yield "smooth", (reference.coords_grid(1, H, W) + smooth(H, W, 0, 6, 0.2)[None]).contiguous()
    scatter = torch.rand(1, 2, H, W, generator=g) * torch.tensor([W - 1.0, H - 1.0]).view(1, 2, 1, 1)
    yield "scatter", scatter.contiguous()


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


def grid_sample_masked(img, coords, valid):
    """For orientation: the library's sampler on normalised coordinates, then the mask."""
    _, _, Hs, Ws = img.shape
    x, y = coords[:, 0], coords[:, 1]
    grid = torch.stack([2 * x / (Ws - 1) - 1, 2 * y / (Hs - 1) - 1], dim=-1)
    out = F.grid_sample(img, grid, mode="bilinear", padding_mode="zeros", align_corners=True)
    ok = valid & (x >= 0)[:, None] & (x <= Ws - 1)[:, None] & (y >= 0)[:, None] & (y <= Hs - 1)[:, None]
    return torch.where(ok, out, torch.zeros_like(out)), ok


def bench_op(dev, calls, repeats, keep):
    N = H * W
    g = torch.Generator().manual_seed(5)
    valid = (torch.rand(1, 1, H, W, generator=g) < 0.9).to(dev)
    for fname, coords in fields():
        coords = coords.to(dev)
        keep += [coords, valid]
        for dt in (torch.float32, torch.uint8):
            for C in (1, 3, 4):
                base = torch.rand(1, C, H, W, generator=g) * 255
                base = base.to(dt).to(dev)
                for layout in ("planar", "channels_last"):
                    img = base if layout == "planar" else base.contiguous(memory_format=torch.channels_last)
                    out = (torch.empty(1, C, H, W, dtype=dt, device=dev),
                           torch.empty(1, 1, H, W, dtype=torch.bool, device=dev))
                    keep += [img, out]

                    def hip(img=img, out=out):
                        return ops.backward_warp(img, coords, valid, 0, out=out)

                    def aten(img=img):
                        return reference.backward_warp(img, coords, valid, 0)

                    graph, _ = capture(dev, hip)
                    keep.append(graph)
                    graph.replay()
                    ref = aten()
                    es = img.element_size()
                    row = {"bench": "backward_warp", "field": fname, "dtype": str(dt).split(".")[-1], "C": C,
                           "layout": layout, "shape": [H, W], "calls": calls,
                           "hip_graph_us": [round(device_us(graph.replay, calls), 2) for _ in range(repeats)],
                           "aten_gpu_eager_us": [round(device_us(aten, 20), 1) for _ in range(repeats)],
                           "bit_equal_to_aten_gpu": all(same(a, b) for a, b in zip(out, ref)),
                           "bit_equal_to_cpu_oracle": all(same(a.cpu(), b) for a, b in zip(
                               out, reference.backward_warp(img.cpu(), coords.cpu(), valid.cpu(), 0)))}
                    if dt == torch.float32:
                        def lib(img=img):
                            return grid_sample_masked(img, coords, valid)
                        lib()
                        row["grid_sample_masked_eager_us"] = [round(device_us(lib, 20), 1) for _ in range(repeats)]
                    floor_mb = (2 * C * es + 10) * N / 1e6
                    best = min(row["hip_graph_us"])
                    row.update(ok=round(out[1].float().mean().item(), 3), floor_MB=round(floor_mb, 2),
                               GBps_at_floor=round(floor_mb / 1e3 / (best / 1e6), 1),
                               aten_gpu_over_hip=round(min(row["aten_gpu_eager_us"]) / best, 1))
                    print(json.dumps(row), flush=True)


def bench_tracker(dev, frames_n, repeats, keep):
    torch.manual_seed(0)
    model = RAFT(make_args(small=True, mixed_precision=True)).to(dev).to(memory_format=torch.channels_last).eval()
    g = torch.Generator().manual_seed(1)
    pool = [(torch.rand(1, 3, H, W, generator=g) * 255).to(dev) for _ in range(8)]
    frames = [pool[t % len(pool)] for t in range(frames_n)]
    trk = DenseMultiFlowTracker(model, iters=12, deltas=(1, 2, 4, 8, None), cache_features=True)
    keep += [model, pool, frames, trk]

    def run(stabilize):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        trk.reset()
        for t in range(frames_n):
            trk.step(frames[t])
            if stabilize:
                last = trk.stabilize()
        torch.cuda.synchronize()
        if stabilize:
            keep.append(last[0][:, :1, :1, :1].clone())
        return (time.perf_counter() - t0) * 1e3 / frames_n

    variants = {"plain": lambda: run(False), "stabilized": lambda: run(True)}
    for fn in variants.values():  # capture + warm-up
        fn()
    ms = {k: [] for k in variants}
    for _ in range(repeats):
        for k, fn in variants.items():
            ms[k].append(round(fn(), 4))
    print(json.dumps({"bench": "stabilize_tracker", "model": "raft-small", "precision": "bf16", "size": [H, W],
                      "iters": 12, "deltas": 5, "frames": frames_n, "graphs": len(trk.graphs), "ms_per_frame": ms,
                      "added_us_per_frame": round((min(ms["stabilized"]) - min(ms["plain"])) * 1e3, 1),
                      "plain_spread_us": round((max(ms["plain"]) - min(ms["plain"])) * 1e3, 1),
                      "stabilized_spread_us": round((max(ms["stabilized"]) - min(ms["stabilized"])) * 1e3, 1)}),
          flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=200, help="timed op replays per repeat (at least 200)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--frames", type=int, default=40, help="frames per tracked sequence")
    ap.add_argument("--only", choices=("op", "tracker"), help="one of the two measurements")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_backward_warp needs a GPU")
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
