#!/usr/bin/env python
"""Forward splatting on the GPU: what the inverse map of a dense track field costs.

    python scripts/bench_forward_splat.py [--calls 200] [--repeats 3] [--frames 40] [--only op|tracker]

1. Op time: ``ops.forward_splat`` (csrc/forward_splat.hip: clear, scatter,
   resolve) at 512x640 with footprints 1 and 2 and C = 0 and 1 carried
   channels, on two fields: ``smooth``, the pixel grid plus
   ``smooth(amp=6, noise=0.2)`` as in bench_dense_flow.py with 10 % of the
   scores +inf, and ``contract``, the grid contracted by 0.5 about the centre
   with a jitter of a quarter pixel and scores from a short list (four sources
   per cell on average, many ties).  Each call is captured with
   ``runtime.graph.capture`` and its replays are timed with device events.
   Next to it: the ATen oracle (``reference.forward_splat``) run eagerly on
   the same GPU tensors (or the error it raises there), and what track.py did
   before the kernel: two copies to the host and the oracle on the CPU.  The
   byte floor is what the three launches must move without the atomics and
   the gathers: 3 planes read, 8 B/cell cleared, 8 B/cell resolved and
   13 + 4C B/cell written.
2. Tracker time: ``DenseMultiFlowTracker.track(frames, labels)`` against
   ``track(frames)`` on the same tracker, RAFT-small, bf16, 512x640, 12
   iterations, ``cache_features``, frames on the device, for uint8 labels (the
   splat, one gather along ``src_index`` and a ``where``) and fp32 labels (the
   splat carries them), the three variants alternating inside every repeat.

Every tensor a captured graph reads or writes, every graph and every tracker
is kept in one list until ``main`` returns; nothing is deleted and the
allocator's cache is never emptied.  The op section builds no graph of the
dense step or of a tracker; the tracker section uses public tracker methods
only.  Every repeat is printed, one JSON line per measurement.  Needs a GPU:
there is no CPU fall-back.
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


def fields():
    grid = reference.coords_grid(1, H, W)
    g = torch.Generator().manual_seed(1)
    score = torch.rand(1, 1, H, W, generator=g)
    score[torch.rand(1, 1, H, W, generator=g) < 0.1] = INF
    yield "smooth", (grid + smooth(H, W, 0, 6, 0.2)[None]).contiguous(), score
    centre = torch.tensor([(W - 1) / 2, (H - 1) / 2]).view(1, 2, 1, 1)
    pos = centre + (grid - centre) * 0.5 + (torch.rand(1, 2, H, W, generator=g) * 0.5 - 0.25)
    levels = torch.tensor([0.0, 0.5, 0.5, 1.0, 2.0])
    yield "contract", pos.contiguous(), levels[torch.randint(0, len(levels), (1, 1, H, W), generator=g)]


def atomics(pos, score, footprint):
    """How many offers the scatter makes (one atomicMin each), by the rule."""
    x, y, s = pos[0, 0], pos[0, 1], score[0, 0]
    src = (s >= 0) & (s < INF) & (x > -1) & (x < W) & (y > -1) & (y < H)
    x, y = torch.where(src, x, torch.zeros_like(x)), torch.where(src, y, torch.zeros_like(y))
    if footprint == 1:
        nx, ny = torch.round(x), torch.round(y)
        return int((src & (nx >= 0) & (nx < W) & (ny >= 0) & (ny < H)).sum())
    x0, y0 = torch.floor(x), torch.floor(y)
    wx, wy = x - x0, y - y0
    n = 0
    for dx, dy, w in ((0, 0, (1 - wx) * (1 - wy)), (1, 0, wx * (1 - wy)), (0, 1, (1 - wx) * wy), (1, 1, wx * wy)):
        xi, yi = x0 + dx, y0 + dy
        n += int((src & (w != 0) & (xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)).sum())
    return n


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
    g = torch.Generator().manual_seed(2)
    values = torch.randn(1, 1, H, W, generator=g)
    for name, pos, score in fields():
        d_pos, d_score, d_val = pos.to(dev), score.to(dev), values.to(dev)
        keep += [d_pos, d_score, d_val]
        for footprint in (1, 2):
            for C in (0, 1):
                vals = d_val if C else None

                def hip(vals=vals, footprint=footprint):
                    return ops.forward_splat(d_pos, d_score, vals, footprint=footprint, fill=0.0)

                def aten(vals=vals, footprint=footprint):
                    return reference.forward_splat(d_pos, d_score, vals, footprint, 0.0)

                def host(footprint=footprint):
                    return reference.forward_splat(d_pos.cpu(), d_score.cpu(), values if C else None, footprint, 0.0)

                graph, out = capture(dev, hip)
                keep += [graph, out]
                graph.replay()
                row = {"bench": "forward_splat", "field": name, "shape": [H, W], "footprint": footprint, "C": C,
                       "calls": calls, "hip_graph_us": [round(device_us(graph.replay, calls), 2)
                                                        for _ in range(repeats)]}
                try:
                    ref = aten()
                    keep.append(ref)
                    row["aten_gpu_eager_us"] = [round(device_us(aten, 20), 1) for _ in range(repeats)]
                    row["bit_equal_to_aten_gpu"] = all(same(a, b) for a, b in zip(out, ref) if a is not None)
                except Exception as e:  # what the device refuses is part of the record
                    row["aten_gpu_error"] = f"{type(e).__name__}: {str(e)[:200]}"
                torch.cuda.synchronize()
                times = []
                for _ in range(repeats):
                    t0 = time.perf_counter()
                    cpu = host()
                    times.append(round((time.perf_counter() - t0) * 1e3, 2))
                row["copies_and_cpu_oracle_ms"] = times
                row["bit_equal_to_cpu_oracle"] = all(same(a.cpu(), b) for a, b in zip(out, cpu) if a is not None)
                floor_mb = (12 + 8 + 8 + 13 + 4 * C) * N / 1e6
                best = min(row["hip_graph_us"])
                row.update(covered=round(out[1].float().mean().item(), 3), atomics=atomics(pos, score, footprint),
                           floor_MB=round(floor_mb, 2), GBps_at_floor=round(floor_mb / 1e3 / (best / 1e6), 1))
                if "aten_gpu_eager_us" in row:
                    row["aten_gpu_over_hip"] = round(min(row["aten_gpu_eager_us"]) / best, 1)
                row["cpu_path_over_hip"] = round(min(times) * 1e3 / best, 1)
                print(json.dumps(row), flush=True)


def bench_tracker(dev, frames_n, repeats, keep):
    torch.manual_seed(0)
    model = RAFT(make_args(small=True, mixed_precision=True)).to(dev).to(memory_format=torch.channels_last).eval()
    g = torch.Generator().manual_seed(1)
    pool = [(torch.rand(1, 3, H, W, generator=g) * 255).to(dev) for _ in range(8)]
    frames = [pool[t % len(pool)] for t in range(frames_n)]
    labels = {"uint8": torch.randint(0, 255, (H, W), generator=g, dtype=torch.uint8).to(dev),
              "fp32": torch.randn(1, 1, H, W, generator=g).to(dev)}
    keep += [model, pool, frames, labels]
    for tag, deltas in (("1_anchor", (1, None)), ("5", (1, 2, 4, 8, None))):
        trk = DenseMultiFlowTracker(model, iters=12, deltas=deltas, cache_features=True)
        keep.append(trk)

        def timed(lab):
            def go():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = trk.track(frames) if lab is None else trk.track(frames, lab)
                torch.cuda.synchronize()
                keep.append(out[-1][:1])
                return (time.perf_counter() - t0) * 1e3 / frames_n
            return go

        variants = {"plain": timed(None), "uint8": timed(labels["uint8"]), "fp32": timed(labels["fp32"])}
        for fn in variants.values():  # capture + warm-up
            fn()
        ms = {k: [] for k in variants}
        for _ in range(repeats):
            for k, fn in variants.items():
                ms[k].append(round(fn(), 4))
        extra = {k: {"added_us_per_frame": round((min(ms[k]) - min(ms["plain"])) * 1e3, 1),
                     "spread_us": round((max(ms[k]) - min(ms[k])) * 1e3, 1)} for k in ("uint8", "fp32")}
        extra["plain_spread_us"] = round((max(ms["plain"]) - min(ms["plain"])) * 1e3, 1)
        print(json.dumps({"bench": "forward_splat_tracker", "model": "raft-small", "precision": "bf16",
                          "size": [H, W], "iters": 12, "deltas": tag, "frames": frames_n, "graphs": len(trk.graphs),
                          "ms_per_frame": ms, "difference": extra}), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=200, help="timed op replays per repeat (at least 200)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--frames", type=int, default=40, help="frames per tracked sequence")
    ap.add_argument("--only", choices=("op", "tracker"), help="one of the two measurements")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_forward_splat needs a GPU")
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
