#!/usr/bin/env python
"""Forward-backward check in the sequence tracker: what visibility costs.

    python scripts/bench_fb_check.py [--calls 200] [--repeats 3] [--frames 100]

1. Op time: ``ops.fb_consistency`` and ``ops.fb_track_points`` (32 points)
   (csrc/fb_check.hip), device events around ``--calls`` back-to-back calls at
   (1,2,512,640), on a ``smooth(amp=6, noise=0.2)`` forward field and its
   disturbed negation.  Next to each the ATen oracle (ops/reference.py) on the
   same device tensors.
2. Model time: RAFT-small, 512x640, 12 iterations, each form in its own
   hipGraph: one direction, the bidirectional pass, and both directions as
   ``model(cat[a,b], cat[b,a])``.
3. Tracker time: ms per frame, RAFT-small, 512x640, 32 points, 12 iterations,
   bf16 and fp32, frames already on the device, the variants alternating inside
   every repeat:
     tracker        SequenceTracker(fb_check=False)
     tracker_fb     SequenceTracker(fb_check=True): the bidirectional pass and
                    the fused op
     batched_aten   both directions from ``model(cat[a,b], cat[b,a])``, two
                    ATen ``sample_points`` chains (the forward flow at the
                    points, the backward flow at the targets) and the check in
                    ATen ops, with the same warm start, in one hipGraph too.

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
from raft_stir_amd.export.pointtrack import SequenceTracker, sample_points  # noqa: E402
from raft_stir_amd.models import RAFT  # noqa: E402
from raft_stir_amd.ops import reference  # noqa: E402

ALPHA = (0.01, 0.5)


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


def bench_ops(dev, calls, repeats):
    H, W = 512, 640
    fw = smooth(H, W, 0, 6, 0.2)[None].to(dev)
    bw = (-fw[0].cpu() + smooth(H, W, 100, 0.4, 0.05))[None].to(dev)
    g = torch.Generator().manual_seed(1)
    pts = (torch.rand(1, 32, 2, generator=g) * torch.tensor([W - 1.0, H - 1.0])).to(dev)
    variants = {
        "fb_consistency": (lambda: ops.fb_consistency(fw, bw, *ALPHA), lambda: reference.fb_consistency(fw, bw, *ALPHA)),
        "fb_track_points": (lambda: ops.fb_track_points(fw, bw, pts, *ALPHA),
                            lambda: reference.fb_track_points(fw, bw, pts, *ALPHA)),
    }
    for name, (hip, aten) in variants.items():
        for _ in range(20):
            hip()
            aten()
        t_hip, t_aten = [], []
        for _ in range(repeats):
            t_hip.append(device_ms(hip, calls))
            t_aten.append(device_ms(aten, max(20, calls // 10)))
        ok = hip()[-1]
        print(json.dumps({"bench": name, "shape": [1, 2, H, W], "points": 32 if "points" in name else None,
                          "calls": calls, "op_us": [round(v * 1e3, 2) for v in t_hip],
                          "aten_oracle_us": [round(v * 1e3, 1) for v in t_aten],
                          "ok_fraction": round(ok.float().mean().item(), 3)}), flush=True)


class BatchedAtenTracker:
    """The checked tracker from the interfaces that existed before the
    bidirectional pass and the fused op, graphed like SequenceTracker."""

    def __init__(self, model, iters):
        self.model, self.iters, self.st = model, iters, None

    def _run(self, st):
        a, b, p = st["i1"], st["i2"], st["p"]
        lo, up = self.model(torch.cat([a, b]), torch.cat([b, a]), iters=self.iters, flow_init=st["init"],
                            test_mode=True)
        H, W = up.shape[-2:]
        uv = sample_points(up[0:1], p)
        q = p + uv
        buv = sample_points(up[1:2], q)
        inside = ((p[..., 0] >= 0) & (p[..., 0] <= W - 1) & (p[..., 1] >= 0) & (p[..., 1] <= H - 1)
                  & (q[..., 0] >= 0) & (q[..., 0] <= W - 1) & (q[..., 1] >= 0) & (q[..., 1] <= H - 1))
        e2 = ((uv + buv) ** 2).sum(-1)
        m2 = (uv ** 2).sum(-1) + (buv ** 2).sum(-1)
        err = torch.where(inside, e2.sqrt(), torch.full_like(e2, float("inf")))
        ok = inside & (e2 <= ALPHA[0] * m2 + ALPHA[1])
        nxt = st["sgn"] * ops.forward_interpolate(st["sgn"] * lo)
        return q, err, ok, nxt

    @torch.no_grad()
    def capture(self, frame, points):
        dev = frame.device
        st = {"i1": frame.clone().contiguous(memory_format=torch.channels_last), "p": points.clone(),
              "init": torch.zeros(2, 2, frame.shape[-2] // 8, frame.shape[-1] // 8, device=dev),
              "sgn": torch.tensor([1.0, -1.0], device=dev).view(2, 1, 1, 1)}
        st["i2"] = st["i1"].clone()
        s = torch.cuda.Stream(device=dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(s):
            for _ in range(2):
                self._run(st)
        torch.cuda.current_stream(dev).wait_stream(s)
        st["graph"] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(st["graph"]):
            st["out"], st["err"], st["ok"], st["next"] = self._run(st)
        self.st = st

    @torch.no_grad()
    def first(self, frame, points):
        if self.st is None:
            self.capture(frame, points)
        self.st["i2"].copy_(frame)
        self.st["init"].zero_()
        self.points = points.clone()

    @torch.no_grad()
    def step(self, frame):
        st = self.st
        st["i1"].copy_(st["i2"])
        st["i2"].copy_(frame)
        st["p"].copy_(self.points)
        st["graph"].replay()
        st["init"].copy_(st["next"])
        self.points, self.fb_err, self.visible = st["out"].clone(), st["err"].clone(), st["ok"].clone()
        return self.points


def bench_tracker(dev, frames_n, repeats, mixed):
    torch.manual_seed(0)
    model = RAFT(make_args(small=True, mixed_precision=mixed)).to(dev).to(memory_format=torch.channels_last).eval()
    g = torch.Generator().manual_seed(1)
    pool = [(torch.rand(1, 3, 512, 640, generator=g) * 255).to(dev) for _ in range(8)]
    points = (torch.rand(1, 32, 2, generator=g) * 500).to(dev)
    plain = SequenceTracker(model, iters=12)
    checked = SequenceTracker(model, iters=12, fb_check=True, fb_alpha=ALPHA)
    batched = BatchedAtenTracker(model, 12)

    def timed(first, step):
        def go():
            first()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for t in range(1, frames_n + 1):
                step(pool[t % len(pool)])
            b.record()
            b.synchronize()
            return a.elapsed_time(b) / frames_n
        return go

    def first_of(trk):
        def first():
            trk.reset()
            trk.step(pool[0], points)
        return first

    variants = {"tracker": timed(first_of(plain), plain.step), "tracker_fb": timed(first_of(checked), checked.step),
                "batched_aten": timed(lambda: batched.first(pool[0], points), batched.step)}
    for fn in variants.values():  # capture + warm-up
        fn()
    ms = {k: [] for k in variants}
    for _ in range(repeats):
        for k, fn in variants.items():
            ms[k].append(round(fn(), 4))
    best = {k: min(v) for k, v in ms.items()}
    print(json.dumps({"bench": "sequence_tracker_fb_check", "model": "raft-small",
                      "precision": "bf16" if mixed else "fp32", "size": [512, 640], "points": 32, "iters": 12,
                      "frames": frames_n, "ms_per_frame": ms,
                      "fb_check_cost_ms": round(best["tracker_fb"] - best["tracker"], 4),
                      "fb_check_over_plain": round(best["tracker_fb"] / best["tracker"], 3),
                      "tracker_fb_over_batched_aten": round(best["tracker_fb"] / best["batched_aten"], 3)}),
          flush=True)


def bench_pass(dev, calls, repeats, mixed):
    """The model alone, each form captured in its own hipGraph."""
    torch.manual_seed(0)
    model = RAFT(make_args(small=True, mixed_precision=mixed)).to(dev).to(memory_format=torch.channels_last).eval()
    g = torch.Generator().manual_seed(1)
    a, b = ((torch.rand(1, 3, 512, 640, generator=g) * 255).to(dev).contiguous(memory_format=torch.channels_last)
            for _ in range(2))
    init1, init2 = torch.zeros(1, 2, 64, 80, device=dev), torch.zeros(2, 2, 64, 80, device=dev)
    forms = {
        "one_direction": lambda: model(a, b, iters=12, flow_init=init1, test_mode=True),
        "bidirectional": lambda: model(a, b, iters=12, flow_init=init2, test_mode=True, bidirectional=True),
        "batched_pairs": lambda: model(torch.cat([a, b]), torch.cat([b, a]), iters=12, flow_init=init2,
                                       test_mode=True),
    }
    graphs = {}
    with torch.no_grad():
        for name, fn in forms.items():
            s = torch.cuda.Stream(device=dev)
            s.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(s):
                for _ in range(2):
                    fn()
            torch.cuda.current_stream(dev).wait_stream(s)
            graphs[name] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[name]):
                out = fn()
            graphs[name].replay()
            del out
    ms = {k: [] for k in forms}
    for _ in range(repeats):
        for k, gr in graphs.items():
            ms[k].append(round(device_ms(gr.replay, calls), 4))
    best = {k: min(v) for k, v in ms.items()}
    print(json.dumps({"bench": "raft_pass_graphed", "model": "raft-small", "precision": "bf16" if mixed else "fp32",
                      "size": [512, 640], "iters": 12, "calls": calls, "ms_per_call": ms,
                      "bidirectional_over_batched_pairs": round(best["bidirectional"] / best["batched_pairs"], 3),
                      "bidirectional_over_one_direction": round(best["bidirectional"] / best["one_direction"], 3)}),
          flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=200, help="timed op calls per repeat (at least 200)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--frames", type=int, default=100, help="timed frames per tracker repeat")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_fb_check needs a GPU")
    dev = torch.device("cuda", 0)
    ops._ext.load(raise_on_error=True)
    bench_ops(dev, max(200, a.calls), a.repeats)
    for mixed in (True, False):
        bench_pass(dev, max(50, a.calls // 2), a.repeats, mixed)
        bench_tracker(dev, a.frames, a.repeats, mixed)


if __name__ == "__main__":
    main()
