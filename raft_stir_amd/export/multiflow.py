"""Multi-delta point tracking that recovers points after an occlusion (MFT:
Neoral, Serych, Matas, "MFT: Long-Term Tracking of Every Pixel", WACV 2024).

:class:`SequenceTracker` (export/pointtrack.py) builds every position on the
one before it, so a point carried away while something passes over it stays
wrong for the rest of the sequence.  :class:`MultiFlowTracker` estimates the
flow into every new frame over several spans at once, ``t-D -> t`` for every D
of ``deltas`` and ``0 -> t`` from the anchor frame, and lets each point take
the most reliable one (ops.multi_flow_track_points, csrc/multi_flow.hip): a
long span jumps over the occlusion and the anchor span carries no drift.
"""
from __future__ import annotations

import torch

from ..ops.multi_flow import MAX_SLOTS
from .pointtrack import NUMITERS


def _check_deltas(deltas):
    try:
        deltas = tuple(deltas)
    except TypeError:
        raise ValueError(f"deltas must be a sequence of positive ints, optionally ending in None, got {deltas!r}")
    if not 1 <= len(deltas) <= MAX_SLOTS:
        raise ValueError(f"deltas must have 1 to {MAX_SLOTS} entries, got {len(deltas)}")
    finite = deltas[:-1] if deltas[-1] is None else deltas
    for d in finite:
        if d is None:
            raise ValueError(f"None (the anchor frame) comes last in deltas, got {deltas!r}")
        if isinstance(d, bool) or not isinstance(d, int) or d < 1:
            raise ValueError(f"deltas must be positive ints, optionally ending in None, got {deltas!r}")
    if any(b <= a for a, b in zip(finite, finite[1:])):
        raise ValueError(f"deltas must be distinct and in growing order, got {deltas!r}")
    return deltas


class MultiFlowTracker:
    """Follow points through a video over several time spans at once.

    ``step(frame, points)`` on the first frame (the anchor) stores both and
    returns the points; every later ``step(frame)`` returns the (1,N,2)
    positions in the new frame t.  With K = len(deltas) slots, slot k spanning
    ``t-D_k -> t`` (``None``: the anchor frame, ``0 -> t``), a step is::

        lo, up = model(i1, frame x K, iters, flow_init=init, test_mode=True, bidirectional=True)   # batch K
        points, score, visible, choice, fb_err, cand_err = ops.multi_flow_track_points(
            up[:K], up[K:], starts, start_score, start_visible, active, *fb_alpha)

    ``i1[k]`` is frame t-D_k and ``starts[k]``, ``start_score[k]``,
    ``start_visible[k]`` are what this tracker returned for that frame (the
    anchor slot: the given points, score 0, visible).  Slot k is active once
    ``t >= D_k``, the anchor from t = 1; an inactive slot is fed the oldest
    stored frame and ignored.  Every point takes the candidate of the eligible
    slot (active, visible in its start frame, passing the forward-backward
    check) with the smallest ``score = start_score + fb_err``, the shortest
    span among equals.  A point without an eligible slot follows the shortest
    active span, as SequenceTracker would, with ``visible = 0``; its score is
    stored as +inf, so nothing that chains from it is taken for reliable
    before a longer span has found the point again.

    After a step ``visible``, ``score``, ``fb_err`` (1,N) and ``delta`` (1,N)
    int32, the span chosen (0: the anchor, -1: no slot was active), describe
    the returned positions; after the first step they are all true, zeros,
    zeros and 0.  ``flow_up``, ``flow_bw_up``, ``flow_low``, ``flow_bw_low``
    (K,2,..), ``flow_init``, ``next_init`` (2K,2,h,w: forward slots first) and
    ``cand_err`` (K,N) are readable until the next step.

    Warm start (``warm_start=True``), per slot from that slot's own last
    output ``lo``, all 2K fields in one ``ops.forward_interpolate`` call: a
    finite span D with direction sign g (+1 forward, -1 backward) starts the
    next step from ``(g D) * FI(lo / (g D))``: every sample moves by one
    frame's share of its vector (against it for the backward field) and
    carries the whole vector; for D = 1 that is SequenceTracker's rule bit for
    bit.  The anchor slot starts from ``lo`` unchanged in both directions: the
    forward field lives in the anchor frame's coordinates, which do not move;
    for the backward field, which lives in the current frame, this assumes no
    motion over one frame.  A slot that was inactive in the step before
    starts from zeros.

    On the GPU all of this is one captured hipGraph per (frame shape, N,
    deltas) over static buffers.  The frames of the last max(D) steps and what
    was returned for them stay on the device; before a replay the host issues
    only device-to-device copies chosen by indices it knows from t, so with
    frames and points on the device a step does not synchronise with the
    host, and a frame is uploaded once.  On a CPU model the same loop runs
    eagerly on the ATen oracle.
    """

    def __init__(self, model, iters: int = NUMITERS, deltas=(1, 2, 4, 8, None), fb_alpha=(0.01, 0.5),
                 warm_start: bool = True):
        self.model = model.eval()
        self.iters = iters
        self.deltas = _check_deltas(deltas)
        self.K = len(self.deltas)
        self._finite = [d for d in self.deltas if d is not None]
        self.L = max(self._finite, default=1)  # frames kept
        self.fb_alpha = (float(fb_alpha[0]), float(fb_alpha[1]))
        if not (self.fb_alpha[0] >= 0 and self.fb_alpha[1] >= 0):
            raise ValueError(f"fb_alpha must be two numbers >= 0, got {fb_alpha}")
        self.warm_start = warm_start
        self.graphs = {}
        self._wkey = None
        self.reset()

    def reset(self):
        """Forget the frames, the points and the inits."""
        self.t = 0
        self._st = None       # the buffers of the running sequence
        self._hist = None     # what was returned for the last L frames, by frame index mod L
        self._active_row = None
        self._next = None     # the init of the next step, (2K,2,h,w)
        self._shape = None
        self.points = self.visible = self.score = self.fb_err = self.delta = self.cand_err = None
        self.flow_up = self.flow_bw_up = self.flow_low = self.flow_bw_low = None
        self.flow_init = self.next_init = None

    # ------------------------------------------------------------------ public
    @torch.no_grad()
    def step(self, frame, points=None):
        if frame.dim() != 4 or frame.shape[0] != 1 or frame.shape[1] != 3:
            raise ValueError(f"frame must be (1,3,H,W), got {tuple(frame.shape)}")
        if frame.shape[-2] % 8 or frame.shape[-1] % 8:
            raise ValueError(f"frame height and width must be multiples of 8, got {tuple(frame.shape[-2:])}")
        if self._shape is not None and self._shape != tuple(frame.shape):
            raise ValueError(f"frame shape changed within a sequence: {self._shape} -> "
                             f"{tuple(frame.shape)} (call reset())")
        if self.t == 0:
            if points is None:
                raise ValueError("the first step of a sequence needs points")
            if points.dim() != 3 or points.shape[0] != 1 or points.shape[2] != 2:
                raise ValueError(f"points must be (1,N,2), got {tuple(points.shape)}")
        elif points is not None:
            raise ValueError("points are given with the first frame of a sequence only (call reset())")
        dev = next(self.model.parameters()).device
        if dev.type == "cuda":
            from ..runtime.weights import refresh_all, weights_key
            wkey = weights_key(self.model)
            if self._wkey is not None and wkey != self._wkey:
                refresh_all(self.model)  # weights moved since capture: re-pack into the captured storage
            self._wkey = wkey
        if self.t == 0:
            return self._first(dev, frame, points)
        return self._advance(frame)

    @torch.no_grad()
    def track(self, frames, points):
        """frames (T,1,3,H,W) or a list of (1,3,H,W); points (1,N,2) in the
        first frame -> (traj (T,N,2), visible (T,N) bool, score (T,N), delta
        (T,N) int32), ``traj[0] == points``."""
        if len(frames) < 1:
            raise ValueError("track() needs at least one frame")
        self.reset()
        traj, vis, score, delta = [], [], [], []
        for t in range(len(frames)):
            traj.append(self.step(frames[t], points if t == 0 else None)[0])
            vis.append(self.visible[0])
            score.append(self.score[0])
            delta.append(self.delta[0])
        return torch.stack(traj), torch.stack(vis), torch.stack(score), torch.stack(delta)

    # ------------------------------------------------------------------- state
    def _buffers(self, dev, frame, N):
        """The static inputs of a step, the frame ring and the constants."""
        K, L = self.K, self.L
        H, W = frame.shape[-2:]
        fmt = torch.channels_last if dev.type == "cuda" else torch.contiguous_format
        span = [float(d) if d is not None else 1.0 for d in self.deltas]
        table = [[(d is not None and t >= d) or (d is None and t >= 1) for d in self.deltas] for t in range(L + 1)]
        return {
            "i1": torch.zeros(K, 3, H, W, device=dev).contiguous(memory_format=fmt),
            "frame": torch.zeros(1, 3, H, W, device=dev).contiguous(memory_format=fmt),
            "starts": torch.zeros(K, N, 2, device=dev),
            "sscore": torch.zeros(K, N, device=dev),
            "svis": torch.ones(K, N, dtype=torch.bool, device=dev),
            "active": torch.ones(K, dtype=torch.bool, device=dev),
            "init": torch.zeros(2 * K, 2, H // 8, W // 8, device=dev),
            "zero": torch.zeros(2 * K, 2, H // 8, W // 8, device=dev),
            "ring": torch.zeros(L, 3, H, W, device=dev).contiguous(memory_format=fmt),
            # constants: g*D per field, the anchor's fields, D per slot, the active slots at t = 0..L
            "scale": torch.tensor(span + [-s for s in span], device=dev).view(2 * K, 1, 1, 1),
            "anchor": torch.tensor([d is None for d in self.deltas] * 2, device=dev).view(2 * K, 1, 1, 1),
            "delta": torch.tensor([d or 0 for d in self.deltas], dtype=torch.int32, device=dev),
            "table": torch.tensor(table, dtype=torch.bool, device=dev),
            "inf": torch.full((1, N), float("inf"), device=dev),
            "minus": torch.full((1, N), -1, dtype=torch.int32, device=dev),
            "graph": None,
        }

    def _run(self, st):
        """One step on the static inputs: (lo, up, points, score, visible,
        delta, fb_err, cand_err, next init)."""
        from ..ops import forward_interpolate, multi_flow_track_points
        K = self.K
        lo, up = self.model(st["i1"], st["frame"].expand(K, -1, -1, -1), iters=self.iters, flow_init=st["init"],
                            test_mode=True, bidirectional=True)
        pts, score, vis, choice, err, cand = multi_flow_track_points(
            up[:K], up[K:], st["starts"], st["sscore"], st["svis"], st["active"], *self.fb_alpha)
        score = torch.where(vis, score, st["inf"])  # a lost point: nothing chains from it with a finite score
        span = st["delta"].index_select(0, choice.clamp(min=0).view(-1).long()).view(choice.shape)
        delta = torch.where(choice >= 0, span, st["minus"])
        nxt = None
        if self.warm_start:
            lo32 = lo.float()
            nxt = st["scale"] * forward_interpolate(lo32 / st["scale"])
            nxt = torch.where(st["anchor"], lo32, nxt)
            # a slot that is inactive now starts its first active step from zeros
            nxt = torch.where(torch.cat([st["active"], st["active"]]).view(2 * K, 1, 1, 1), nxt, st["zero"])
        return lo, up, pts, score, vis, delta, err, cand, nxt

    def _capture(self, dev, st, frame, points):
        st["i1"].copy_(frame.expand(self.K, -1, -1, -1))
        st["frame"].copy_(frame)
        st["starts"].copy_(points.expand(self.K, -1, -1))
        s = torch.cuda.Stream(device=dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(s):
            for _ in range(2):
                self._run(st)
        torch.cuda.current_stream(dev).wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            st["out"] = self._run(st)
        st["graph"] = g

    def _first(self, dev, frame, points):
        N = points.shape[1]
        key = (tuple(frame.shape), N, self.deltas)
        st = self.graphs.get(key)
        if st is None:
            st = self.graphs[key] = self._buffers(dev, frame, N)
            if dev.type == "cuda":
                self._capture(dev, st, frame, points)
        self._st, self._shape = st, tuple(frame.shape)
        p = points.to(dev, torch.float32).clone()
        st["frame"].copy_(frame)
        st["ring"][0].copy_(st["frame"][0])
        self.points = p
        self.visible = torch.ones(1, N, dtype=torch.bool, device=dev)
        self.score = torch.zeros(1, N, device=dev)
        self.fb_err = torch.zeros(1, N, device=dev)
        self.delta = torch.zeros(1, N, dtype=torch.int32, device=dev)
        self._hist = [None] * self.L
        self._hist[0] = (self.points, self.score, self.visible)
        if self.deltas[-1] is None:  # the anchor slot's inputs do not change within a sequence
            k = self.K - 1
            st["i1"][k].copy_(st["frame"][0])
            st["starts"][k].copy_(p[0])
            st["sscore"][k].zero_()
            st["svis"][k].fill_(True)
        self._next = st["zero"]
        self.next_init = self._next
        self.t = 1
        return self.points

    def _advance(self, frame):
        st, t, L = self._st, self.t, self.L
        for k, d in enumerate(self._finite):
            src = (t - d if t >= d else 0) % L  # inactive: the oldest stored frame, frame 0
            p, s, v = self._hist[src]
            st["i1"][k].copy_(st["ring"][src])
            st["starts"][k].copy_(p[0])
            st["sscore"][k].copy_(s[0])
            st["svis"][k].copy_(v[0])
        row = min(t, L)
        if row != self._active_row:
            st["active"].copy_(st["table"][row])
            self._active_row = row
        st["frame"].copy_(frame)
        st["init"].copy_(self._next)
        if st["graph"] is not None:
            st["graph"].replay()
            out = st["out"]
        else:
            out = self._run(st)
        lo, up, pts, score, vis, delta, err, cand, nxt = out
        st["ring"][t % L].copy_(st["frame"][0])
        self.points, self.score, self.visible = pts.clone(), score.clone(), vis.clone()
        self.delta, self.fb_err, self.cand_err = delta.clone(), err.clone(), cand
        self._hist[t % L] = (self.points, self.score, self.visible)
        K = self.K
        self.flow_low, self.flow_bw_low, self.flow_up, self.flow_bw_up = lo[:K], lo[K:], up[:K], up[K:]
        self._next = nxt if self.warm_start else st["zero"]
        self.flow_init, self.next_init = st["init"], self._next
        self.t = t + 1
        return self.points
