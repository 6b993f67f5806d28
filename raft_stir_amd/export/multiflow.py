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


def ring_index_table(deltas):
    """The feature ring's index rows of a ``cache_features`` tracker, one per
    step: ``[src_0 .. src_{K-1}, dst]``, the ring row each slot reads and the
    row the new frame is written to (ops.feature_ring_step).  The ring has
    L + 2 rows, L the longest finite span: frame t lives in row t % (L + 1)
    and row L + 1 keeps the anchor frame.  An active slot of span D reads
    frame t - D, an inactive one frame 0 (row 0, not yet overwritten: t < L),
    the anchor slot row L + 1; as D <= L the row written is never read.  From
    t = L on the rows repeat with period L + 1, so 2L rows serve every t >= 1:
    :func:`ring_index_row` picks the one of step t."""
    deltas = _check_deltas(deltas)
    L = max((d for d in deltas if d is not None), default=1)
    rows = []
    for t in range(1, 2 * L + 1):
        src = [L + 1 if d is None else ((t - d) % (L + 1) if t >= d else 0) for d in deltas]
        rows.append(src + [t % (L + 1)])
    return rows


def ring_index_row(t: int, L: int) -> int:
    """The row of :func:`ring_index_table` for step t >= 1."""
    return t - 1 if t < L else L - 1 + (t - L) % (L + 1)


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

    ``cache_features=True`` encodes every frame once.  The step above runs
    both encoders on 2K images, K of them the new frame and the others frames
    that were encoded before.  Instead the tracker keeps ``model.encode``'s
    output of the last L + 1 frames and of the anchor in a ring on the device,
    and a step is::

        f, c = model.encode(frame)                               # batch 1
        ops.feature_ring_step(ring_f, ring_c, f, c, idx, x, ctx) # store, and gather the 2K pairs
        lo, up = model.refine(x[:2K], x[K:], ctx, iters, flow_init=init)

    followed by the same selection and warm start; what was returned for the
    stored frames lives in rings of the same row layout and is read and
    written inside the graph with the same ``idx`` (:func:`ring_index_table`).
    Before a replay the host issues the frame upload, one row of the index
    table, the ``active`` row when it changes and the init: no per-slot
    copies.  The first frame of a sequence is encoded by a small graph of its
    own.  The flows differ from the uncached tracker's only by the batch size
    at which the encoders ran.
    """

    def __init__(self, model, iters: int = NUMITERS, deltas=(1, 2, 4, 8, None), fb_alpha=(0.01, 0.5),
                 warm_start: bool = True, cache_features: bool = False):
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
        self.cache_features = bool(cache_features)
        if self.cache_features and not (hasattr(model, "encode") and hasattr(model, "refine")):
            raise ValueError("cache_features=True needs a model with encode() and refine()")
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
        if self.cache_features:
            return self._first_cached(dev, frame, points) if self.t == 0 else self._advance_cached(frame)
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
        return {
            "i1": torch.zeros(K, 3, H, W, device=dev).contiguous(memory_format=fmt),
            "starts": torch.zeros(K, N, 2, device=dev),
            "sscore": torch.zeros(K, N, device=dev),
            "svis": torch.ones(K, N, dtype=torch.bool, device=dev),
            "ring": torch.zeros(L, 3, H, W, device=dev).contiguous(memory_format=fmt),
            **self._common(dev, frame, N),
        }

    def _common(self, dev, frame, N):
        """What the uncached and the cached step share: the new frame, the
        active slots, the init and the constants."""
        K, L = self.K, self.L
        H, W = frame.shape[-2:]
        fmt = torch.channels_last if dev.type == "cuda" else torch.contiguous_format
        span = [float(d) if d is not None else 1.0 for d in self.deltas]
        table = [[(d is not None and t >= d) or (d is None and t >= 1) for d in self.deltas] for t in range(L + 1)]
        return {
            "frame": torch.zeros(1, 3, H, W, device=dev).contiguous(memory_format=fmt),
            "active": torch.ones(K, dtype=torch.bool, device=dev),
            "init": torch.zeros(2 * K, 2, H // 8, W // 8, device=dev),
            "zero": torch.zeros(2 * K, 2, H // 8, W // 8, device=dev),
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
        K = self.K
        lo, up = self.model(st["i1"], st["frame"].expand(K, -1, -1, -1), iters=self.iters, flow_init=st["init"],
                            test_mode=True, bidirectional=True)
        return self._select(st, lo, up, st["starts"], st["sscore"], st["svis"])

    def _select(self, st, lo, up, starts, sscore, svis):
        """The points' choice among the K flow pairs and the next init."""
        from ..ops import forward_interpolate, multi_flow_track_points
        K = self.K
        pts, score, vis, choice, err, cand = multi_flow_track_points(
            up[:K], up[K:], starts, sscore, svis, st["active"], *self.fb_alpha)
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
        st["ring"][t % L].copy_(st["frame"][0])
        self._publish(st, out)
        self._hist[t % L] = (self.points, self.score, self.visible)
        return self.points

    def _publish(self, st, out):
        """The attributes of a step from the graph's outputs; the step is counted."""
        lo, up, pts, score, vis, delta, err, cand, nxt = out
        self.points, self.score, self.visible = pts.clone(), score.clone(), vis.clone()
        self.delta, self.fb_err, self.cand_err = delta.clone(), err.clone(), cand
        K = self.K
        self.flow_low, self.flow_bw_low, self.flow_up, self.flow_bw_up = lo[:K], lo[K:], up[:K], up[K:]
        self._next = nxt if self.warm_start else st["zero"]
        self.flow_init, self.next_init = st["init"], self._next
        self.t += 1

    # ---------------------------------------------------------- cache_features
    def _buffers_cached(self, dev, frame, N):
        """The static buffers of the cached step: :meth:`_common`, the feature
        and history rings and the index table.
        The features' shapes and dtype come from encoding ``frame``, eagerly;
        the rings are left holding it as a sequence's first frame."""
        from ..ops import to_nhwc
        K, R = self.K, self.L + 2
        st = self._common(dev, frame, N)
        st["frame"].copy_(frame)
        f, c = self.model.encode(st["frame"])
        f, c = to_nhwc(f), to_nhwc(c)
        if f.dtype != c.dtype:
            raise ValueError(f"cache_features: encode() returned {f.dtype} features and {c.dtype} context")
        st.update({
            "ring_f": f.new_zeros((R,) + tuple(f.shape[1:])), "ring_c": c.new_zeros((R,) + tuple(c.shape[1:])),
            "x": f.new_zeros((3 * K,) + tuple(f.shape[1:])), "ctx": c.new_zeros((2 * K,) + tuple(c.shape[1:])),
            # what was returned for the frame of every ring row
            "hist_p": torch.zeros(R, N, 2, device=dev), "hist_s": torch.zeros(R, N, device=dev),
            "hist_v": torch.ones(R, N, dtype=torch.bool, device=dev),
            "idx_table": torch.tensor(ring_index_table(self.deltas), dtype=torch.int32, device=dev),
            "idx": torch.zeros(K + 1, dtype=torch.int32, device=dev),
            "graph0": None,
        })
        st["idx"].copy_(st["idx_table"][0])
        self._store_first(st, f, c)
        return st

    def _run_first(self, st):
        """The first frame of a sequence: encoded into row 0 and the anchor's row."""
        from ..ops import to_nhwc
        f, c = self.model.encode(st["frame"])
        self._store_first(st, to_nhwc(f), to_nhwc(c))

    def _store_first(self, st, f, c):
        for row in (0, self.L + 1):
            st["ring_f"][row].copy_(f[0])
            st["ring_c"][row].copy_(c[0])

    def _run_cached(self, st):
        """One step on the static inputs, as :meth:`_run`."""
        from ..ops import feature_ring_step, from_nhwc, to_nhwc
        K = self.K
        f, c = self.model.encode(st["frame"])
        feature_ring_step(st["ring_f"], st["ring_c"], to_nhwc(f), to_nhwc(c), st["idx"], st["x"], st["ctx"])
        x = from_nhwc(st["x"])
        lo, up = self.model.refine(x[:2 * K], x[K:], from_nhwc(st["ctx"]), iters=self.iters, flow_init=st["init"])
        idx = st["idx"].long()
        src, dst = idx[:K], idx[K:]
        out = self._select(st, lo, up, st["hist_p"].index_select(0, src), st["hist_s"].index_select(0, src),
                           st["hist_v"].index_select(0, src))
        st["hist_p"].index_copy_(0, dst, out[2])
        st["hist_s"].index_copy_(0, dst, out[3])
        st["hist_v"].index_copy_(0, dst, out[4])
        return out

    def _capture_cached(self, dev, st):
        s = torch.cuda.Stream(device=dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(s):
            for _ in range(2):
                self._run_first(st)
                self._run_cached(st)
        torch.cuda.current_stream(dev).wait_stream(s)
        g0 = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g0):
            self._run_first(st)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            st["out"] = self._run_cached(st)
        st["graph0"], st["graph"] = g0, g

    def _first_cached(self, dev, frame, points):
        N = points.shape[1]
        key = (tuple(frame.shape), N, self.deltas, "cache_features")
        st = self.graphs.get(key)
        if st is None:
            st = self.graphs[key] = self._buffers_cached(dev, frame, N)  # encodes this frame into the rings
            if dev.type == "cuda":
                self._capture_cached(dev, st)
        else:
            st["frame"].copy_(frame)
            if st["graph0"] is not None:
                st["graph0"].replay()
            else:
                self._run_first(st)
        self._st, self._shape = st, tuple(frame.shape)
        p = points.to(dev, torch.float32).clone()
        self.points = p
        self.visible = torch.ones(1, N, dtype=torch.bool, device=dev)
        self.score = torch.zeros(1, N, device=dev)
        self.fb_err = torch.zeros(1, N, device=dev)
        self.delta = torch.zeros(1, N, dtype=torch.int32, device=dev)
        # frame 0's row, which the inactive slots read too, and the anchor's
        for row in (0, self.L + 1):
            st["hist_p"][row].copy_(p[0])
            st["hist_s"][row].zero_()
            st["hist_v"][row].fill_(True)
        self._next = st["zero"]
        self.next_init = self._next
        self.t = 1
        return self.points

    def _advance_cached(self, frame):
        st, t, L = self._st, self.t, self.L
        st["idx"].copy_(st["idx_table"][ring_index_row(t, L)])
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
            out = self._run_cached(st)
        self._publish(st, out)
        return self.points
