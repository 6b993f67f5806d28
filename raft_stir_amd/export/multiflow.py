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
from .pointtrack import (NUMITERS, check_step_inputs, check_tracker_options, encode_and_gather, encode_first,
                         image_buffer)


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
    """The index rows of the tracker's rings (of frames, or of features with
    ``cache_features``, and of what was returned for them), one per step:
    ``[src_0 .. src_{K-1}, dst]``, the ring row each slot reads and the row
    the new frame is written to (ops.feature_ring_step).  A ring has
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
    deltas) over static buffers.  The last L + 1 frames (L the longest finite
    span) stay on the device in a ring of L + 2 rows, and what was returned
    for them and for the anchor in rings ``hist_p`` / ``hist_s`` / ``hist_v``
    of the same row layout (:func:`ring_index_table`).  The graph gathers the
    starts from the rows ``idx[:K]`` and stores the new result in row
    ``idx[K]``.  Before a replay the host issues the frame upload, one row of
    the index table into ``idx``, the ``active`` row when it changes, the
    init and one image copy per finite slot from the frame ring into ``i1``,
    and after it one of the new frame into the ring, the rows taken from the
    same table row (the anchor's image stays in ``i1``).  No state is copied
    per slot, and with frames and points on the device a step does not
    synchronise with the host; a frame is uploaded once.  The first frame of
    a sequence is stored by a small graph of its own.  On a CPU model the
    same step runs eagerly on the ATen oracle.

    ``cache_features=True`` encodes every frame once.  The step above runs
    both encoders on 2K images, K of them the new frame and the others frames
    that were encoded before.  Instead the tracker keeps ``model.encode``'s
    output of the last L + 1 frames and of the anchor in a ring on the device,
    and a step is::

        f, c = model.encode(frame)                               # batch 1
        ops.feature_ring_step(ring_f, ring_c, f, c, idx, x, ctx) # store, and gather the 2K pairs
        lo, up = model.refine(x[:2K], x[K:], ctx, iters, flow_init=init)

    followed by the same selection and warm start.  The feature ring takes
    the frame ring's place, with the same rows, read and written inside the
    graph by the same ``idx``, so the host issues none of the image copies;
    the rest of the step is unchanged, and the small graph of the first
    frame encodes it.  The flows differ from the uncached tracker's only by
    the batch size at which the encoders ran.
    """

    _needs_points = True  # the first frame comes with the points to follow

    def __init__(self, model, iters: int = NUMITERS, deltas=(1, 2, 4, 8, None), fb_alpha=(0.01, 0.5),
                 warm_start: bool = True, cache_features: bool = False):
        self.model = model.eval()
        self.iters = iters
        self.deltas = _check_deltas(deltas)
        self.K = len(self.deltas)
        self.L = max((d for d in self.deltas if d is not None), default=1)  # frames kept
        self._table = ring_index_table(self.deltas)
        self.fb_alpha, self.cache_features = check_tracker_options(model, fb_alpha, cache_features)
        self.warm_start = warm_start
        self.graphs = {}
        self._wkey = None
        self.reset()

    def reset(self):
        """Forget the frames, the points and the inits."""
        self.t = 0
        self._st = None       # the buffers of the running sequence
        self._active_row = None
        self._next = None     # the init of the next step, (2K,2,h,w)
        self._shape = None
        self.points = self.visible = self.score = self.fb_err = self.delta = self.cand_err = None
        self.flow_up = self.flow_bw_up = self.flow_low = self.flow_bw_low = None
        self.flow_init = self.next_init = None

    # ------------------------------------------------------------------ public
    @torch.no_grad()
    def step(self, frame, points=None):
        from ..runtime.weights import refresh_if_moved
        check_step_inputs(frame, self._shape, points if self.t == 0 else None)
        if self.t == 0 and points is None and self._needs_points:
            raise ValueError("the first step of a sequence needs points")
        if self.t > 0 and points is not None:
            raise ValueError("points are given with the first frame of a sequence only (call reset())")
        dev = next(self.model.parameters()).device
        if dev.type == "cuda":
            self._wkey = refresh_if_moved(self.model, self._wkey)
        return self._first(dev, frame, points) if self.t == 0 else self._advance(frame)

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
    def _buffers(self, dev, frame, points):
        """The static inputs of a step, the rings and the constants.  Every
        ring has L + 2 rows in the layout of :func:`ring_index_table` (the
        frame ring leaves the anchor's row unused: its image stays in ``i1``);
        the feature ring of a ``cache_features`` tracker comes with the first frame."""
        K, L = self.K, self.L
        H, W = frame.shape[-2:]
        span = [float(d) if d is not None else 1.0 for d in self.deltas]
        active = [[(d is not None and t >= d) or (d is None and t >= 1) for d in self.deltas] for t in range(L + 1)]
        table = self._table
        st = {
            "frame": image_buffer((1, 3, H, W), dev),
            "active": torch.ones(K, dtype=torch.bool, device=dev),
            "init": torch.zeros(2 * K, 2, H // 8, W // 8, device=dev),
            "zero": torch.zeros(2 * K, 2, H // 8, W // 8, device=dev),
            "idx_table": torch.tensor(table, dtype=torch.int32, device=dev),
            "idx": torch.tensor(table[0], dtype=torch.int32, device=dev),
            # constants: g*D per field, the anchor's fields, D per slot, the active slots at t = 0..L
            "scale": torch.tensor(span + [-s for s in span], device=dev).view(2 * K, 1, 1, 1),
            "anchor": torch.tensor([d is None for d in self.deltas] * 2, device=dev).view(2 * K, 1, 1, 1),
            "delta": torch.tensor([d or 0 for d in self.deltas], dtype=torch.int32, device=dev),
            "table": torch.tensor(active, dtype=torch.bool, device=dev),
            "graph0": None, "graph": None,
            **self._history(dev, frame, points),
        }
        if not self.cache_features:
            st["ring"], st["i1"] = image_buffer((L + 2, 3, H, W), dev), image_buffer((K, 3, H, W), dev)
        return st

    def _history(self, dev, frame, points):
        """What was returned for the frame of every ring row, and the constants of its shape."""
        R, N = self.L + 2, points.shape[1]
        return {"hist_p": torch.zeros(R, N, 2, device=dev), "hist_s": torch.zeros(R, N, device=dev),
                "hist_v": torch.ones(R, N, dtype=torch.bool, device=dev),
                "inf": torch.full((1, N), float("inf"), device=dev),
                "minus": torch.full((1, N), -1, dtype=torch.int32, device=dev)}

    def _run_first(self, st):
        """The first frame of a sequence: its features into ring row 0, which
        the inactive slots read too, and into the anchor's row; without
        ``cache_features`` the frame into row 0 and into every slot of ``i1``,
        where the anchor slot's stays for the whole sequence."""
        if self.cache_features:
            encode_first(self.model, st, self.L + 2, (0, self.L + 1), self.K)
        else:
            st["ring"][0].copy_(st["frame"][0])
            st["i1"].copy_(st["frame"].expand(self.K, -1, -1, -1))

    def _flows(self, st):
        """(lo, up) of the K pairs in both directions: the only place in the
        graph where the step of a ``cache_features`` tracker differs."""
        K = self.K
        if self.cache_features:
            x, ctx = encode_and_gather(self.model, st)
            return self.model.refine(x[:2 * K], x[K:], ctx, iters=self.iters, flow_init=st["init"])
        return self.model(st["i1"], st["frame"].expand(K, -1, -1, -1), iters=self.iters, flow_init=st["init"],
                          test_mode=True, bidirectional=True)

    def _run(self, st):
        """One step on the static inputs: (lo, up, points, score, visible,
        delta, fb_err, cand_err, next init)."""
        lo, up = self._flows(st)
        pts, score, vis, choice, err, cand = self._choose(st, up)
        span = st["delta"].index_select(0, choice.clamp(min=0).view(-1).long()).view(choice.shape)
        delta = torch.where(choice >= 0, span, st["minus"])
        return lo, up, pts, score, vis, delta, err, cand, self._next_init(st, lo)

    def _choose(self, st, up):
        """The points' choice among the K flow pairs, from and into the history rings."""
        from ..ops import multi_flow_track_points
        K = self.K
        src, dst = st["idx"][:K], st["idx"][K:].long()
        pts, score, vis, choice, err, cand = multi_flow_track_points(
            up[:K], up[K:], st["hist_p"].index_select(0, src), st["hist_s"].index_select(0, src),
            st["hist_v"].index_select(0, src), st["active"], *self.fb_alpha)
        score = torch.where(vis, score, st["inf"])  # a lost point: nothing chains from it with a finite score
        st["hist_p"].index_copy_(0, dst, pts)
        st["hist_s"].index_copy_(0, dst, score)
        st["hist_v"].index_copy_(0, dst, vis)
        return pts, score, vis, choice, err, cand

    def _next_init(self, st, lo):
        """The warm start of the next step from this step's ``lo`` (None without)."""
        from ..ops import forward_interpolate
        if not self.warm_start:
            return None
        lo32 = lo.float()
        nxt = st["scale"] * forward_interpolate(lo32 / st["scale"])
        nxt = torch.where(st["anchor"], lo32, nxt)
        # a slot that is inactive now starts its first active step from zeros
        return torch.where(torch.cat([st["active"], st["active"]]).view(2 * self.K, 1, 1, 1), nxt, st["zero"])

    def _first(self, dev, frame, points):
        shape = tuple(frame.shape)
        key = ((shape,) + (() if points is None else (points.shape[1],)) + (self.deltas,)
               + (("cache_features",) if self.cache_features else ()))
        st = self.graphs.get(key)
        new = st is None
        if new:
            st = self.graphs[key] = self._buffers(dev, frame, points)
        st["frame"].copy_(frame)
        if st["graph0"] is not None:
            st["graph0"].replay()
        else:
            self._run_first(st)
        if new and dev.type == "cuda":
            # on the first step's inputs: the warm-up runs write the ring rows that the first step writes
            from ..runtime.graph import capture
            st["graph0"], _ = capture(dev, lambda: self._run_first(st))
            st["graph"], st["out"] = capture(dev, lambda: self._run(st))
        self._st, self._shape = st, shape
        self._next = st["zero"]
        self.next_init = self._next
        self.t = 1
        return self._start(st, dev, frame, points)

    def _start(self, st, dev, frame, points):
        """The state of a sequence's first frame: the points, score 0, visible,
        in row 0 (which the inactive slots name too) and in the anchor's row."""
        N = points.shape[1]
        self.points = points.to(dev, torch.float32).clone()
        self.visible = torch.ones(1, N, dtype=torch.bool, device=dev)
        self.score = torch.zeros(1, N, device=dev)
        self.fb_err = torch.zeros(1, N, device=dev)
        self.delta = torch.zeros(1, N, dtype=torch.int32, device=dev)
        for row in (0, self.L + 1):
            st["hist_p"][row].copy_(self.points[0])
            st["hist_s"][row].zero_()
            st["hist_v"][row].fill_(True)
        return self.points

    def _advance(self, frame):
        """Before the replay the host issues the frame upload, one row of the
        index table, the ``active`` row when it changes and the init; without
        ``cache_features`` also one image copy per finite slot and one after
        the replay, by the same row of the table.  The ring row written is
        never among the rows read (D <= L, :func:`ring_index_table`)."""
        st, t, L = self._st, self.t, self.L
        step = ring_index_row(t, L)
        st["idx"].copy_(st["idx_table"][step])
        if not self.cache_features:
            for k, d in enumerate(self.deltas):
                if d is not None:
                    st["i1"][k].copy_(st["ring"][self._table[step][k]])
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
        if not self.cache_features:
            st["ring"][self._table[step][-1]].copy_(st["frame"][0])
        lo, up, nxt = out[0], out[1], out[8]
        K = self.K
        self.flow_low, self.flow_bw_low, self.flow_up, self.flow_bw_up = lo[:K], lo[K:], up[:K], up[K:]
        self._next = nxt if self.warm_start else st["zero"]
        self.flow_init, self.next_init = st["init"], self._next
        self.t += 1
        return self._publish(*out[2:8])

    def _publish(self, pts, score, vis, delta, err, cand):
        """The attributes that describe the returned positions: tensors of the
        caller's own (the history rings keep theirs)."""
        self.points, self.score, self.visible = pts.clone(), score.clone(), vis.clone()
        self.delta, self.fb_err, self.cand_err = delta.clone(), err.clone(), cand
        return self.points
