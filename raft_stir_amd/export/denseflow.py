"""Long-term tracking of every pixel: the dense form of the multi-delta
tracker (MFT: Neoral, Serych, Matas, "MFT: Long-Term Tracking of Every
Pixel", WACV 2024).

:class:`MultiFlowTracker` (export/multiflow.py) applies MFT's selection rule
to a short list of query points that must be given with the first frame.  The
K bidirectional flow pairs it computes do not depend on the points, so the
same pass serves every pixel of the anchor frame: :class:`DenseMultiFlowTracker`
keeps, for every anchor pixel, its position and score in the last L + 1 frames
in a planar ring on the device and advances all of them in one launch per
step (ops.dense_multi_flow_step, csrc/dense_flow.hip).  The result is a
long-term flow field ``anchor -> t`` with a visibility map, and points can be
asked for after the sequence has run (:meth:`DenseMultiFlowTracker.query`).
"""
from __future__ import annotations

import torch

from .multiflow import MultiFlowTracker, ring_index_row, ring_index_table
from .pointtrack import NUMITERS


class DenseMultiFlowTracker(MultiFlowTracker):
    """Follow every pixel of the first frame through a video.

    ``step(frame)`` on the first frame (the anchor) returns the pixel grid
    itself, (1,2,H,W) with channel 0 = x; every later ``step(frame)`` returns
    ``pos``, the position in the new frame t of every pixel of the anchor
    frame.  The model pass, ``deltas``, the ``active`` slots, the warm start
    and ``cache_features`` are MultiFlowTracker's; the selection is its rule at
    every pixel::

        pos, score, visible, choice, fb_err, _ = ops.dense_multi_flow_step(
            up[:K], up[K:], ring_pos, ring_score, idx, active, *fb_alpha)

    ``ring_pos`` (L+2,2,H,W) and ``ring_score`` (L+2,H,W) hold what this
    tracker returned for the last L + 1 frames and for the anchor, in the row
    layout of the feature ring (:func:`ring_index_table`: frame t in row
    t % (L+1), row L+1 the anchor, which holds the grid with score 0).  The
    launch reads the rows of the slots' start frames in place and writes the
    new frame's row; a pixel that is not visible is stored with score +inf, so
    a stored score is finite iff the pixel was visible and no ring of flags is
    kept.

    After a step ``pos`` (1,2,H,W), ``visible``, ``score``, ``fb_err``
    (1,1,H,W) and ``delta`` (1,1,H,W) int32, the span chosen (0: the anchor,
    -1: no slot was active), describe the new frame; ``flow`` is ``pos`` minus
    the grid, the long-term flow anchor -> t.  On the GPU ``pos``, ``visible``,
    ``score``, ``fb_err``, ``delta`` and ``cand_err`` are the static outputs of
    the captured graph: they are valid until the next step, which overwrites
    them (``track()`` and ``flow`` return tensors of their own).  ``cand_err``
    (K,H,W) is None unless the tracker was built with ``cand_err=True``, which
    costs K planes of stores per step.  ``points`` stays None: there is no
    list of points.

    On the GPU a step is one captured hipGraph per (frame shape, deltas): the
    number of pixels is the frame's, so no N enters the key.  Before a replay
    the host issues the frame upload, one row of the index table, the
    ``active`` row when it changes and the init; there is no per-slot copy of
    dense state, with ``cache_features`` or without (without it the frame ring
    still needs one image copy per finite slot, as in MultiFlowTracker).  On a
    CPU model the same loop runs eagerly on the ATen oracle.
    """

    def __init__(self, model, iters: int = NUMITERS, deltas=(1, 2, 4, 8, None), fb_alpha=(0.01, 0.5),
                 warm_start: bool = True, cache_features: bool = False, cand_err: bool = False):
        self.want_cand_err = bool(cand_err)
        super().__init__(model, iters=iters, deltas=deltas, fb_alpha=fb_alpha, warm_start=warm_start,
                         cache_features=cache_features)

    def reset(self):
        """Forget the frames, the tracked field and the inits."""
        super().reset()
        self.pos = None

    # ------------------------------------------------------------------ public
    @torch.no_grad()
    def step(self, frame, points=None):
        if points is not None:
            raise ValueError("DenseMultiFlowTracker tracks every pixel: step() takes no points "
                             "(ask for them with query())")
        # the checks, the weights refresh and the dispatch are MultiFlowTracker's; its first step wants
        # points, and gets an empty list that _first / _first_cached ignore
        none = torch.empty(1, 0, 2) if self.t == 0 else None
        return super().step(frame, none)

    @property
    def flow(self):
        """The long-term flow anchor -> t, (1,2,H,W): ``pos`` minus the pixel grid."""
        return None if self.pos is None else self.pos - self._st["grid"]

    @torch.no_grad()
    def query(self, points):
        """points (1,N,2) xy in the anchor frame, asked after the fact ->
        (positions (1,N,2) in the current frame, visible (1,N) bool, score
        (1,N)): the bilinear sample of ``pos`` at the points, visible iff every
        pixel it is read from is, the score the worst of theirs
        (ops.reference.dense_query).  A point outside the anchor frame or
        non-finite comes back unchanged, not visible, with score +inf."""
        from ..ops import reference
        if self.pos is None:
            raise ValueError("query() needs a step first")
        if points.dim() != 3 or points.shape[0] != 1 or points.shape[2] != 2:
            raise ValueError(f"points must be (1,N,2), got {tuple(points.shape)}")
        return reference.dense_query(self.pos, self.score, points.to(self.pos.device, torch.float32))

    @torch.no_grad()
    def track(self, frames):
        """frames (T,1,3,H,W) or a list of (1,3,H,W) -> (flows (T,2,H,W), the
        long-term flow 0 -> t of every pixel, visible (T,1,H,W) bool);
        ``flows[0] == 0``."""
        if len(frames) < 1:
            raise ValueError("track() needs at least one frame")
        self.reset()
        flows, vis = [], []
        for t in range(len(frames)):
            self.step(frames[t])
            flows.append(self.flow[0])
            vis.append(self.visible[0].clone())
        return torch.stack(flows), torch.stack(vis)

    # ------------------------------------------------------------------- state
    def _dense_state(self, dev, frame):
        """The planar state ring, its index table and the constants of a frame's size."""
        from ..ops.reference import coords_grid
        R = self.L + 2
        H, W = frame.shape[-2:]
        table = ring_index_table(self.deltas)
        return {
            "ring_pos": torch.zeros(R, 2, H, W, device=dev),
            "ring_score": torch.zeros(R, H, W, device=dev),
            "grid": coords_grid(1, H, W, device=dev).contiguous(),
            "minus": torch.full((1, 1, H, W), -1, dtype=torch.int32, device=dev),
            "idx_table": torch.tensor(table, dtype=torch.int32, device=dev),
            "idx": torch.tensor(table[0], dtype=torch.int32, device=dev),
        }

    def _buffers(self, dev, frame):
        K, L = self.K, self.L
        H, W = frame.shape[-2:]
        fmt = torch.channels_last if dev.type == "cuda" else torch.contiguous_format
        st = self._common(dev, frame, 1)
        st.update({
            "i1": torch.zeros(K, 3, H, W, device=dev).contiguous(memory_format=fmt),
            "ring": torch.zeros(L, 3, H, W, device=dev).contiguous(memory_format=fmt),
            **self._dense_state(dev, frame),
        })
        return st

    def _buffers_cached(self, dev, frame):
        st = super()._buffers_cached(dev, frame, 1)  # encodes this frame into the feature rings
        for name in ("hist_p", "hist_s", "hist_v"):  # the point tracker's array-of-structs history
            del st[name]
        st.update(self._dense_state(dev, frame))
        return st

    def _run(self, st):
        K = self.K
        lo, up = self.model(st["i1"], st["frame"].expand(K, -1, -1, -1), iters=self.iters, flow_init=st["init"],
                            test_mode=True, bidirectional=True)
        return self._select(st, lo, up)

    def _run_cached(self, st):
        from ..ops import feature_ring_step, from_nhwc, to_nhwc
        K = self.K
        f, c = self.model.encode(st["frame"])
        feature_ring_step(st["ring_f"], st["ring_c"], to_nhwc(f), to_nhwc(c), st["idx"], st["x"], st["ctx"])
        x = from_nhwc(st["x"])
        lo, up = self.model.refine(x[:2 * K], x[K:], from_nhwc(st["ctx"]), iters=self.iters, flow_init=st["init"])
        return self._select(st, lo, up)

    def _select(self, st, lo, up):
        """Every pixel's choice among the K flow pairs, read from and written
        to the state ring in place, and the next init (MultiFlowTracker's)."""
        from ..ops import dense_multi_flow_step, forward_interpolate
        K = self.K
        pos, score, vis, choice, err, cand = dense_multi_flow_step(
            up[:K], up[K:], st["ring_pos"], st["ring_score"], st["idx"], st["active"], *self.fb_alpha,
            cand_err=self.want_cand_err)
        span = st["delta"].index_select(0, choice.clamp(min=0).view(-1).long()).view(choice.shape)
        delta = torch.where(choice >= 0, span, st["minus"])
        nxt = None
        if self.warm_start:
            lo32 = lo.float()
            nxt = st["scale"] * forward_interpolate(lo32 / st["scale"])
            nxt = torch.where(st["anchor"], lo32, nxt)
            # a slot that is inactive now starts its first active step from zeros
            nxt = torch.where(torch.cat([st["active"], st["active"]]).view(2 * K, 1, 1, 1), nxt, st["zero"])
        return lo, up, pos, score, vis, delta, err, cand, nxt

    def _capture(self, dev, st, frame):
        st["i1"].copy_(frame.expand(self.K, -1, -1, -1))
        st["frame"].copy_(frame)
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

    def _start(self, dev, st, frame):
        """The state of a sequence's first frame: the grid, score 0, in row 0
        (which the inactive slots name too) and in the anchor's row."""
        H, W = frame.shape[-2:]
        for row in (0, self.L + 1):
            st["ring_pos"][row].copy_(st["grid"][0])
            st["ring_score"][row].zero_()
        self._st, self._shape = st, tuple(frame.shape)
        self.pos = st["grid"].clone()
        self.visible = torch.ones(1, 1, H, W, dtype=torch.bool, device=dev)
        self.score = torch.zeros(1, 1, H, W, device=dev)
        self.fb_err = torch.zeros(1, 1, H, W, device=dev)
        self.delta = torch.zeros(1, 1, H, W, dtype=torch.int32, device=dev)
        self._next = st["zero"]
        self.next_init = self._next
        self.t = 1
        return self.pos

    def _first(self, dev, frame, points):
        key = (tuple(frame.shape), self.deltas)
        st = self.graphs.get(key)
        if st is None:
            st = self.graphs[key] = self._buffers(dev, frame)
            if dev.type == "cuda":
                self._capture(dev, st, frame)
        st["frame"].copy_(frame)
        st["ring"][0].copy_(st["frame"][0])
        if self.deltas[-1] is None:  # the anchor slot's image does not change within a sequence
            st["i1"][self.K - 1].copy_(st["frame"][0])
        return self._start(dev, st, frame)

    def _advance(self, frame):
        st, t, L = self._st, self.t, self.L
        for k, d in enumerate(self._finite):
            st["i1"][k].copy_(st["ring"][(t - d if t >= d else 0) % L])  # inactive: the oldest stored frame
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
            out = self._run(st)
        st["ring"][t % L].copy_(st["frame"][0])
        self._publish(st, out)
        return self.pos

    def _publish(self, st, out):
        """The attributes of a step: the graph's outputs themselves; the step is counted."""
        lo, up, pos, score, vis, delta, err, cand, nxt = out
        self.pos, self.score, self.visible = pos, score, vis
        self.delta, self.fb_err, self.cand_err = delta, err, cand
        K = self.K
        self.flow_low, self.flow_bw_low, self.flow_up, self.flow_bw_up = lo[:K], lo[K:], up[:K], up[K:]
        self._next = nxt if self.warm_start else st["zero"]
        self.flow_init, self.next_init = st["init"], self._next
        self.t += 1

    # ---------------------------------------------------------- cache_features
    def _first_cached(self, dev, frame, points):
        key = (tuple(frame.shape), self.deltas, "cache_features")
        st = self.graphs.get(key)
        if st is None:
            st = self.graphs[key] = self._buffers_cached(dev, frame)
            if dev.type == "cuda":
                self._capture_cached(dev, st)
        else:
            st["frame"].copy_(frame)
            if st["graph0"] is not None:
                st["graph0"].replay()
            else:
                self._run_first(st)
        return self._start(dev, st, frame)

    def _advance_cached(self, frame):
        super()._advance_cached(frame)
        return self.pos
