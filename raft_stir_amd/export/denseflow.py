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
The inverse map, which anchor pixel sits on every cell of frame t, comes from
forward splatting (:meth:`DenseMultiFlowTracker.splat`, ops.forward_splat)
and carries labels of the first frame through the video
(:meth:`DenseMultiFlowTracker.warp_labels`); on the GPU it is the scatter and
resolve kernels of csrc/forward_splat.hip, an eager call after the step's
replay, on the CPU the ATen oracle.  The holes the splat leaves where the
scene stretches can be filled from the nearest covered cell within a radius
(``inpaint=R`` of the three methods, ops.splat_inpaint, csrc/splat_inpaint.hip).
On a long sequence the tracker can be re-anchored on the current frame
(:meth:`DenseMultiFlowTracker.reanchor`): the field so far is kept as a base and
every later field is composed with it (ops.dense_compose,
csrc/dense_compose.hip), so everything published stays indexed by the pixels of
the first frame.  Images move through the two maps by a bilinear backward warp
(ops.backward_warp, csrc/backward_warp.hip): the current frame into the first
frame's coordinates through ``pos`` (:meth:`DenseMultiFlowTracker.stabilize`),
an image drawn on the first frame into the current one through ``inv_pos``
(:meth:`DenseMultiFlowTracker.warp_image`).
"""
from __future__ import annotations

import torch

from .multiflow import MultiFlowTracker
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
    number of pixels is the frame's, so no N enters the key.  The step is
    MultiFlowTracker's with this selection in place of its own: before a
    replay the host issues the frame upload, one row of the index table, the
    ``active`` row when it changes and the init (without ``cache_features``
    also its image copy per finite slot), and no copy per slot of dense
    state.  On a CPU model the same step runs eagerly on the ATen oracle.

    Re-anchoring.  When most of the first frame has left the view, the pair
    ``anchor -> t`` is the hardest of the step and finally useless.
    :meth:`reanchor`, called after a step on frame r, keeps the published field
    ``0 -> r`` as a base and restarts the sequence with frame r as the anchor.
    From then on a step is the same graph, which now yields the inner field
    ``r -> t``, followed by one eager ``ops.dense_compose(base_pos, base_score,
    pos, score, delta, fb_err, out=...)`` on the same stream, and ``pos``,
    ``score``, ``visible``, ``delta`` and ``fb_err`` are the composed ones,
    ``0 -> t`` indexed by the pixels of frame 0 (static buffers of their own,
    valid until the next step), so ``flow``, :meth:`splat`,
    :meth:`warp_labels`, :meth:`query` and :meth:`track` work unchanged.  The
    inner field is ``anchor_pos``, ``anchor_score`` and ``anchor_visible``,
    indexed by the pixels of the current anchor, whose absolute frame index is
    ``anchor_frame``; ``cand_err`` stays the inner field's, indexed by the
    pixels of the current anchor.  Without a re-anchor the ``anchor_*``
    attributes are ``pos``, ``score`` and ``visible`` themselves, the op is
    never called, and bits, launches and published tensors are those of a
    tracker without the feature.  Re-anchors chain: the base becomes the
    composed field each time.  ``reanchor_every=N`` re-anchors after
    publishing the N-th frame past the current anchor, without a host
    synchronisation; ``reanchor_below=f``, 0 < f < 1, after publishing a frame
    on which fewer than f of the current anchor's pixels are visible
    (``anchor_visible``), which reads one scalar from the device per step: it
    is the one option that synchronises with the host.  The price: a pixel
    that is not visible on the re-anchor frame is lost for the rest of the
    sequence (its base score is +inf, and the old anchor slot that could have
    found it again is gone), the first step after a re-anchor starts cold, and
    positions pass through one more bilinear interpolation per re-anchor.
    """

    def __init__(self, model, iters: int = NUMITERS, deltas=(1, 2, 4, 8, None), fb_alpha=(0.01, 0.5),
                 warm_start: bool = True, cache_features: bool = False, cand_err: bool = False,
                 reanchor_every: int | None = None, reanchor_below: float | None = None):
        self.want_cand_err = bool(cand_err)
        if reanchor_every is not None and (isinstance(reanchor_every, bool) or not isinstance(reanchor_every, int)
                                           or reanchor_every < 1):
            raise ValueError(f"reanchor_every must be a positive int or None, got {reanchor_every!r}")
        if reanchor_below is not None and not 0.0 < float(reanchor_below) < 1.0:
            raise ValueError(f"reanchor_below must be in (0, 1) or None, got {reanchor_below!r}")
        self.reanchor_every = reanchor_every
        self.reanchor_below = None if reanchor_below is None else float(reanchor_below)
        super().__init__(model, iters=iters, deltas=deltas, fb_alpha=fb_alpha, warm_start=warm_start,
                         cache_features=cache_features)

    def reset(self):
        """Forget the frames, the tracked field, the base of a re-anchor and the inits."""
        super().reset()
        self.pos = None
        self.anchor_pos = self.anchor_score = self.anchor_visible = None
        self.anchor_frame = 0
        self._based = False   # a base field is held: the published field is composed with it

    # ------------------------------------------------------------------ public
    _needs_points = False

    @torch.no_grad()
    def step(self, frame, points=None):
        if points is not None:
            raise ValueError("DenseMultiFlowTracker tracks every pixel: step() takes no points "
                             "(ask for them with query())")
        super().step(frame)
        since = self.t - 1  # frames past the current anchor
        if since >= 1 and ((self.reanchor_every is not None and since >= self.reanchor_every)
                           or (self.reanchor_below is not None  # one scalar from the device: synchronises
                               and float(self.anchor_visible.float().mean()) < self.reanchor_below)):
            self.reanchor()
        return self.pos

    @torch.no_grad()
    def reanchor(self):
        """Make the current frame the anchor.  Valid after a step; before the
        first advance of a sequence (or right after a re-anchor) it does
        nothing.  The published ``pos`` and ``score`` are copied into the
        tracker's base buffers (one set per frame shape) and the sequence
        restarts on the current frame, which is still in the static frame
        buffer, through the first-frame path (one re-encode with
        ``cache_features``): the frame becomes the anchor in the feature or
        image ring and in the state ring, ``t`` counts from it, every init is
        zero and the finite slots become active again as frames arrive.  What
        is published for this frame stays what it was (the composition through
        the identity is not taken: a bilinear sample of the grid is not
        bit-equal to the point); from the next step on it is the composed
        field.  ``anchor_pos``, ``anchor_score`` and ``anchor_visible`` become
        the identity field of the new anchor.  No host synchronisation."""
        if self.t <= 1:
            return
        st = self._st
        dev = st["grid"].device
        H, W = st["grid"].shape[-2:]
        if "base_pos" not in st:
            st["base_pos"] = torch.empty(1, 2, H, W, device=dev)
            st["base_score"] = torch.empty(1, 1, H, W, device=dev)
            st["composed"] = (torch.empty(1, 2, H, W, device=dev), torch.empty(1, 1, H, W, device=dev),
                              torch.empty(1, 1, H, W, dtype=torch.bool, device=dev),
                              torch.empty(1, 1, H, W, dtype=torch.int32, device=dev),
                              torch.empty(1, 1, H, W, device=dev))
        st["base_pos"].copy_(self.pos)
        st["base_score"].copy_(self.score)
        if self._based:
            # what is published lives in the buffers the next composition writes: keep this frame's own
            self.pos, self.score, self.visible = self.pos.clone(), self.score.clone(), self.visible.clone()
            self.delta, self.fb_err = self.delta.clone(), self.fb_err.clone()
        if st["graph0"] is not None:
            st["graph0"].replay()
        else:
            self._run_first(st)
        self._seed(st)
        self.anchor_frame += self.t - 1
        self.t = 1
        self._active_row = None  # the active table starts from row 1 again
        self._next = st["zero"]
        self.next_init = self._next
        self._based = True
        self.anchor_pos = st["grid"].clone()
        self.anchor_score = torch.zeros(1, 1, H, W, device=dev)
        self.anchor_visible = torch.ones(1, 1, H, W, dtype=torch.bool, device=dev)

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
        (ops.dense_query: csrc/dense_compose.hip on the GPU, the ATen oracle on
        the CPU).  A point outside the anchor frame or non-finite comes back
        unchanged, not visible, with score +inf."""
        from ..ops import dense_query
        if self.pos is None:
            raise ValueError("query() needs a step first")
        if points.dim() != 3 or points.shape[0] != 1 or points.shape[2] != 2:
            raise ValueError(f"points must be (1,N,2), got {tuple(points.shape)}")
        return dense_query(self.pos, self.score, points.to(self.pos.device, torch.float32))

    @torch.no_grad()
    def splat(self, values=None, footprint: int = 2, fill: float = 0.0, inpaint: int | None = 0):
        """The inverse map of the current frame, by forward splatting
        (ops.forward_splat on ``pos`` and ``score``): for every cell of frame
        t the anchor pixel that sits there.  values (1,C,H,W) or None ->
        (src_index (1,1,H,W) int32, -1 at holes; covered (1,1,H,W) bool;
        inv_pos (1,2,H,W), the cell's position in the anchor frame, NaN at
        holes; out (1,C,H,W) fp32, ``values`` carried along and ``fill`` at
        holes, None without values).  On the first frame it is the identity:
        every cell is covered by itself.  The tensors are the caller's own,
        on the tracker's device.  On the GPU this is an eager call of
        csrc/forward_splat.hip on the current stream, after the step's replay:
        it reads the graph's static ``pos`` and ``score``, is not part of the
        step graph and does not synchronise with the host.

        ``inpaint`` = R > 0 (None: unlimited) fills every hole that has a
        covered cell within R cells from the nearest one (ops.splat_inpaint,
        csrc/splat_inpaint.hip on the GPU, right after the splat on the same
        stream): ``src_index``, ``inv_pos`` and ``out`` are the in-painted
        ones, ``covered`` stays the true coverage, so
        ``(src_index >= 0) & ~covered`` marks the in-painted cells.  With the
        default 0 the op is not called."""
        from ..ops import forward_splat, splat_inpaint
        if self.pos is None:
            raise ValueError("splat() needs a step first")
        if values is not None:
            values = values.to(self.pos.device)
        if inpaint == 0:  # None is unlimited, not 0
            return forward_splat(self.pos, self.score, values, footprint=footprint, fill=fill)
        src, covered, inv, _ = forward_splat(self.pos, self.score, None, footprint=footprint)
        src, _, _, inv, out = splat_inpaint(src, self.pos, inv, values, max_dist=inpaint, fill=fill)
        return src, covered, inv, out

    @torch.no_grad()
    def warp_labels(self, labels, footprint: int = 2, fill=0, inpaint: int | None = 0):
        """Carry labels of the anchor frame into the current frame.  labels
        (H,W), (1,1,H,W) or (1,C,H,W), of any dtype -> (warped, of labels'
        shape and dtype: at every cell the label of the anchor pixel that
        :meth:`splat` finds there, ``fill`` at holes; covered (1,1,H,W) bool).
        fp32 labels are gathered by the splat itself; every other dtype by one
        gather along ``src_index``, so integer labels stay exact; both on the
        tracker's device, as :meth:`splat`.  With ``inpaint`` = R > 0 (None:
        unlimited) holes within R cells of a covered cell take that cell's
        label, as :meth:`splat` describes; ``covered`` is the true coverage
        all the same."""
        if self.pos is None:
            raise ValueError("warp_labels() needs a step first")
        H, W = self.pos.shape[-2:]
        shape = tuple(labels.shape)
        if not (shape == (H, W) or (labels.dim() == 4 and shape[0] == 1 and shape[1] >= 1 and shape[2:] == (H, W))):
            raise ValueError(f"labels must be (H,W), (1,1,H,W) or (1,C,H,W) with H, W = {(H, W)}, got {shape}")
        lab = labels.to(self.pos.device).reshape(1, -1, H, W)
        if lab.dtype == torch.float32:
            _, covered, _, out = self.splat(lab, footprint=footprint, fill=float(fill), inpaint=inpaint)
            return out.reshape(shape), covered
        src, covered, _, _ = self.splat(None, footprint=footprint, inpaint=inpaint)
        got = lab.reshape(-1, H * W).index_select(1, src.reshape(-1).long().clamp_(min=0)).reshape(1, -1, H, W)
        hole = torch.full((), fill, dtype=lab.dtype, device=lab.device)
        return torch.where(covered if inpaint == 0 else src >= 0, got, hole).reshape(shape), covered

    def _image(self, what, image):
        """An image argument of stabilize() / warp_image(), checked, on the tracker's device."""
        if self.pos is None:
            raise ValueError(f"{what}() needs a step first")
        H, W = self.pos.shape[-2:]
        shape = tuple(image.shape)
        if not (image.dim() == 4 and shape[0] == 1 and shape[1] >= 1 and shape[2:] == (H, W)):
            raise ValueError(f"image must be (1,C,H,W) with H, W = {(H, W)}, got {shape}")
        if image.dtype not in (torch.float32, torch.uint8):
            raise ValueError(f"image must be float32 or uint8, got {image.dtype}")
        return image.to(self.pos.device)

    @torch.no_grad()
    def stabilize(self, image=None, fill=0):
        """The current frame seen from the first one: a motion-compensated view.
        image (1,C,H,W), fp32 or uint8, aligned with frame t (the frame itself,
        or a second modality recorded with it); None: the current frame as the
        tracker holds it, fp32 (on the GPU the static frame buffer,
        channels-last, read in place) -> (stab (1,C,H,W) of the image's dtype:
        at every pixel of frame 0 the image read bilinearly at the pixel's
        position in frame t, ``fill`` where it is not ok; ok (1,1,H,W) bool:
        the pixel is visible and its position is inside the frame).  This is
        ``ops.backward_warp(image, pos, valid=visible, fill=fill)``
        (csrc/backward_warp.hip on the GPU, an eager call on the current stream
        after the step's replay, without a host synchronisation; the ATen
        oracle on the CPU).  On the first frame it is the image itself.  ``pos``
        stays indexed by the pixels of frame 0 through a re-anchor, so this
        does too.  The tensors are the caller's own."""
        from ..ops import backward_warp
        if self.pos is None:
            raise ValueError("stabilize() needs a step first")
        image = self._st["frame"] if image is None else self._image("stabilize", image)
        return backward_warp(image, self.pos, valid=self.visible, fill=fill)

    @torch.no_grad()
    def warp_image(self, image, footprint: int = 2, inpaint: int | None = 0, fill=0):
        """Carry an image drawn on the first frame into the current one.
        image (1,C,H,W), fp32 or uint8, in the coordinates of frame 0 ->
        (warped (1,C,H,W) of the image's dtype, ok (1,1,H,W) bool): every cell
        of frame t reads the image bilinearly at ``inv_pos``, the cell's
        position in frame 0 that :meth:`splat` finds (``footprint`` and
        ``inpaint`` are its arguments), not by nearest neighbour as
        :meth:`warp_labels` does: ``ops.backward_warp(image, inv_pos,
        fill=fill)``.  A hole of the splat (NaN ``inv_pos``), or an in-painted
        cell whose rigid extension leaves the image, holds ``fill`` and is not
        ok.  On the GPU two or three eager calls on the current stream after the
        step's replay, without a host synchronisation.  The tensors are the
        caller's own."""
        from ..ops import backward_warp
        image = self._image("warp_image", image)
        inv_pos = self.splat(None, footprint=footprint, inpaint=inpaint)[2]
        return backward_warp(image, inv_pos, fill=fill)

    @torch.no_grad()
    def track(self, frames, labels=None, footprint: int = 2, fill=0, inpaint: int | None = 0):
        """frames (T,1,3,H,W) or a list of (1,3,H,W) -> (flows (T,2,H,W), the
        long-term flow 0 -> t of every pixel, visible (T,1,H,W) bool);
        ``flows[0] == 0``.  With ``labels`` of the first frame
        (:meth:`warp_labels`, which takes ``inpaint``) two more: the labels
        warped into every frame, (T,) + labels.shape, and covered (T,1,H,W)
        bool."""
        if len(frames) < 1:
            raise ValueError("track() needs at least one frame")
        self.reset()
        flows, vis, warped, cov = [], [], [], []
        for t in range(len(frames)):
            self.step(frames[t])
            flows.append(self.flow[0])
            vis.append(self.visible[0].clone())
            if labels is not None:
                w, c = self.warp_labels(labels, footprint=footprint, fill=fill, inpaint=inpaint)
                warped.append(w)
                cov.append(c[0])
        if labels is None:
            return torch.stack(flows), torch.stack(vis)
        return torch.stack(flows), torch.stack(vis), torch.stack(warped), torch.stack(cov)

    # ------------------------------------------------------------------- state
    def _history(self, dev, frame, points):
        """The planar state ring in place of the point tracker's history, and the constants of a frame's size."""
        from ..ops.reference import coords_grid
        R = self.L + 2
        H, W = frame.shape[-2:]
        return {"ring_pos": torch.zeros(R, 2, H, W, device=dev),
                "ring_score": torch.zeros(R, H, W, device=dev),
                "grid": coords_grid(1, H, W, device=dev).contiguous(),
                "minus": torch.full((1, 1, H, W), -1, dtype=torch.int32, device=dev)}

    def _choose(self, st, up):
        """Every pixel's choice among the K flow pairs, read from and written
        to the state ring in place."""
        from ..ops import dense_multi_flow_step
        K = self.K
        return dense_multi_flow_step(up[:K], up[K:], st["ring_pos"], st["ring_score"], st["idx"], st["active"],
                                     *self.fb_alpha, cand_err=self.want_cand_err)

    def _start(self, st, dev, frame, points):
        """The state of a sequence's first frame: the grid, score 0, in row 0
        (which the inactive slots name too) and in the anchor's row."""
        H, W = frame.shape[-2:]
        self._seed(st)
        self.pos = st["grid"].clone()
        self.visible = torch.ones(1, 1, H, W, dtype=torch.bool, device=dev)
        self.score = torch.zeros(1, 1, H, W, device=dev)
        self.fb_err = torch.zeros(1, 1, H, W, device=dev)
        self.delta = torch.zeros(1, 1, H, W, dtype=torch.int32, device=dev)
        self.anchor_pos, self.anchor_score, self.anchor_visible = self.pos, self.score, self.visible
        return self.pos

    def _seed(self, st):
        """The anchor's state: the grid with score 0 in row 0 and in the anchor's row of the state ring."""
        for row in (0, self.L + 1):
            st["ring_pos"][row].copy_(st["grid"][0])
            st["ring_score"][row].zero_()

    def _publish(self, pos, score, vis, delta, err, cand):
        """The attributes that describe the new frame: the graph's outputs
        themselves, or after a re-anchor their composition with the base."""
        self.anchor_pos, self.anchor_score, self.anchor_visible = pos, score, vis
        self.cand_err = cand
        if self._based:
            from ..ops import dense_compose
            st = self._st
            # on the GPU into static buffers, as the graph's outputs are; on the CPU every step has its own tensors
            pos, score, vis, delta, err = dense_compose(st["base_pos"], st["base_score"], pos, score, delta, err,
                                                        out=st["composed"] if pos.is_cuda else None)
        self.pos, self.score, self.visible = pos, score, vis
        self.delta, self.fb_err = delta, err
        return self.pos
