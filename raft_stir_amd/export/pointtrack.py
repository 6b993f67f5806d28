"""STIR point tracker + TorchScript / ONNX export (reference rafttoonnx.py).

``RaftPointTrack(model).forward(pointlist (1,N,2) xy, image1, image2)``
    runs RAFT for ``NUMITERS`` (12) iterations in test mode, bilinearly samples
    the full-resolution flow at the points (grid_sample, align_corners=True)
    and returns ``pointlist + flow`` (1, N, 2)  (reference rafttoonnx.py:137-154).

Export (reference rafttoonnx.py:49-118, 156-223):
  * :func:`export_torchscript` -- ``torch.jit.trace`` of the tracker, saved and
    reloaded, with a parity check against eager;
  * :func:`export_onnx` -- opset 17, input names ``pointlist/image1/image2``,
    output ``end_points`` (or the bare model with ``image1/image2 ->
    flow_low/flow_up``), legacy TorchScript-based exporter (``dynamo=False``);
    optional onnxruntime parity check at atol=rtol=1e-2 when onnxruntime is
    importable (it is not in this image: parity unpinned there).
Tracing always takes the pure-ATen composite path of every op (ops/_ext.py
``_exporting``) so the graphs contain only standard operators, whichever
device the model lives on.

:class:`PointTrackServer` is the serving path on MI355X: the whole tracker
(encoders, 12 iterations, upsampling and point sampling) captured once in a
hipGraph per input shape and replayed per request with the HIP kernels.
:class:`SequenceTracker` follows points through a whole video on top of it:
one frame per step, each pair warm-started from the forward-interpolated flow
of the pair before (ops.forward_interpolate, csrc/forward_interp.hip); with
``fb_check`` it also reports a per-point visibility from a forward-backward
check of the two flow directions (ops.fb_track_points, csrc/fb_check.hip).
export/multiflow.py ``MultiFlowTracker`` tracks over several time spans at
once and finds a point again after it was lost.
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

NUMITERS = 12
POINTCOUNT = 32


def sample_points(flow_up: torch.Tensor, pointlist: torch.Tensor) -> torch.Tensor:
    """flow (1,2,H,W), points (1,N,2) xy pixels -> flow at points (1,N,2)."""
    H, W = flow_up.shape[-2:]
    g = pointlist.unsqueeze(2)  # (1,N,1,2)
    gx = 2 * g[..., :1] / (W - 1) - 1
    gy = 2 * g[..., 1:] / (H - 1) - 1
    s = F.grid_sample(flow_up, torch.cat([gx, gy], dim=-1), align_corners=True)  # (1,2,N,1)
    return s.squeeze(3).permute(0, 2, 1)


class RaftPointTrack(nn.Module):
    def __init__(self, model, iters: int = NUMITERS):
        super().__init__()
        self.model = model
        self.iters = iters

    def forward(self, pointlist, image1, image2):
        _, flow_up = self.model(image1, image2, iters=self.iters, test_mode=True)
        return pointlist + sample_points(flow_up.to(pointlist.dtype), pointlist)


class _FlowOnly(nn.Module):
    def __init__(self, model, iters):
        super().__init__()
        self.model = model
        self.iters = iters

    def forward(self, image1, image2):
        return self.model(image1, image2, iters=self.iters, test_mode=True)


def _reference_mode():
    from ..ops._ext import reference_mode
    return reference_mode()


@torch.no_grad()
def export_torchscript(tracker: nn.Module, example, path: str, check: bool = True,
                       atol: float = 1e-3):
    tracker.eval()
    with _reference_mode():
        traced = torch.jit.trace(tracker, example, check_trace=False)
        traced.save(path)
        loaded = torch.jit.load(path, map_location=example[0].device)
        if check:
            want = tracker(*example)
            got = loaded(*example)
            err = (want - got).abs().max().item()
            if err > atol:
                raise AssertionError(f"TorchScript parity failed: max|diff|={err}")
    return loaded


def onnx_available() -> bool:
    try:
        import onnx  # noqa: F401
        return True
    except Exception:
        return False


@torch.no_grad()
def export_onnx(module: nn.Module, example, path: str, input_names, output_names,
                opset: int = 17, check: bool = True, tol: float = 1e-2):
    module.eval()
    with _reference_mode():
        torch.onnx.export(module, example, path, export_params=True, opset_version=opset,
                          do_constant_folding=True, input_names=list(input_names),
                          output_names=list(output_names), verbose=False, dynamo=False)
    if check:
        try:
            import onnxruntime as ort
        except Exception:
            return None  # parity unpinned: onnxruntime absent
        sess = ort.InferenceSession(path, providers=["CPUExecutionProvider"])
        feeds = {n: t.detach().cpu().numpy() for n, t in zip(input_names, example)}
        outs = sess.run(None, feeds)
        with _reference_mode():
            want = module(*example)
        want = want if isinstance(want, (tuple, list)) else (want,)
        for w, o in zip(want, outs):
            if not torch.allclose(w.cpu(), torch.from_numpy(o), atol=tol, rtol=tol):
                raise AssertionError("ONNX model not close to the PyTorch model")
    return path


def export_pointtrack(model, path_prefix="raft_pointtrackSTIR", size=(512, 640),
                      npoints=POINTCOUNT, device=None, onnx=True, iters=NUMITERS):
    """Export the STIR tracker like reference convertmodelpointtrack:
    ``<prefix>.pt`` (TorchScript) and ``<prefix>.onnx`` (when onnx exists)."""
    device = device or next(model.parameters()).device
    tracker = RaftPointTrack(model, iters=iters).to(device).eval()
    H, W = size
    g = torch.Generator().manual_seed(0)
    image1 = (torch.rand(1, 3, H, W, generator=g) * 255).to(device)
    image2 = (torch.rand(1, 3, H, W, generator=g) * 255).to(device)
    points = (torch.rand(1, npoints, 2, generator=g) * min(H, W)).to(device)
    example = (points, image1, image2)
    out = {"torchscript": path_prefix + ".pt"}
    export_torchscript(tracker, example, out["torchscript"])
    if onnx and onnx_available():
        export_onnx(tracker, example, path_prefix + ".onnx", ["pointlist", "image1", "image2"],
                    ["end_points"])
        out["onnx"] = path_prefix + ".onnx"
    return out


def check_step_inputs(frame, seq_shape, points):
    """What every tracker's ``step`` asks of its inputs.  ``seq_shape``: the
    frame shape of the running sequence, None before its first frame;
    ``points`` may be None."""
    if frame.dim() != 4 or frame.shape[0] != 1 or frame.shape[1] != 3:
        raise ValueError(f"frame must be (1,3,H,W), got {tuple(frame.shape)}")
    if frame.shape[-2] % 8 or frame.shape[-1] % 8:
        raise ValueError(f"frame height and width must be multiples of 8, got {tuple(frame.shape[-2:])}")
    if seq_shape is not None and seq_shape != tuple(frame.shape):
        raise ValueError(f"frame shape changed within a sequence: {seq_shape} -> "
                         f"{tuple(frame.shape)} (call reset())")
    if points is not None and (points.dim() != 3 or points.shape[0] != 1 or points.shape[2] != 2):
        raise ValueError(f"points must be (1,N,2), got {tuple(points.shape)}")


def check_tracker_options(model, fb_alpha, cache_features):
    """-> (fb_alpha as two floats, cache_features as a bool), both checked."""
    alpha = (float(fb_alpha[0]), float(fb_alpha[1]))
    if not (alpha[0] >= 0 and alpha[1] >= 0):
        raise ValueError(f"fb_alpha must be two numbers >= 0, got {fb_alpha}")
    if cache_features and not (hasattr(model, "encode") and hasattr(model, "refine")):
        raise ValueError("cache_features=True needs a model with encode() and refine()")
    return alpha, bool(cache_features)


def encode_first(model, ft, R, rows, K):
    """``cache_features``, the first frame of a sequence: ``ft["frame"]``
    encoded into ``rows`` of the feature ring.  The first call allocates the
    ring of R rows and the gathered batch of K pairs from the features'
    shapes and dtype."""
    from ..ops import to_nhwc
    f, c = model.encode(ft["frame"])
    f, c = to_nhwc(f), to_nhwc(c)
    if "ring_f" not in ft:
        if f.dtype != c.dtype:
            raise ValueError(f"cache_features: encode() returned {f.dtype} features and {c.dtype} context")
        for name, like, n in (("ring_f", f, R), ("ring_c", c, R), ("x", f, 3 * K), ("ctx", c, 2 * K)):
            ft[name] = like.new_zeros((n,) + tuple(like.shape[1:]))
    for row in rows:
        ft["ring_f"][row].copy_(f[0])
        ft["ring_c"][row].copy_(c[0])


def encode_and_gather(model, ft):
    """``cache_features``, every later frame: ``ft["frame"]`` encoded at batch
    1, stored in the ring row ``ft["idx"][-1]`` and gathered with the rows
    ``ft["idx"][:-1]`` -> (x, ctx) for ``model.refine`` (ops.feature_ring_step)."""
    from ..ops import feature_ring_step, from_nhwc, to_nhwc
    f, c = model.encode(ft["frame"])
    feature_ring_step(ft["ring_f"], ft["ring_c"], to_nhwc(f), to_nhwc(c), ft["idx"], ft["x"], ft["ctx"])
    return from_nhwc(ft["x"]), from_nhwc(ft["ctx"])


def image_buffer(shape, dev):
    """A static image buffer: channels-last on the GPU, as the model's kernels read it."""
    fmt = torch.channels_last if dev.type == "cuda" else torch.contiguous_format
    return torch.zeros(tuple(shape), device=dev).contiguous(memory_format=fmt)


class PointTrackServer:
    """Graphed STIR point tracker for serving on the GPU (HIP kernels)."""

    def __init__(self, model, iters: int = NUMITERS):
        self.model = model.eval()
        self.iters = iters
        self.graphs = {}

    @torch.no_grad()
    def __call__(self, pointlist, image1, image2):
        dev = next(self.model.parameters()).device
        if dev.type != "cuda":
            return RaftPointTrack(self.model, self.iters)(pointlist, image1, image2)
        key = (tuple(image1.shape), tuple(pointlist.shape))
        st = self.graphs.get(key)
        if st is None:
            st = self._capture(dev, pointlist, image1, image2)
            self.graphs[key] = st
        st["p"].copy_(pointlist)
        st["i1"].copy_(image1)
        st["i2"].copy_(image2)
        st["graph"].replay()
        return st["out"].clone()

    def _capture(self, dev, pointlist, image1, image2):
        from ..runtime.graph import capture
        p = pointlist.detach().clone()
        i1 = image1.detach().clone().contiguous(memory_format=torch.channels_last)
        i2 = image2.detach().clone().contiguous(memory_format=torch.channels_last)
        tracker = RaftPointTrack(self.model, self.iters)
        g, out = capture(dev, lambda: tracker(p, i1, i2))
        return {"graph": g, "p": p, "i1": i1, "i2": i2, "out": out}


class SequenceTracker:
    """Follow points through a video, one frame per :meth:`step`.

    ``step(frame, points)`` on the first frame stores both and returns the
    points unchanged; every later ``step(frame)`` returns the (1,N,2) positions
    in the new frame::

        flow_low, flow_up = model(prev, frame, iters, flow_init=init, test_mode=True)
        points = points + sample_points(flow_up, points)
        init = ops.forward_interpolate(flow_low)      # warm_start; zeros without

    The first pair of a sequence starts from zeros.  After a step,
    ``flow_low``, ``flow_up``, ``flow_init`` (the init that step used) and
    ``next_init`` (the init the next step will use) are readable until the next
    step.

    On the GPU the model forward, the point sampling and the forward
    interpolation are one captured hipGraph per (frame shape, N) over static
    buffers.  A frame is uploaded once: between steps the ``image2`` buffer is
    copied into ``image1`` on the device (the two belong to the frame shape,
    so N may change within a sequence), and the new init into the
    ``flow_init`` buffer.  With frames and points already on the device no step
    synchronises with the host.  On a CPU model the same step runs on the same
    buffers, eagerly.

    ``fb_check=True`` adds a visibility to every position.  A step is then::

        lo, up = model(prev, frame, iters, flow_init=init, test_mode=True, bidirectional=True)
        points, fb_err, visible = ops.fb_track_points(up[0:1], up[1:2], points, *fb_alpha)
        init = sgn * ops.forward_interpolate(sgn * lo)     # sgn = +1 forward, -1 backward

    still one graph per (frame shape, N).  ``init`` holds both directions,
    (2,2,h,w).  The backward field's warm start moves every sample against its
    own vector and carries the vector along: the same constant-velocity
    assumption as the forward one.  After a step ``fb_err`` (1,N) is the
    distance by which each point misses its start on the way back (+inf for a
    point that left the image) and ``visible`` (1,N) the check's verdict; after
    the first step of a sequence they are zeros and all true.  ``visible`` is
    per step, not sticky: what to do with a lost point is the caller's policy.
    ``flow_bw_low``, ``flow_bw_up``, ``flow_bw_init`` and ``next_bw_init`` are
    the backward direction's counterparts of the forward attributes, which
    stay (1,2,..) tensors.  :meth:`fb_map` gives the dense check of the last
    step's fields.

    ``cache_features=True`` encodes every frame once instead of twice (as
    ``image2``, and one step later as ``image1``): the tracker keeps
    ``model.encode``'s output of the previous frame in a two-row ring on the
    device and a step is ``model.encode(frame)`` at batch 1,
    ``ops.feature_ring_step`` (store the new features, gather the pair) and
    ``model.refine`` on the gathered features, with or without ``fb_check``;
    the rest of the step is the same.  Still one graph per (frame shape, N),
    beside a small one per frame shape that encodes a sequence's first frame;
    the ring belongs to the frame shape, so N may change within a sequence as
    without the cache.  The flows
    differ from the uncached tracker's only by the batch size at which the
    encoders ran.
    """

    def __init__(self, model, iters: int = NUMITERS, warm_start: bool = True, fb_check: bool = False,
                 fb_alpha=(0.01, 0.5), cache_features: bool = False):
        self.model = model.eval()
        self.iters = iters
        self.warm_start = warm_start
        self.fb_check = fb_check
        self.fb_alpha, self.cache_features = check_tracker_options(model, fb_alpha, cache_features)
        self.graphs = {}
        self._frames = {}  # frame shape -> the frame buffers or the feature ring, and the zero init
        self._wkey = None
        self.reset()

    def reset(self):
        """Forget the previous frame, the points and the init."""
        self._t = 0            # frames seen (cache_features: frame t lives in ring row t % 2)
        self._next = None      # the init of the next step: (1,2,h,w), or (2,2,h,w) with fb_check
        self._shape = None     # the frame shape of the running sequence
        self.points = None
        self.flow_low = self.flow_up = self.flow_init = self.next_init = None
        self.flow_bw_low = self.flow_bw_up = self.flow_bw_init = self.next_bw_init = None
        self.fb_err = self.visible = None

    @torch.no_grad()
    def step(self, frame, points=None):
        """The feature ring or the pair of frame buffers belongs to the frame
        shape, so that it outlives a change of N within a sequence; the step's
        graph and its points and init buffers belong to (frame shape, N)."""
        from ..runtime.graph import capture
        from ..runtime.weights import refresh_if_moved
        check_step_inputs(frame, self._shape, points)
        if points is None:
            points = self.points
        if points is None:
            raise ValueError("the first step of a sequence needs points")
        dev = next(self.model.parameters()).device
        gpu = dev.type == "cuda"
        if gpu:
            self._wkey = refresh_if_moved(self.model, self._wkey)
        shape = tuple(frame.shape)
        ft = self._frames.get(shape)
        if ft is None:
            ft = self._frames[shape] = self._frame_state(dev, frame)
        if self._t == 0:
            ft["frame"].copy_(frame)
            if self.cache_features:  # encoded into ring row 0, on the GPU by a small graph of its own
                if gpu and ft["graph0"] is None:
                    ft["graph0"], _ = capture(dev, lambda: encode_first(self.model, ft, 2, (0,), 1))
                ft["graph0"].replay() if gpu else encode_first(self.model, ft, 2, (0,), 1)
            self._shape, self._next, self._t = shape, ft["zero"], 1
            return self._first(points.to(dev, torch.float32).clone())
        key = (shape, points.shape[1]) + (("cache_features",) if self.cache_features else ())
        st = self.graphs.get(key)
        if st is None:
            st = self.graphs[key] = {"p": torch.zeros(1, points.shape[1], 2, device=dev), "frames": ft,
                                     "init": torch.zeros_like(ft["zero"]), "sgn": self._sgn(dev), "graph": None}
        if self.cache_features:
            ft["idx"].copy_(ft["idx_table"][(self._t - 1) % 2])
        else:
            ft["prev"].copy_(ft["frame"])  # on the device: a frame is uploaded once
        ft["frame"].copy_(frame)
        st["p"].copy_(points)
        st["init"].copy_(self._next)
        if gpu and st["graph"] is None:
            # captured on the step's own inputs: the warm-up runs write the ring row that this step writes
            st["graph"], st["outs"] = capture(dev, lambda: self._run(st))
        if gpu:
            st["graph"].replay()
            lo, up, out, err, ok, nxt = st["outs"]
        else:
            lo, up, out, err, ok, nxt = self._run(st)
        self._t += 1
        self.points = out.clone()
        if self.fb_check:
            self.fb_err, self.visible = err.clone(), ok.clone()
        self._publish(st["init"], lo, up, nxt if self.warm_start else ft["zero"])
        return self.points

    @torch.no_grad()
    def track(self, frames, points, return_visibility: bool = False):
        """frames (T,1,3,H,W) or a list of (1,3,H,W); points (1,N,2) in the
        first frame -> (T,N,2) trajectory, ``traj[0] == points``.  With
        ``return_visibility`` (an ``fb_check`` tracker only):
        ``(traj, visible (T,N) bool, fb_err (T,N))``."""
        if return_visibility and not self.fb_check:
            raise ValueError("return_visibility=True needs a tracker built with fb_check=True")
        self.reset()
        traj, vis, err = [], [], []
        for t in range(len(frames)):
            traj.append(self.step(frames[t], points if t == 0 else None)[0].clone())
            if return_visibility:
                vis.append(self.visible[0].clone())
                err.append(self.fb_err[0].clone())
        if return_visibility:
            return torch.stack(traj), torch.stack(vis), torch.stack(err)
        return torch.stack(traj)

    def fb_map(self):
        """Dense forward-backward check of the last step's full-resolution
        fields: (err (1,1,H,W), ok (1,1,H,W) bool).  On demand, outside the graph."""
        if not self.fb_check:
            raise ValueError("fb_map() needs a tracker built with fb_check=True")
        if self.flow_up is None:
            raise ValueError("fb_map() needs a step on a second frame first")
        from ..ops import fb_consistency
        return fb_consistency(self.flow_up, self.flow_bw_up, *self.fb_alpha)

    def _first(self, points):
        """Bookkeeping of the first step of a sequence; ``self._next`` is set."""
        self.points = points
        self.next_init = self._next[0:1]
        if self.fb_check:
            self.next_bw_init = self._next[1:2]
            self.fb_err = torch.zeros(points.shape[:2], device=points.device)
            self.visible = torch.ones(points.shape[:2], dtype=torch.bool, device=points.device)
        return self.points

    def _publish(self, init, lo, up, nxt):
        """The per-step attributes: views of the (1 or 2, 2, ..) tensors."""
        self._next = nxt
        self.flow_init, self.flow_low, self.flow_up, self.next_init = init[0:1], lo[0:1], up[0:1], nxt[0:1]
        if self.fb_check:
            self.flow_bw_init, self.flow_bw_low, self.flow_bw_up, self.next_bw_init = (
                init[1:2], lo[1:2], up[1:2], nxt[1:2])

    def _frame_state(self, dev, frame):
        """What belongs to a frame shape: the new frame's buffer, one zero init
        (never written: both directions in one tensor with fb_check, forward
        first), and the previous frame's buffer or, with ``cache_features``,
        what the feature ring needs (the ring itself comes with its first frame)."""
        ft = {"frame": image_buffer(frame.shape, dev),
              "zero": torch.zeros(2 if self.fb_check else 1, 2, frame.shape[-2] // 8, frame.shape[-1] // 8, device=dev)}
        if self.cache_features:
            # [source row, row written] of an odd and of an even step: frame t lives in row t % 2
            ft.update({"idx_table": torch.tensor([[0, 1], [1, 0]], dtype=torch.int32, device=dev),
                       "idx": torch.tensor([0, 1], dtype=torch.int32, device=dev), "graph0": None})
        else:
            ft["prev"] = torch.zeros_like(ft["frame"])
        return ft

    def _run(self, st):
        """One pair on the static buffers: (flow_low, flow_up, new points,
        fb_err, visible, next init).  The two modes differ in how the flows
        are obtained only."""
        ft = st["frames"]
        if self.cache_features:
            x, ctx = encode_and_gather(self.model, ft)
            if self.fb_check:
                lo, up = self.model.refine(x[:2], x[1:], ctx, iters=self.iters, flow_init=st["init"])
            else:
                lo, up = self.model.refine(x[0:1], x[1:2], ctx[0:1], iters=self.iters, flow_init=st["init"])
        elif self.fb_check:
            lo, up = self.model(ft["prev"], ft["frame"], iters=self.iters, flow_init=st["init"], test_mode=True,
                                bidirectional=True)
        else:
            lo, up = self.model(ft["prev"], ft["frame"], iters=self.iters, flow_init=st["init"], test_mode=True)
        return self._follow(lo, up, st["p"], st["sgn"])

    def _follow(self, lo, up, p, sgn):
        """The points through the flows of one pair, and the next init."""
        from ..ops import fb_track_points, forward_interpolate
        if not self.fb_check:
            out = p + sample_points(up.to(p.dtype), p)
            return lo, up, out, None, None, (forward_interpolate(lo) if self.warm_start else None)
        out, err, ok = fb_track_points(up[0:1], up[1:2], p, *self.fb_alpha)
        # the backward field moves against its own vectors; negation is exact
        nxt = sgn * forward_interpolate(sgn * lo) if self.warm_start else None
        return lo, up, out, err, ok, nxt

    def _sgn(self, dev):
        return torch.tensor([1.0, -1.0], device=dev).view(2, 1, 1, 1) if self.fb_check else None
