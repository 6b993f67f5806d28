"""Composition of two dense track fields, and the point form of reading one.
The rules and their ATen implementations are ops/reference.py: dense_compose
and dense_query, which run tensors on the CPU; tensors on the GPU go to
csrc/dense_compose.hip (one launch, one thread per pixel or per point), never
through eager ATen."""
from __future__ import annotations

import torch

from . import _ext
from . import reference as ref

_MAX_CELLS = 2 ** 31  # exclusive: a cell index is a 32-bit int in the kernels


def _field(name, pos, score, what="pos"):
    """(H, W) of a field, checked."""
    if pos.dim() != 4 or pos.shape[0] != 1 or pos.shape[1] != 2:
        raise ValueError(f"{name}: {what} must be (1,2,H,W), got {tuple(pos.shape)}")
    H, W = pos.shape[2:]
    if H < 2 or W < 2:
        raise ValueError(f"{name}: H, W >= 2 expected, got {(H, W)}")
    if H * W >= _MAX_CELLS:
        raise ValueError(f"{name}: H*W = {H * W} must be below 2^31")
    if tuple(score.shape) != (1, 1, H, W):
        raise ValueError(f"{name}: the score of {what} must be {(1, 1, H, W)}, got {tuple(score.shape)}")
    if pos.device.type not in ("cpu", "cuda"):
        raise NotImplementedError(f"{name}: no HIP kernel yet for {pos.device}; tensors on the CPU or the GPU expected")
    return H, W


def _same_device(name, pos, others):
    for what, t in others:
        if t.device != pos.device:
            raise ValueError(f"{name}: pos and {what} must be on the same device, got {pos.device} and {t.device}")


def dense_compose(base_pos: torch.Tensor, base_score: torch.Tensor, pos: torch.Tensor, score: torch.Tensor,
                  delta: torch.Tensor, fb_err: torch.Tensor, out=None):
    """base_pos (1,2,H,W), base_score (1,1,H,W): a dense track field anchor a
    -> frame r, as DenseMultiFlowTracker publishes ``pos`` and ``score``
    (finite iff visible); pos, score, delta (1,1,H,W) int32 and fb_err
    (1,1,H,W): the field r -> t of a tracker anchored on frame r.  -> (pos_c,
    score_c, visible_c (1,1,H,W) bool, delta_c int32, fb_err_c): the field a
    -> t, every anchor pixel's base position carried on by the bilinear sample
    of the inner field there (ops.dense_query's rule), its score the sum of
    the two, visible iff it was visible in both; ``delta`` and ``fb_err`` are
    the inner field's at the pixel nearest to the base position, -1 and +inf
    where not visible (the rule: ops/reference.py).  Float inputs of any
    float dtype or layout, on the CPU or the GPU.

    ``out``: five tensors to write into, contiguous, of the outputs' dtypes
    and shapes, on the inputs' device and none of them an input; they are
    returned.  On the GPU the call is one launch on the current stream without
    a host synchronisation; with ``out`` and contiguous fp32 / int32 inputs it
    allocates nothing and can be captured in a graph."""
    name = "dense_compose"
    H, W = _field(name, pos, score)
    if tuple(base_pos.shape) != (1, 2, H, W) or tuple(base_score.shape) != (1, 1, H, W):
        raise ValueError(f"{name}: base_pos and base_score must be {(1, 2, H, W)} and {(1, 1, H, W)}, got "
                         f"{tuple(base_pos.shape)} and {tuple(base_score.shape)}")
    if tuple(delta.shape) != (1, 1, H, W) or tuple(fb_err.shape) != (1, 1, H, W):
        raise ValueError(f"{name}: delta and fb_err must be {(1, 1, H, W)}, got {tuple(delta.shape)} and "
                         f"{tuple(fb_err.shape)}")
    if delta.dtype != torch.int32:
        raise ValueError(f"{name}: delta must be int32, got {delta.dtype}")
    for what, t in (("base_pos", base_pos), ("base_score", base_score), ("pos", pos), ("score", score),
                    ("fb_err", fb_err)):
        if not t.is_floating_point():
            raise ValueError(f"{name}: {what} must be a float tensor, got {t.dtype}")
    _same_device(name, pos, (("base_pos", base_pos), ("base_score", base_score), ("score", score), ("delta", delta),
                             ("fb_err", fb_err)))
    if out is not None:
        out = tuple(out)
        spec = (("pos", torch.float32, (1, 2, H, W)), ("score", torch.float32, (1, 1, H, W)),
                ("visible", torch.bool, (1, 1, H, W)), ("delta", torch.int32, (1, 1, H, W)),
                ("fb_err", torch.float32, (1, 1, H, W)))
        if len(out) != len(spec):
            raise ValueError(f"{name}: out must be (pos, score, visible, delta, fb_err), got {len(out)} tensors")
        for t, (what, dt, shape) in zip(out, spec):
            if t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous() or t.device != pos.device:
                raise ValueError(f"{name}: out {what} must be a contiguous {dt} tensor of shape {shape} on "
                                 f"{pos.device}, got {t.dtype} {tuple(t.shape)} on {t.device}")
    args = (base_pos.float().contiguous(), base_score.float().contiguous(), pos.float().contiguous(),
            score.float().contiguous(), delta.contiguous(), fb_err.float().contiguous())
    if pos.device.type == "cpu":
        res = ref.dense_compose(*args)
        if out is None:
            return res
        for o, r in zip(out, res):
            o.copy_(r)
        return out
    # a missing extension is an error, never a quiet run through eager ATen on the device
    _ext.load(raise_on_error=True)
    if out is None:
        dev = pos.device
        out = (torch.empty(1, 2, H, W, device=dev), torch.empty(1, 1, H, W, device=dev),
               torch.empty(1, 1, H, W, dtype=torch.bool, device=dev),
               torch.empty(1, 1, H, W, dtype=torch.int32, device=dev), torch.empty(1, 1, H, W, device=dev))
    torch.ops.raft_stir.dense_compose(*args, *out)
    return out


def dense_query(pos: torch.Tensor, score: torch.Tensor, points: torch.Tensor):
    """Read a dense track field at points of its anchor frame.  pos (1,2,H,W),
    score (1,1,H,W) (+inf: not visible), points (1,N,2) xy, N >= 0; any float
    dtype or layout, on the CPU or the GPU -> (positions (1,N,2) fp32, visible
    (1,N) bool, score (1,N) fp32): the bilinear sample of ``pos`` at the
    points, visible iff every pixel it is read from is, the score the worst of
    theirs; a point outside the frame or non-finite comes back unchanged, not
    visible, with score +inf (the rule: ops/reference.py: dense_query).  On the
    GPU one launch on the current stream, no host synchronisation."""
    name = "dense_query"
    H, W = _field(name, pos, score)
    if points.dim() != 3 or points.shape[0] != 1 or points.shape[2] != 2:
        raise ValueError(f"{name}: points must be (1,N,2), got {tuple(points.shape)}")
    N = points.shape[1]
    if N >= _MAX_CELLS:
        raise ValueError(f"{name}: N = {N} must be below 2^31")
    for what, t in (("pos", pos), ("score", score), ("points", points)):
        if not t.is_floating_point():
            raise ValueError(f"{name}: {what} must be a float tensor, got {t.dtype}")
    _same_device(name, pos, (("score", score), ("points", points)))
    p, s, q = pos.float().contiguous(), score.float().contiguous(), points.float().contiguous()
    if pos.device.type == "cpu":
        return ref.dense_query(p, s, q)
    _ext.load(raise_on_error=True)
    dev = pos.device
    out = torch.empty(1, N, 2, device=dev)
    visible = torch.empty(1, N, dtype=torch.bool, device=dev)
    out_score = torch.empty(1, N, device=dev)
    torch.ops.raft_stir.dense_query(p, s, q, out, visible, out_score)
    return out, visible, out_score
