"""Feature ring of the trackers that encode a frame once: store the new
frame's features and assemble the refinement batch in one launch
(csrc/feat_ring.hip on GPU, ATen index ops on CPU and while tracing)."""
from __future__ import annotations

import torch

from . import _ext
from . import reference as ref
from .multi_flow import MAX_SLOTS


def feature_ring_step(ring_f: torch.Tensor, ring_c: torch.Tensor, f_new: torch.Tensor, c_new: torch.Tensor,
                      idx: torch.Tensor, x: torch.Tensor, ctx: torch.Tensor) -> None:
    """ring_f (R,h,w,C), ring_c (R,h,w,Cc), f_new (1,h,w,C), c_new (1,h,w,Cc),
    x (3K,h,w,C), ctx (2K,h,w,Cc): contiguous, one dtype (bf16 or fp32 on the
    GPU), no two of them overlapping in memory; idx (K+1,) int32 on their
    device, never read on the host: the K source rows, then the row to write.
    In place (the rule: ops/reference.py)::

        ring_f[dst] = f_new;  x[k] = ring_f[src[k]];  x[K+k] = f_new;  x[2K+k] = x[k]
        ring_c[dst] = c_new;  ctx[k] = ring_c[src[k]];  ctx[K+k] = c_new

    ``x[:2K]`` and ``x[K:]`` are then fmap1 and fmap2 of a bidirectional pass
    over the K pairs (stored frame, new frame).  Every index is clamped to
    [0, R-1]; a source equal to the row written reads the new features."""
    name = "feature_ring_step"
    if ring_f.dim() != 4 or ring_c.dim() != 4 or ring_f.shape[:3] != ring_c.shape[:3]:
        raise ValueError(f"{name}: ring_f (R,h,w,C) and ring_c (R,h,w,Cc) expected, got {tuple(ring_f.shape)} "
                         f"and {tuple(ring_c.shape)}")
    R, h, w, C = ring_f.shape
    Cc = ring_c.shape[3]
    if idx.dim() != 1 or not 1 <= idx.shape[0] - 1 <= MAX_SLOTS or idx.dtype != torch.int32:
        raise ValueError(f"{name}: idx must be int32 (K+1,) with 1 <= K <= {MAX_SLOTS}, got {idx.dtype} "
                         f"{tuple(idx.shape)}")
    K = idx.shape[0] - 1
    for what, t, shape in (("f_new", f_new, (1, h, w, C)), ("c_new", c_new, (1, h, w, Cc)),
                           ("x", x, (3 * K, h, w, C)), ("ctx", ctx, (2 * K, h, w, Cc))):
        if tuple(t.shape) != shape:
            raise ValueError(f"{name}: {what} must be {shape}, got {tuple(t.shape)}")
    if _ext.use_hip(ring_f):
        torch.ops.raft_stir.feature_ring_step(ring_f, ring_c, f_new, c_new, idx, x, ctx)
    else:
        ref.feature_ring_step(ring_f, ring_c, f_new, c_new, idx, x, ctx)
